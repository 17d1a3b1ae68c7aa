"""bench.py --dump-outputs: what the last timed step handed its caller, as float32 .npy files.  The steps computed before
the dump depend on the arguments alone -- the time-based warm-up runs on a snapshot of the simulator that is put back
afterwards -- so two runs that differ only in --min-warm-seconds write the same arrays, for every workload; and the files
stay within 64 MB where the outputs are larger (crowd50_laser at 4096 envs: a seeded sample of envs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENV_DROP = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GYM_CONFIG_CLASS", "GYM_CONFIG_PATH")


def _bench(out, args, warm_s):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--min-warm-seconds", str(warm_s),
           "--dump-outputs", str(out)] + args
    env = {k: v for k, v in os.environ.items() if k not in _ENV_DROP}
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("workload, args", [
    ("rvo10", ["--envs", "256", "--steps", "20", "--warmup", "5"]),
    ("ga3c20", ["--envs", "256", "--steps", "20", "--warmup", "5"]),
    ("crowd50_laser", ["--steps", "10", "--warmup", "2"]),
])
def test_bench_dump_does_not_depend_on_the_clock(tmp_path, workload, args):
    a, b = tmp_path / "a", tmp_path / "b"
    la = _bench(a, ["--workload", workload] + args, 0.05)
    lb = _bench(b, ["--workload", workload] + args, 0.4)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"obs.npy", "rewards.npy", "done.npy", "game_over.npy"} <= set(names)
    assert ("laserscan.npy" in names) == (workload == "crowd50_laser")
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype == np.float32 and x.shape[0] == la["dump_outputs"]["envs"], f
        assert np.array_equal(x, y), "%s differs between --min-warm-seconds 0.05 and 0.4" % f
    assert sum(os.path.getsize(a / f) for f in names) <= 64 * 10 ** 6
    da, db = dict(la["dump_outputs"]), dict(lb["dump_outputs"])
    assert da.pop("dir") == str(a) and db.pop("dir") == str(b) and da == db
    assert la["steps"] == lb["steps"] == int(args[args.index("--steps") + 1])
    if workload == "crowd50_laser":   # 4096 x 50 observations + scans exceed the budget: the seeded env sample
        assert da["of_envs"] == 4096 and 0 < da["envs"] < 4096 and da["sample"]
    else:
        assert da["envs"] == da["of_envs"] == 256 and da["sample"] is None
