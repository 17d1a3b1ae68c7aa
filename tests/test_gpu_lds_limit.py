"""The dynamic-LDS limit of a kernel whose LDS varies per call (raise_lds, csrc/cagpu_launch.inc): a launch above the 48 KiB
default needs the limit of its (kernel, device) pair raised first, a later launch that needs more needs it raised AGAIN,
and a smaller one afterwards needs nothing.  In a fresh child process, so that no other test has raised a limit first
(the marks live as long as the library); the child is this file run as a module.

  * scan_kernel: 2 envs x 2 agents, 16 beams, maps of 160^2, 240^2 and 340^2 cells, scanned in the order small, middle,
    large, middle; every history equals tests/laserscan_ref.py on every decided beam, as tests/test_gpu_laserscan_edges.py
    compares (its _Judge).
  * ca_kernel: 2 envs of 50, 64 and 50 agents; every reset and step equals the oracle as tests/test_gpu_parity.py compares
    a re-injected step.  Both counts run the same instantiation, ca_kernel<512, false, 0, false, false, 0>, with an `lds=`
    above 48 KiB (71200 and 111440 bytes): the limit is raised, raised again, and then left alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

KIB = 1024
# laserscan_impl's total for N = 2 agents and 16 beams: the byte grid with its border of 8 cells, (rows + 16) * pitch(cols + 16),
# + 2 * 120 (agents) + 16 * 16 (beams) + 1024 + 32 + 4 * 512 (tables, history staging) = grid + 3600 bytes
#   160 x 160 cells:  30976 + 3600 =  34576   in (0, 48 KiB]
#   240 x 240 cells:  65536 + 3600 =  69136   in (48 KiB, 96 KiB]
#   340 x 340 cells: 126736 + 3600 = 130336   in (96 KiB, 160 KiB]
# (a byte per cell, csrc/cagpu_scan.inc: 400^2 cells and more do not fit the 160 KiB of a workgroup at all)
SCAN_MAPS = [(160, 34576), (240, 69136), (340, 130336)]
SCAN_ORDER = [0, 1, 2, 1]
STEP_AGENTS = [50, 64, 50]


def scan_lds_bytes(side, N=2, beams=16):
    pitch = (side + 16 + 3) & ~3
    grid = ((side + 16) * pitch + 15) & ~15
    return grid + N * (4 * 8 + 2 * 8 + 3 * 4 + 2 * 8 + 2 * 8 + 3 * 4 + 4 * 4) + beams * 16 + 256 * 4 + 32 + 4 * 512


def scan_scene(side):
    """2 envs x 2 agents in and around a side x side map of 0.1 m cells with walls and scattered cells, 16 beams over +-pi/2"""
    from tests import laserscan_scenes as scenes
    return scenes._random("lds_%d" % side, 700 + side, side, side, 0.1, 0.1, 6.0, 16, -np.pi / 2, np.pi / 2, E=2, N=2, H=2)


def _scans():
    from tests import test_gpu_laserscan_edges as edges
    assert [scan_lds_bytes(side) for side, _ in SCAN_MAPS] == [total for _, total in SCAN_MAPS]
    assert SCAN_MAPS[0][1] <= 48 * KIB < SCAN_MAPS[1][1] <= 96 * KIB < SCAN_MAPS[2][1] <= 160 * KIB
    runs = []
    for side, _ in SCAN_MAPS:
        sc = scan_scene(side)
        sim = edges._sim(sc)
        runs.append((sc, edges._Judge(sim, sc)))
    for k, i in enumerate(SCAN_ORDER):
        sc, judge = runs[i]
        got = judge.scan("scan %d (%d x %d cells)" % (k, sc.rows, sc.cols))
        assert (got != edges.lref.NOTHING).any(), sc.name
    for sc, judge in runs:
        judge.finish()


def _steps():
    from tests import test_gpu_parity as par
    nat, core, orc = par._mods()
    lds = []
    for k, N in enumerate(STEP_AGENTS):
        E = 2
        rng = np.random.default_rng(10 * N + k)
        o, g = par._pair(E, N, 3)
        o.s["policy"][:] = orc.POL_RVO
        g.set_plugins(nat.POL_RVO)
        cases = np.zeros((E, N, 6))
        cases[..., 0:2] = rng.uniform(-8, 8, (E, N, 2))
        cases[..., 2:4] = rng.uniform(-8, 8, (E, N, 2))
        cases[..., 4] = rng.uniform(0.5, 2.0, (E, N))
        cases[..., 5] = rng.uniform(0.2, 0.5, (E, N))
        o.reset(cases)
        g.reset(cases)
        par._compare_reset(o, g)
        for t in range(2):
            par._upload(o, g)
            o.step()
            g.step()
            par._compare(o, g, what="launch %d, N=%d, step %d" % (k, N, t))
        kern = nat.lib().cagpu_last_kernel().decode()
        print(kern)
        assert kern.startswith("ca_kernel<512, false, 0, false, false, 0> grid=2 "), kern
        lds.append(int(re.search(r" lds=(\d+) ", kern).group(1)))
    assert 48 * KIB < lds[0] < lds[1] and lds[2] == lds[0], lds     # raised, raised again, then within the mark
    assert nat.device_faults() == 0


def _child():
    assert torch.cuda.is_available()
    _scans()
    _steps()
    print("lds limit ok")


def test_limit_is_raised_again_when_a_later_launch_needs_more():
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_lds_limit"], cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"lds limit ok" in r.stdout, r.stdout.decode()[-4000:]


if __name__ == "__main__":
    _child()
