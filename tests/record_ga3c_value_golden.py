#!/usr/bin/env python3
"""tests/record_ga3c_value_golden.py -- RECORDER, not a test (no test imports it).  The value head of the GA3C-CADRL network
from the checkpoints' OWN graphs: oracle/tf_graph_exec.predict on the three reference checkpoints over the 1 024 recorded
inputs of tests/golden/ga3c_graph.npz ("X"), fetching `Squeeze` (NetworkVPCore.v, GA3C_CADRL/network.py:74) next to
`logits_p/BiasAdd`.  Writes tests/golden/ga3c_value.npz: value_<key> float32 [1024], the keys those of logits_<key> in
ga3c_graph.npz.  On the way it asserts that the logits it gets are the committed golden's, byte for byte -- the value is
recorded from the very evaluation the logits golden stands for.

Works only where the reference checkout is present (CA_REFERENCE_ROOT, default /root/reference); its output is committed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("CA_REFERENCE_ROOT", "/root/reference")
CKPT = os.path.join(REF, "gym_collision_avoidance", "envs", "policies", "GA3C_CADRL", "checkpoints")
SHIPPED = {"IROS18": "network_01900000", "run-20190727_015942-jzuhlntn": "network_01490000",
           "run-20190727_192048-qedrf08y": "network_01900000"}
OUT = os.path.join(HERE, "golden", "ga3c_value.npz")


def main():
    sys.path.insert(0, REPO)
    from oracle import tf_graph_exec as tg
    with np.load(os.path.join(HERE, "golden", "ga3c_graph.npz")) as z:
        golden = {k: z[k] for k in z.files}
    x = golden["X"]
    out = {}
    for run, name in SHIPPED.items():
        key = run.replace("-", "_")
        (logits, value), _ = tg.predict(os.path.join(CKPT, run, name), x, fetches=("logits_p/BiasAdd", "Squeeze"))
        logits, value = np.asarray(logits, np.float32), np.asarray(value, np.float32)
        assert logits.tobytes() == golden["logits_" + key].tobytes(), "%s: the logits differ from the committed golden" % run
        assert value.shape == (x.shape[0],), value.shape
        out["value_" + key] = value
        print("%s/%s: value %s, range %.3f .. %.3f" % (run, name, value.shape, value.min(), value.max()))
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
