#!/usr/bin/env python3
"""oracle/gen_reference_digests.py -- TEST INFRASTRUCTURE.   python oracle/gen_reference_digests.py <reference checkout>

Records tests/golden_util.digest() of reference files that the tests compare shipped data against, so that the comparison
runs where the reference is absent: the CARRL fixture pickles (envs/test_cases/2_agents_500_cases_carrl*.p, loaded like
test_cases.py:618-622 loads them) and the IROS18 GA3C-CADRL checkpoint as read by the package's TF-free reader
(network.read_checkpoint), one digest per tensor.  Output: tests/golden/reference_digests.json (committed)."""
import json
import os
import pickle
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from gym_collision_avoidance_amd.envs.policies.GA3C_CADRL import network  # noqa: E402
from tests.golden_util import GOLD, digest  # noqa: E402


def main(ref):
    envs = os.path.join(ref, "gym_collision_avoidance", "envs")
    out = {"carrl": {}}
    for name in ["2_agents_500_cases_carrl.p"] + ["2_agents_500_cases_carrl_seed%03d.p" % k for k in range(5)]:
        with open(os.path.join(envs, "test_cases", name), "rb") as f:
            out["carrl"][name] = digest(pickle.load(f, encoding="latin1"))
    raw = network.read_checkpoint(os.path.join(envs, "policies", "GA3C_CADRL", "checkpoints", "IROS18", "network_01900000"))
    out["ga3c_iros18_checkpoint"] = {k: digest([raw[k]]) for k in sorted(raw)}
    with open(os.path.join(GOLD, "reference_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
