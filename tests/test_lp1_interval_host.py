"""lp1_interval_pair (csrc/cagpu_lp1.inc), the interval update of the 1-D programmes, against the expression it replaced, bit
for bit, on the host.

tests/lp1_interval_check.cpp includes the rule as the kernels do (plain C++ between two macros) next to a verbatim copy of
the earlier text of p2b_round -- candidates built against +-inf, folded with two comparisons, then applied -- and compares
the two (t_lo, t_hi) words on
  * a full grid of special values in every float slot: +-0, +-1 (equal candidates, ties between t_hi, line m and line m + 1),
    values a float apart, +-inf, NaN, denominators on both sides of +-kRvoEps and exactly at it, all four (use0, use1);
  * 2^21 random tuples: half of them random bit patterns (every class of float, NaN payloads included), half drawn from a
    small set of values so that ties are common.
The program is stand-alone (its own main) and is built with -fsanitize=address,undefined where the host compiler has the
runtimes; nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "lp1_interval_check.cpp")
CSRC = os.path.join(REPO, "gym_collision_avoidance_amd", "csrc")


def _compiler():
    for c in ("g++", "clang++", "c++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("lp1") / "lp1_interval_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", out]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitised = r.returncode == 0
    if not sanitised:      # (a compiler without the sanitizer runtimes: the comparison itself does not depend on them)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out, sanitised


def test_interval_pair_matches_the_earlier_expression_bit_for_bit(program):
    exe, sanitised = program
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    print("sanitised build: %s" % sanitised)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("lp1-interval")][-1].split()
    stats = dict(zip(line[1::2], line[2::2]))
    assert int(stats["differing"]) == 0
    assert int(stats["random"]) >= 1000000 and int(stats["grid"]) > 100000
    # the cases the rule has to get right were really there
    for k in ("nan_tt0_present", "ties", "den_at_eps", "use1_false", "changed"):
        assert int(stats[k]) > 0, k


def test_the_rule_is_part_of_the_library_sources():
    from gym_collision_avoidance_amd import build_native
    assert os.path.join(CSRC, "cagpu_lp1.inc") in build_native.source_files()
    text = open(os.path.join(CSRC, "cagpu_pipe.inc")).read()
    assert "lp1_interval_pair(" in text
