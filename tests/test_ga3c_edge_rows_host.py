"""tests/ga3c_edge_rows.py and tests/ga3c_f64_ref.py held to what they promise, without a GPU: the tile plan covers every
row once, every laid-out batch holds the kernel variants it is meant to drive, the edge classes are what their labels
say, and numpy's float32 network (tests/ga3c_value_ref) stays within the project's bar (rtol 1e-4 / atol 2e-4) of the
float64 reference on every finite class -- so that the same bar is a fair demand on the kernel in
tests/test_gpu_ga3c_edges.py, and those tests are not vacuous."""
import numpy as np
import pytest

from tests import ga3c_edge_rows as er
from tests import ga3c_f64_ref as f64
from tests import ga3c_value_ref as vref

RTOL, ATOL = 1e-4, 2e-4
SLOTS = 512         # two workgroups on each of the MI355X's 256 CUs


@pytest.fixture(scope="module")
def weights():
    return f64.load_weights(er.DEFAULT_WEIGHTS)


@pytest.fixture(scope="module")
def classes(weights):
    rows = er.edge_rows(np.random.default_rng(1905), weights)
    ref = {k: f64.evaluate(weights, v) for k, v in rows.items() if k in er.FINITE}
    return rows, ref


@pytest.mark.parametrize("n_rows", [er.laid_out_rows(SLOTS, 2), er.laid_out_rows(SLOTS, 3), er.laid_out_rows(SLOTS, 4),
                                    16 * (2 * SLOTS) + 5, 16 * (3 * SLOTS) + 5, 1, 16, 17, 16000, 20000, 24576, 27000, 32768,
                                    32769])
def test_tile_plan_covers_every_row_once(n_rows):
    plan = er.tile_plan(n_rows, SLOTS)
    assert len(plan) <= (n_rows + 31) // 32                     # the grid the launchers start
    nxt = 0
    for row0, tm in plan:
        assert row0 == nxt and tm in (32, 48, 64) and row0 < n_rows
        nxt = row0 + tm
    assert n_rows <= nxt < n_rows + 64
    # one round of resident tiles until the rows no longer fit 64-row tiles; a round's tiles differ by one block at most
    assert len(plan) <= SLOTS * -(-n_rows // (64 * SLOTS))
    heights = sorted({tm for _, tm in plan})
    assert len(heights) <= 2 and heights[-1] - heights[0] <= 16
    assert er.tile_plan(0, SLOTS) == []


def test_tile_plan_of_the_issue_row_counts():
    """16 (2 slots) + 5 rows: tile 0 is 48 rows, the others 32; 16 (3 slots) + 5: tile 0 is 64 rows, the others 48"""
    for lo in (2, 3):
        plan = er.tile_plan(16 * (lo * SLOTS) + 5, SLOTS)
        assert len(plan) == SLOTS and plan[0] == (0, 16 * (lo + 1)) and {tm for _, tm in plan[1:]} == {16 * lo}


@pytest.mark.parametrize("nrb", [2, 3, 4])
def test_laid_out_batch_holds_every_variant_of_its_height(nrb):
    b = er.laid_out_batch(SLOTS, nrb, np.random.default_rng(nrb))
    x, tiles = b["x"], b["tiles"]
    assert x.shape == (er.laid_out_rows(SLOTS, nrb), 138) and x.dtype == np.float32
    assert [(t["row0"], t["tm"]) for t in tiles] == er.tile_plan(x.shape[0], SLOTS)
    seq = x[:, 0].astype(np.int64)
    assert np.array_equal(seq, x[:, 0]) and seq.min() == 0 and seq.max() == 19
    tall = [t for t in tiles if t["tm"] == 16 * nrb]
    assert {t["pattern"] for t in tall} == set(range(len(er.PATTERNS)))        # every pattern at the target height
    assert any(t["all_live"] and t["tmax"] == 19 for t in tall) and any(not t["all_live"] for t in tall)
    assert any(t["all_live"] and t["tmax"] == 0 for t in tall)                 # no LSTM step at all on a multi-row tile
    assert 0 < tiles[-1]["real"] < tiles[-1]["tm"] and tiles[-1]["real"] % 16 == 5     # the last tile is partial
    for t in tiles:
        s = seq[t["row0"]:t["row0"] + t["real"]]
        assert t["all_live"] == (s.min() >= s.max()) and t["tmax"] == s.max()
        p = t["pattern"]
        if p < 4:
            assert np.all(s == (19, 0, 1, 7)[p]) and t["all_live"]
        elif p == 4:
            assert s.min() == 0 and s.max() == 19 and not t["all_live"]
        elif p == 5:
            odd = np.flatnonzero(s != 19)
            assert odd.size == 1 and odd[0] >= 16 * ((t["real"] - 1) // 16) and not t["all_live"]
        else:
            assert np.all(s[:-1] == 19) and s[-1] == 5 and not t["all_live"]
    if nrb > 2:      # the tiles below the tall ones are one block lower, and carry every pattern as well
        rest = [t for t in tiles if t["tm"] != 16 * nrb]
        assert {t["tm"] for t in rest} == {16 * (nrb - 1)} and {t["pattern"] for t in rest} == set(range(len(er.PATTERNS)))
    # slots past num_other are zero, the live ones are not
    live = np.repeat(np.arange(19)[None, :] < seq[:, None], 7, axis=1)
    assert np.all(x[:, 5:][~live] == 0) and np.all(x[:, 5:][live] != 0)


def test_edge_classes_are_what_their_labels_say(weights, classes):
    rows, ref = classes
    assert set(rows) == set(er.FINITE) | set(er.RAISES_GUARD)
    for k, x in rows.items():
        assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 138 and 0 < x.shape[0] <= 64, k
    xn = {k: f64.normalise(weights, v) for k, v in rows.items()}
    for k in er.FINITE:
        assert np.all(np.isfinite(rows[k])) and np.abs(xn[k][:, 5:]).max() < er.FP16_MAX, k
    # saturated: the largest scale reaches ~5e4 normalised
    top = [np.abs(xn["saturated x%d" % s][:, 5:]).max() for s in er.SATURATED_SCALES]
    assert top == sorted(top) and 3.0e4 < top[-1] < 6.0e4
    # cell bound: 19 identical slots, |c| up to its bound of 19 (c' = 2.885 |c| -> 54.8 of the documented 55)
    cb = rows["cell bound"]
    assert cb.shape[0] == 16 and np.all(cb[:, 0] == 19)
    assert np.array_equal(cb[:, 5:].reshape(16, 19, 7), np.repeat(cb[:, 5:12][:, None, :], 19, axis=1))
    cmax = ref["cell bound"][2]
    print("cell bound: max|c| %.6f .. %.6f, c' up to %.3f" % (cmax.min(), cmax.max(), 2.885390081777927 * cmax.max()))
    assert np.all(cmax >= 18.9) and np.all(cmax <= 19.0)
    assert ref["plausible"][2].max() < 10.0        # (plausible rows stay far from it)
    # tiny: live other-agent columns without an input_mean lie in [1e-9, 1e-4] after the float32 normalisation, both
    # signs; those with one within 1e-4 of zero
    t, tn = rows["tiny"], xn["tiny"][:, 5:]
    live = np.repeat(np.arange(19)[None, :] < t[:, :1].astype(np.int64), 7, axis=1)
    zero_mean = np.tile(weights["input_mean"][5:12] == 0, 19)[None, :] & live
    assert zero_mean.sum() > 1000
    mag = np.abs(tn[zero_mean])
    assert mag.min() >= 0.99e-9 and mag.max() <= 1.01e-4 and (tn[zero_mean] > 0).any() and (tn[zero_mean] < 0).any()
    assert (mag < 6e-8).mean() > 0.2               # a good share below the low plane's smallest denormal step
    assert np.abs(tn[live]).max() <= 1.01e-4
    # dirty tail: the twins differ only behind num_other, and do differ there
    d, tw = rows["dirty tail"], rows["dirty tail twin"]
    num = tw[:, 0].astype(np.int64)
    assert np.array_equal(num, tw[:, 0]) and num.max() <= 18
    tail = np.repeat(np.arange(19)[None, :] >= num[:, None], 7, axis=1)
    assert np.array_equal(d[:, :5], tw[:, :5]) and np.array_equal(d[:, 5:][~tail], tw[:, 5:][~tail])
    assert np.all(tw[:, 5:][tail] == 0) and np.all(d[:, 5:][tail] != 0) and np.abs(d[:, 5:][tail]).max() <= 50.0
    # count edges
    c, cc = rows["count edges"], rows["count edges clipped"]
    assert sorted(set(c[:, 0].tolist())) == sorted(np.float32(v) for v in er.COUNT_EDGES)
    assert np.array_equal(c[:, 1:], cc[:, 1:]) and np.all(c[:, 5:] != 0)
    assert np.array_equal(cc[:, 0], np.clip(np.trunc(c[:, 0]), 0, 19))
    assert sorted(set(cc[:, 0].tolist())) == [0.0, 2.0, 18.0, 19.0]
    # the guard: exactly one normalised other-agent value where intended, everything else plausible
    # (a column with input_std 5 cannot hit 65 503.996 exactly: it holds the closest value below, 65 503.992)
    for k, wanted in (("near the guard", [65000.0, -65000.0, er.BELOW_FP16_MAX, -er.BELOW_FP16_MAX]),
                      ("at the guard", [er.FP16_MAX, -er.FP16_MAX, np.inf])):
        big = np.abs(xn[k][:, 5:]) > 100.0
        assert np.all(big.sum(axis=1) == 1) and np.all(rows[k][:, 0] == 19)
        got = xn[k][:, 5:][big].astype(np.float64).reshape(len(wanted), -1)      # (rows are ordered by target)
        for g, v in zip(got, wanted):
            if k == "at the guard" or abs(v) == 65000.0:
                assert np.all(g == v), (k, v)
            else:
                assert np.all(np.sign(g) == np.sign(v)) and np.all(np.abs(g) < er.FP16_MAX) and np.all(np.abs(g) > 65503.99), (k, v)
                assert (g == v).any()
        cols = np.nonzero(big)[1]
        assert {c // 7 for c in cols} == set(er.GUARD_SLOTS) and {c % 7 for c in cols} == set(er.GUARD_FEATURES)
    assert er.BELOW_FP16_MAX < er.FP16_MAX and np.float32(er.BELOW_FP16_MAX) == np.nextafter(np.float32(65504), np.float32(0))
    # NaN: one per row, in a live other-agent column / in a host column
    no, nh = rows["nan other"], rows["nan host"]
    assert np.all(np.isnan(no).sum(axis=1) == 1) and not np.isnan(no[:, :5]).any() and np.all(no[:, 0] == 19)
    assert np.all(np.isnan(nh).sum(axis=1) == 1) and not np.isnan(nh[:, 5:]).any() and not np.isnan(nh[:, 0]).any()
    assert set(np.nonzero(np.isnan(nh))[1].tolist()) == {1, 2, 3, 4}


def test_float64_reference_agrees_with_the_float32_network_on_every_finite_class(weights, classes):
    """numpy's float32 evaluation against the float64 one, per class: inside the bar the kernel is held to (measured: max
    abs error 1.5e-5 on plausible rows, rising to 5e-4 at x5000 where the logits reach 131), and the best action is clear
    (top-two gap above 1e-3) on at least 90 % of the rows of each class"""
    rows, ref = classes
    net = vref.GA3CNet(er.DEFAULT_WEIGHTS)
    for k in er.FINITE:
        with np.errstate(over="ignore"):       # (a saturated gate: exp -> inf, 1 / (1 + inf) = 0, as intended)
            l32, v32 = vref.logits_and_value(net, rows[k])
        l64, v64, _ = ref[k]
        err = np.abs(l32 - l64)
        srt = np.sort(l64, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-3
        print("%-20s logits up to %7.2f: |numpy f32 - f64| max %.3g mean %.3g; value max %.3g; clear %.1f %%" % (
            k, np.abs(l64).max(), err.max(), err.mean(), np.abs(v32 - v64).max(), 100 * clear.mean()))
        np.testing.assert_allclose(l32, l64, rtol=RTOL, atol=ATOL, err_msg=k)
        np.testing.assert_allclose(v32, v64, rtol=RTOL, atol=ATOL, err_msg=k)
        assert clear.mean() >= 0.9, k
        assert np.array_equal(np.argmax(l32, axis=1)[clear], np.argmax(l64, axis=1)[clear]), k


def test_float64_reference_is_the_graph(weights):
    """the moved reference still is what tests/test_gpu_parity.py used: the float32 network within round-off on plausible
    rows, the sequence length from the raw count (truncated, clamped by the loop), steps behind it without effect"""
    rng = np.random.default_rng(5)
    x = er.plausible_x(rng, rng.integers(0, 20, 200))
    l64, v64, cmax = f64.evaluate(weights, x)
    net = vref.GA3CNet(er.DEFAULT_WEIGHTS)
    l32, v32 = vref.logits_and_value(net, x)
    assert np.abs(l32 - l64).max() < 1e-4 and np.abs(v32 - v64).max() < 1e-4
    assert np.array_equal(f64.logits_f64(weights, x), l64)
    assert np.all(cmax[x[:, 0] == 0] == 0) and np.all(cmax[x[:, 0] > 0] > 0)
    y = x.copy()
    y[:, 0] = np.where(x[:, 0] == 19, 40.0, x[:, 0] + 0.75)
    assert np.array_equal(f64.evaluate(weights, y)[0], l64)
    y[:, 0] = -2.5
    z = x.copy()
    z[:, 0] = 0
    assert np.array_equal(f64.evaluate(weights, y)[0], f64.evaluate(weights, z)[0])
