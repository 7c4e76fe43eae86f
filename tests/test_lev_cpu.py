"""The leverage-sweep oracle (oracle/lev.py) against the reference's own
coin_smart_lev run (tests/golden/lev.npz, make_golden.py:lev_fixtures)."""
import os

import numpy as np
import pytest

from oracle import lev as olev

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lev.npz"))
CASES = ["pos", "neg", "odd"]


def close_table(d, ref, rtol):
    """Entry-wise within rtol of the reference, with the dispersion rows (mad,
    std) also allowed rtol of their group's mean (they cancel)."""
    means = ref[:, [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0], :]
    tol = rtol * np.abs(ref) + rtol * np.abs(means) * (np.arange(13) >= 3)[None, :, None] * (np.arange(13) < 9)[None, :, None]
    return np.abs(d - ref) <= tol + 1e-30


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference(case):
    a = Z[case + "_args"]
    inv, hor, top = int(a[0]), int(a[1]), int(a[2])
    d, dT = olev.coin_smart_lev(Z[case + "_outcomes"], top, *a[3:])
    assert d.shape == (len(Z[case + "_levs"]), 13, hor - 1) and dT.shape == (len(Z[case + "_levs"]), inv)
    np.testing.assert_array_equal(dT, Z[case + "_data_T"])  # the same sequential f32 products
    assert close_table(d, Z[case + "_data"], 2e-6).all()


def test_param_range_matches_reference_grid():
    for case in CASES:
        a = Z[case + "_args"]
        np.testing.assert_allclose(olev.param_range(*a[6:9]), Z[case + "_levs"], rtol=0, atol=0)


def test_facade_param_range_is_the_oracle_grid():
    from rlmd_amd import lev

    for args in [(0.05, 1.0, 0.05), (0.1, 1.0, 0.1), (0.0, 0.0, 0.1), (0.25, 1.0, 0.25)]:
        assert lev.param_range(*args) == olev.param_range(*args)


SORTED = ["dice", "diceneg", "dicesh", "gbm"]


def sorted_oracle(case, outcomes=None):
    """oracle/lev.py's dice / dice_sh / gbm sweeps on a fixture case's inputs."""
    a, rets = Z[case + "_args"], Z[case + "_rets"]
    top, v0, lo, hi, inc = int(a[2]), a[3], a[4], a[5], a[6]
    o = Z[case + "_outcomes"] if outcomes is None else outcomes
    if case == "gbm":
        return olev.gbm_smart_lev(o, top, v0, lo, hi, inc)
    if case == "dicesh":
        return olev.dice_sh_smart_lev(o, top, v0, *rets, lo, hi, inc)
    return olev.dice_smart_lev(o, top, v0, *rets, lo, hi, inc)


@pytest.mark.parametrize("case", SORTED)
def test_sorted_oracle_matches_reference(case):
    """dice_smart_lev / dice_sh_smart_lev / gbm_smart_lev (lev_exp.py:586, :1209,
    :1008) run by the reference on torch CPU: final values bit-equal for the
    categorical gambles (the same f32 factors and products) and within 2 f32 ulps
    for GBM (NumPy's vs torch's expf); the table within 2e-6 / 2e-5."""
    d, dT = sorted_oracle(case)
    ref_d, ref_dT = Z[case + "_data"], Z[case + "_data_T"]
    assert d.shape == ref_d.shape and dT.shape == ref_dT.shape
    if case == "gbm":
        np.testing.assert_allclose(dT, ref_dT, rtol=2e-5, atol=0)
        assert close_table(d, ref_d, 2e-5).all()
    else:
        np.testing.assert_array_equal(dT, ref_dT)
        assert close_table(d, ref_d, 2e-6).all()


ZF = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lev_final.npz"))


def test_galaxy_brain_matches_reference():
    """coin_galaxy_brain_lev (lev_exp.py:455-505) run by the reference: the
    Kelly-fraction grid, bit-equal (host arithmetic in Python floats, f32 table)."""
    from rlmd_amd import lev

    got = lev.coin_galaxy_brain_lev("cpu", *ZF["galaxy_args"]).numpy()
    np.testing.assert_array_equal(got, ZF["galaxy"])


def close_final(st, ref, rtol):
    """close_table for one [n_lev, 12] block of final statistics."""
    means = ref[:, [0, 1, 2] * 4]
    disp = (np.arange(12) >= 3) & (np.arange(12) < 9)
    return np.abs(st - ref) <= rtol * np.abs(ref) + rtol * np.abs(means) * disp[None, :] + 1e-30


@pytest.mark.parametrize("case", ["coin", "dice", "dicesh", "gbm"])
def test_final_stats_oracle_matches_reference(case):
    """oracle final_stats against the statistics the reference's *_fixed_final_lev
    computed (lev_final.npz): 1e-5 on values and statistics, as the device's test
    (the reference multiplies with gambles.prod(dim=1), the oracle step by step)."""
    a, rets = ZF[case + "_args"], [float(x) for x in ZF[case + "_rets"]]
    st, vals = olev.final_stats(case, ZF[case + "_outcomes"], int(a[2]), a[3], rets, a[4], a[5], a[6])
    np.testing.assert_allclose(vals, ZF[case + "_values"], rtol=1e-5, atol=0)
    ok = close_final(st[:, :12], ZF[case + "_stats"], 1e-5)
    assert ok.all(), np.argwhere(~ok)[:5]
    np.testing.assert_array_equal(st[:, 12], np.array(olev.param_range(a[4], a[5], a[6]), np.float32))


# ---- the sorted sweeps' edge inputs (lev_edges.npz, make_golden.py:lev_edge_fixtures)
ZE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lev_edges.npz"))
EDGES = sorted(k[:-len("_outcomes")] for k in ZE.files if k.endswith("_outcomes"))
EDGE_TOPS = [(name, int(top)) for name in EDGES for top in ZE[name + "_tops"]]


def edge_inputs(name):
    """(kind, outcomes, value_0, rets, (lev_low, lev_high, lev_incr)) of a lev_edges.npz case."""
    a = ZE[name + "_args"]
    return name.split("_")[1], ZE[name + "_outcomes"], a[2], tuple(float(r) for r in ZE[name + "_rets"]), tuple(a[3:6])


def edge_oracle(kind, o, top, v0, rets, grid):
    if kind == "gbm":
        return olev.gbm_smart_lev(o, top, v0, *grid)
    if kind == "dicesh":
        return olev.dice_sh_smart_lev(o, top, v0, *rets, *grid)
    return olev.dice_smart_lev(o, top, v0, *rets, *grid)


def same_finite_and_close(d, ref, rtol, close=close_table):
    """Finite exactly where the reference is, and there within close(..., rtol)."""
    fin = np.isfinite(ref)
    bad = np.isfinite(d) != fin
    assert not bad.any(), (np.argwhere(bad)[:6], d[bad][:6], ref[bad][:6])
    ok = close(np.where(fin, d, 0), np.where(fin, ref, 0), rtol)
    assert ok.all(), (np.argwhere(~ok)[:6], d[~ok][:6], ref[~ok][:6])


def lev_paths(kind, o, v0, rets, grid):
    """The f32 values [n_lev, horizon - 1, investors] behind a sweep's table columns."""
    neg, g_of_lev = olev._gambles(kind, o, rets)
    out = []
    for lev in olev._levs(*grid, neg):
        g = g_of_lev(lev)
        v, rows = (np.float32(v0) * g[:, 0]).astype(np.float32), []
        for t in range(1, o.shape[1]):
            v = (v * g[:, t]).astype(np.float32)
            rows.append(v)
        out.append(rows)
    return np.array(out)


def means_do_not_cancel(table, vals, top, floor=1e-3):
    """Every finite group mean of `table` (rows 0-2) is at least `floor` of that
    group's mean |v|: the 2e-6 bound is then a bound on the sums, not on how far
    a signed group's mean cancels."""
    for l in range(vals.shape[0]):
        for t in range(vals.shape[1]):
            s = np.abs(np.sort(vals[l, t])[::-1].astype(np.float64))
            for row, grp in enumerate((s, s[:top], s[top:])):
                m = table[l, row, t]
                if grp.size and np.isfinite(m) and abs(m) < floor * grp.mean():
                    return False
    return True


def zero_boundary_steps(vals, top):
    """Steps of leverage 0 at which the top group's boundary value is zero and
    the zero class holds both +0 and -0."""
    n = 0
    for v in vals[0]:
        z = v == 0
        n += bool(np.sort(v)[::-1][top - 1] == 0 and (z & np.signbit(v)).any() and (z & ~np.signbit(v)).any())
    return n


@pytest.mark.parametrize("name,top", EDGE_TOPS)
def test_sorted_oracle_matches_reference_at_edges(name, top):
    """The reference's dice / dice_sh / gbm sweeps at 1-5 investors (top 0, 1, N,
    N + 5: empty groups are NaN rows in both), with negative factors, with a zero
    factor (zeros of both signs) and with three investors that dominate every
    sum: values bit-equal (categorical) or 2e-5 (GBM), table 2e-6 / 2e-5."""
    kind, o, v0, rets, grid = edge_inputs(name)
    d, dT = edge_oracle(kind, o, top, v0, rets, grid)
    ref_d, ref_dT = ZE[f"{name}_top{top}_data"], ZE[f"{name}_top{top}_data_T"]
    assert d.shape == ref_d.shape and dT.shape == ref_dT.shape
    if kind == "gbm":
        np.testing.assert_allclose(dT, ref_dT, rtol=2e-5, atol=0)
        same_finite_and_close(d, ref_d, 2e-5)
    else:
        np.testing.assert_array_equal(dT, ref_dT)
        same_finite_and_close(d, ref_d, 2e-6)


@pytest.mark.parametrize("name", ["signed_dice", "signed_dicesh", "zeros_dice"])
def test_signed_edge_inputs_hold_their_premises(name):
    """The signed fixtures do hold negative values, no group mean of the oracle or
    of the reference cancels below 1e-3 of the group's mean |v|, and the
    signed-zeros matrix puts zeros of both signs in the boundary class."""
    kind, o, v0, rets, grid = edge_inputs(name)
    vals = lev_paths(kind, o, v0, rets, grid)
    assert (vals < 0).any() and (vals > 0).any()
    for top in ZE[name + "_tops"]:
        top = int(top)
        assert means_do_not_cancel(edge_oracle(kind, o, top, v0, rets, grid)[0], vals, top)
        assert means_do_not_cancel(ZE[f"{name}_top{top}_data"], vals, top)
    if name == "zeros_dice":
        assert (vals == 0).any()
        assert zero_boundary_steps(vals, 32) >= 2


def test_dominated_edge_input_is_dominated():
    """dom_dice: every value finite, and at the last step the three winners' sum
    exceeds the other 37 investors' by more than 1e16 (the f64 sum of all values
    does not resolve the adjusted group's)."""
    kind, o, v0, rets, grid = edge_inputs("dom_dice")
    vals = lev_paths(kind, o, v0, rets, grid)
    assert np.isfinite(vals).all()
    s = np.sort(vals[0, -1].astype(np.float64))
    assert s[-3:].sum() > 1e16 * s[:-3].sum()


BRAIN = ["coinbrain", "dicebrain", "dicebrain0"]


def close26(d, ref, rtol):
    """close_table for the big-brain tables (value rows 0-11, leverage rows 12-23)."""
    idx = [0, 1, 2] * 4
    means = np.concatenate([ref[:, :, idx, :], ref[:, :, [12 + i for i in idx], :], ref[:, :, 24:26, :]], 2)
    disp = np.zeros(26, bool)
    disp[3:9] = disp[15:21] = True
    tol = rtol * np.abs(ref) + rtol * np.abs(means) * disp[None, None, :, None]
    return np.abs(d - ref) <= tol + 1e-30


def brain_inputs(case):
    a, rets = ZF[case + "_args"], ZF[case + "_rets"]
    inv, hor, top, v0, lf = int(a[0]), int(a[1]), int(a[2]), a[3], a[4]
    o = ZF[case + "_outcomes"]
    return inv, hor, top, v0, lf, tuple(a[5:8]), tuple(a[8:11]), rets, o


@pytest.mark.parametrize("case", BRAIN)
def test_brain_oracle_matches_reference(case):
    """coin_big_brain_lev (roll 0: a ratio > 0 raises TypeError in the reference)
    and dice_big_brain_lev (f64 values; roll 0 and > 0) run by the reference:
    the oracle within 2e-6 (dispersion rows 2e-6 of their group mean)."""
    inv, hor, top, v0, lf, st, rl, rets, o = brain_inputs(case)
    stops = np.array(olev.param_range(*st), np.float32)
    rolls = np.array(olev.param_range(*rl), np.float32)
    if case == "coinbrain":
        d = olev.brain_lev((o == 1).astype(np.int64), [np.float32(rets[1]), np.float32(rets[0]), np.float32(rets[0])],
                           top, v0, np.float32(lf), stops, rolls)
    else:
        d = olev.brain_lev(o.astype(np.int64), list(rets), top, v0, np.float32(lf), stops, rolls, f64=True)
    assert d.shape == ZF[case + "_data"].shape
    assert close26(d, ZF[case + "_data"], 2e-6).all()
