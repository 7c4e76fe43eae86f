"""The leverage sweeps (lev.hip, lev_sort.hip) where their kernels change path:
1-5 investors (the four select targets share prefixes and histograms), counts
around the 128 workgroups' chunks of four, the 32-step outcome windows, tied,
negative, zero and signed-zero values, a top group that dominates every sum or
holds inf, strided outcome rows, every lev_prefix_kernel instantiation, and the
entry points' argument checks.

The device is compared with oracle/lev.py on every case and with the
reference's own run (tests/golden/lev_edges.npz) where the inputs stay finite,
under the bounds of tests/test_lev_gpu.py: categorical values bit-equal and
table 2e-6, GBM 2e-5, coin 1e-5, final statistics 1e-5, big brain 2e-6; an entry
is finite on the device exactly where it is in the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lev as olev
from tests.test_lev_cpu import (EDGES, ZE, close26, close_final, edge_inputs, edge_oracle, lev_paths,
                                means_do_not_cancel, same_finite_and_close, zero_boundary_steps)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DICE, DICESH = (0.5, -0.5, 0.05), (0.5, -0.5, 0.05, -1.0, 5.0, -1.0)
RETS = {"dice": DICE, "dicesh": DICESH, "gbm": ()}
GRID = {"dice": (0.5, 1.0, 0.5), "dicesh": (0.5, 1.0, 0.5), "gbm": (0.5, 2.5, 1.0)}
FLT_MAX = float(np.finfo(np.float32).max)


def outcomes(kind, inv, hor, seed):
    rng = np.random.default_rng(seed)
    if kind == "gbm":
        return (0.0540025395205692 - 0.1897916175617430 ** 2 / 2
                + 0.1897916175617430 * rng.standard_normal((inv, hor))).astype(np.float32)
    u = rng.random((inv, hor))
    return np.where(u < 1 / 6, 0, np.where(u < 2 / 6, 1, 2)).astype(np.float32)


def device_sweep(kind, o, top, v0, rets, grid, final_values=True):
    from rlmd_amd import lev

    o = torch.from_numpy(np.ascontiguousarray(o))
    inv, hor = o.shape
    if kind == "gbm":
        d, dT = lev.gbm_smart_lev(DEV, o, inv, hor, top, v0, *grid, final_values=final_values)
    elif kind == "dicesh":
        d, dT = lev.dice_sh_smart_lev(DEV, o, inv, hor, top, v0, *rets, *grid, final_values=final_values)
    else:
        d, dT = lev.dice_smart_lev(DEV, o, inv, hor, top, v0, *rets, *grid, final_values=final_values)
    return d.cpu().numpy(), None if dT is None else dT.cpu().numpy()


def check_sweep(kind, got, want):
    """Final values bit-equal (categorical) or 2e-5 (GBM: device vs host expf);
    the table finite where the reference's is, and there within 2e-6 / 2e-5."""
    (d, dT), (rd, rdT) = got, want
    assert d.shape == rd.shape and dT.shape == rdT.shape
    if kind == "gbm":
        assert (np.isfinite(dT) == np.isfinite(rdT)).all()
        np.testing.assert_allclose(dT, rdT, rtol=2e-5, atol=0)
        same_finite_and_close(d, rd, 2e-5)
    else:
        np.testing.assert_array_equal(dT, rdT)
        same_finite_and_close(d, rd, 2e-6)


def sweep_vs_oracle(kind, o, top, v0=100.0, rets=None, grid=None):
    rets = RETS[kind] if rets is None else rets
    grid = GRID[kind] if grid is None else grid
    got = device_sweep(kind, o, top, v0, rets, grid)
    want = edge_oracle(kind, o, top, v0, rets, grid)
    check_sweep(kind, got, want)
    return got, want


def fixture_case(name):
    """Every top of a lev_edges.npz case against the oracle and the reference's run."""
    kind, o, v0, rets, grid = edge_inputs(name)
    for top in ZE[name + "_tops"]:
        top = int(top)
        got, _ = sweep_vs_oracle(kind, o, top, v0, rets, grid)
        check_sweep(kind, got, (ZE[f"{name}_top{top}_data"], ZE[f"{name}_top{top}_data_T"]))


# ---- rlmd_lev_sweep_sorted ------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EDGES if n.startswith("tiny")])
def test_sorted_sweep_tiny(name):
    """1-5 investors at horizon 4, top 0, 1, N and N + 5 (clamped to N): 127 of
    the 128 workgroups are empty, the four select targets share prefixes and
    histograms, and an empty group's rows are NaN."""
    fixture_case(name)


@pytest.mark.parametrize("kind", ["dice", "dicesh", "gbm"])
@pytest.mark.parametrize("inv", [63, 65, 511, 513])
def test_sorted_sweep_chunk_edges(kind, inv):
    """Investor counts around the workgroups' chunks of four values: below 513
    most workgroups are empty, at 513 the first chunk is eight wide, and the last
    16-byte vector is ragged; top 1, N // 2 and N - 1 give odd and even lower medians."""
    o = outcomes(kind, inv, 33, inv)
    for top in (1, inv // 2, inv - 1):
        sweep_vs_oracle(kind, o, top)


@pytest.mark.parametrize("kind", ["dice", "gbm"])
@pytest.mark.parametrize("hor", [2, 32, 33, 64, 65])
def test_sorted_sweep_window_edges(kind, hor):
    """Horizons around the 32-step outcome windows (u8 and f32): one full window,
    a one-step last window, and the one-column table of horizon 2."""
    sweep_vs_oracle(kind, outcomes(kind, 65, hor, hor), 7)


@pytest.mark.parametrize("kind", ["dice", "gbm"])
def test_sorted_sweep_all_tied(kind):
    """Every outcome equal: one tie class holds both groups, so every copy is
    placed by count alone and a non-empty group's mad and std are exactly 0."""
    o = np.full((64, 5), 2.0 if kind == "dice" else 0.01, dtype=np.float32)
    for top in (0, 1, 32, 64):
        (d, _), _ = sweep_vs_oracle(kind, o, top)
        rows = [3, 6] + ([4, 7] if top > 0 else []) + ([5, 8] if top < 64 else [])
        assert (d[:, rows, :] == 0).all(), d[:, 3:9, :]


@pytest.mark.parametrize("name", ["signed_dice", "signed_dicesh"])
def test_sorted_sweep_signed(name):
    """Factors 3, -0.5, 1.1 (dice-SH 4, -5.5, 2.1) at leverage 2: negative values,
    the negative half of the order-preserving key.  No group mean cancels below
    1e-3 of the group's mean |v| (asserted on the oracle)."""
    kind, o, v0, rets, grid = edge_inputs(name)
    vals = lev_paths(kind, o, v0, rets, grid)
    assert (vals < 0).any()
    for top in ZE[name + "_tops"]:
        assert means_do_not_cancel(edge_oracle(kind, o, int(top), v0, rets, grid)[0], vals, int(top))
    fixture_case(name)


def test_sorted_sweep_signed_zeros():
    """Factors 3, -0.5 and 0: a zero value keeps the running product's sign, so
    -0 and +0 (equal values, adjacent keys) share the top group's boundary class."""
    kind, o, v0, rets, grid = edge_inputs("zeros_dice")
    vals = lev_paths(kind, o, v0, rets, grid)
    assert zero_boundary_steps(vals, 32) >= 2
    for top in ZE["zeros_dice_tops"]:
        assert means_do_not_cancel(edge_oracle(kind, o, int(top), v0, rets, grid)[0], vals, int(top))
    fixture_case("zeros_dice")


def test_sorted_sweep_dominated_top():
    """Three investors that only win (3^t against the others' ~1.14^t): by step
    60 their sum exceeds the adjusted group's by more than 1e16, past what a
    difference of two f64 sums resolves.  Every value is finite; all rows at 2e-6."""
    kind, o, v0, rets, grid = edge_inputs("dom_dice")
    assert np.isfinite(lev_paths(kind, o, v0, rets, grid)).all()
    fixture_case("dom_dice")


def overflow_inputs(kind):
    """dom_dice's matrix continued to horizon 90 (100 * 3^n passes the f32 range
    at n = 77 factors), and a GBM twin: three investors whose log-returns are 1,
    1.02 and 1.04 every step, leverages 1 and 2."""
    _, o62, v0, rets, grid = edge_inputs("dom_dice")
    if kind == "dice":
        o = np.concatenate([o62, outcomes("dice", 40, 28, 90)], axis=1)
    else:
        o, rets, grid = outcomes("gbm", 40, 90, 91), (), (1.0, 2.0, 1.0)
    for k, row in enumerate((3, 17, 38)):
        o[row] = 0.0 if kind == "dice" else 1.0 + 0.02 * k
    return o, v0, rets, grid


@pytest.mark.parametrize("kind", ["dice", "gbm"])
def test_sorted_sweep_overflow(kind):
    """The three winners' values become +inf and all lie in the top group (top 3,
    5): the adjusted rows 2, 5, 8, 11 stay finite at every step (asserted on the
    oracle), and no statistic of the adjusted group may pass through inf - inf.
    With top 2 one inf is adjusted: those rows are non-finite in both.  Oracle
    only: the reference's f32 reductions overflow before its values do.  GBM: no
    exact value lies within 0.1 % of the f32 limit, 50 times the 2e-5 that 90
    expf factors may differ by, so device and oracle overflow at the same step."""
    o, v0, rets, grid = overflow_inputs(kind)
    if kind == "gbm":
        for lev in olev.param_range(*grid):
            v = v0 * np.exp(np.cumsum(lev * o.astype(np.float64), axis=1))
            assert ((v < FLT_MAX / 1.001) | (v > FLT_MAX * 1.001)).all()
    for top in (2, 3, 5):
        with np.errstate(over="ignore", invalid="ignore"):  # the oracle's own inf and inf - inf
            (d, dT), (od, odT) = sweep_vs_oracle(kind, o, top, v0, rets, grid)
        assert np.isinf(odT).sum() == 3 * odT.shape[0]
        if top >= 3:
            assert np.isfinite(od[:, [2, 5, 8, 11], :]).all()
            assert not np.isfinite(od[:, 1, -1]).any()


def abi_sorted(kind, view, top, v0, rets, grid, entry="rlmd_lev_sweep_sorted", ws_short=0, n_lev=None):
    """rlmd_lev_sweep_sorted / rlmd_lev_final_sorted on a device matrix that may be
    a strided view (ld = its row stride).  Returns (rc, data, data_T)."""
    from rlmd_amd import _abi

    lib = _abi.lib()
    inv, hor = view.shape
    neg, _ = olev._gambles(kind, np.zeros((1, 1)), tuple(rets))
    levs = olev._levs(*grid, neg) if n_lev is None else np.linspace(0.1, 1.0, n_lev, dtype=np.float32)
    codes = np.array([[0.0, 1.0, 2.0]], dtype=np.float32)
    table = None if kind == "gbm" else np.ascontiguousarray(
        [olev._gambles(kind, codes, tuple(rets))[1](lv)[0] for lv in levs], dtype=np.float32)
    need = int(lib.rlmd_lev_sorted_workspace_bytes(inv, len(levs)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    final = entry == "rlmd_lev_final_sorted"
    data = torch.zeros((len(levs), 13) if final else (len(levs), 13, max(hor - 1, 1)), dtype=torch.float32, device=DEV)
    data_T = torch.zeros((len(levs), inv), dtype=torch.float32, device=DEV)
    rc = getattr(lib, entry)(1 if kind == "gbm" else 0, C.c_void_p(view.data_ptr()), inv, hor, view.stride(0), top,
                             float(v0), None if table is None else table.ctypes.data, levs.ctypes.data, len(levs),
                             _abi.ptr(ws), need - ws_short, _abi.ptr(data), _abi.ptr(data_T), _abi.stream_ptr())
    torch.cuda.synchronize()
    return rc, data.cpu().numpy(), data_T.cpu().numpy()


@pytest.mark.parametrize("kind", ["dice", "gbm"])
def test_sorted_sweep_strided_rows(kind):
    """65 x 33 outcomes as columns 5-37 of a 65 x 40 buffer (u8 codes, f32
    log-returns): ld 40 > horizon; the columns outside hold values that would
    show in the table if the window kernel read them."""
    o = outcomes(kind, 65, 33, 40)
    buf = np.full((65, 40), 7 if kind == "dice" else 3.0, dtype=np.uint8 if kind == "dice" else np.float32)
    buf[:, 5:38] = o
    view = torch.from_numpy(buf).to(DEV)[:, 5:38]
    assert view.stride(0) == 40 and not view.is_contiguous()
    rc, d, dT = abi_sorted(kind, view, 7, 100.0, RETS[kind], GRID[kind])
    assert rc == 0
    check_sweep(kind, (d, dT), edge_oracle(kind, o, 7, 100.0, RETS[kind], GRID[kind]))


def test_sorted_sweep_repeats_bit_equal():
    """The f64 sums run in a fixed order: two runs give the same bits."""
    o = outcomes("gbm", 513, 33, 5)
    a = device_sweep("gbm", o, 50, 100.0, (), GRID["gbm"])
    b = device_sweep("gbm", o, 50, 100.0, (), GRID["gbm"])
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    check_sweep("gbm", a, edge_oracle("gbm", o, 50, 100.0, (), GRID["gbm"]))


# ---- *_fixed_final_lev (rlmd_lev_final_sorted) -----------------------------------
def check_final(kind, got, want):
    (st, vals), (ost, ovals) = got, want
    st, vals = st.cpu().numpy(), vals.cpu().numpy()
    assert st.shape == ost.shape and vals.shape == ovals.shape
    assert (np.isfinite(vals) == np.isfinite(ovals)).all()
    np.testing.assert_allclose(vals, ovals, rtol=1e-5, atol=0)
    same_finite_and_close(st[:, :12], ost[:, :12], 1e-5, close=close_final)
    np.testing.assert_array_equal(st[:, 12], ost[:, 12])


@pytest.mark.parametrize("kind", ["coin", "dice", "dicesh", "gbm"])
@pytest.mark.parametrize("inv,hor", [(i, h) for i in (1, 5, 513) for h in (1, 33)])
def test_fixed_final_shapes(kind, inv, hor):
    """Horizon 1 (only this entry point accepts it) and 33, 1 / 5 / 513 investors,
    top 0, 1 and N.  Coin at leverages 2.5 and 3 with returns (0.5, -0.4): the
    down factor is 0 and -0.2."""
    from rlmd_amd import lev

    if kind == "coin":
        o = (np.random.default_rng(inv + hor).random((inv, hor)) < 0.5).astype(np.float32)
        rets, grid = (0.5, -0.4), (2.5, 3.0, 0.5)
        down = olev._gambles("coin", np.zeros((1, 1)), rets)[1]
        assert down(np.float32(2.5))[0, 0] == 0 and down(np.float32(3.0))[0, 0] < 0
    else:
        o, rets, grid = outcomes(kind, inv, hor, inv + hor), RETS[kind], GRID[kind]
    fn = {"coin": lev.coin_fixed_final_lev, "dice": lev.dice_fixed_final_lev, "dicesh": lev.dice_sh_fixed_final_lev,
          "gbm": lev.gbm_fixed_final_lev}[kind]
    for top in (0, 1, inv):
        got = fn(DEV, torch.from_numpy(o), top, 100.0, *rets, *grid)
        check_final(kind, got, olev.final_stats(kind, o, top, 100.0, rets, *grid))


@pytest.mark.parametrize("name", ["zeros_dice", "dom_dice"])
def test_fixed_final_signed_zeros_and_dominated(name):
    from rlmd_amd import lev

    kind, o, v0, rets, grid = edge_inputs(name)
    for top in ZE[name + "_tops"]:
        got = lev.dice_fixed_final_lev(DEV, torch.from_numpy(o), int(top), v0, *rets, *grid)
        check_final(kind, got, olev.final_stats(kind, o, int(top), v0, rets, *grid))


# ---- rlmd_lev_brain ----------------------------------------------------------------
STOPS, ROLLS = (0.1, 0.5), (0.0, 0.9)


def brain_case(f64, inv, hor, seed):
    """(codes [inv, hor] int64, rets3 as the facade passes them, lev_factor)."""
    u = np.random.default_rng(seed).random((inv, hor))
    if f64:
        return np.where(u < 1 / 6, 0, np.where(u < 2 / 6, 1, 2)).astype(np.int64), [0.5, -0.5, 0.05], 1.6
    return (u < 0.5).astype(np.int64), [-0.4, 0.5, 0.5], 1.8  # code 0 down, 1 up


def brain_device(f64, codes_dev, inv, hor, top, rets3, lf):
    """The facade's launch (it takes the stop and retention grids as tensors: the
    public functions build them with param_range, which drops 0 from a longer grid)."""
    from rlmd_amd import lev

    return lev._brain(DEV, codes_dev, inv, hor, top, 100.0, rets3, lf, torch.tensor(STOPS), torch.tensor(ROLLS),
                      f64).cpu().numpy()


def brain_abi(f64, view, hor, top, rets3, lf, ws_short=0):
    """rlmd_lev_brain on a device code matrix that may be a strided view, with the
    configurations [floor, roll, first leverage, roll > 0, stop] in f32 as the
    oracle forms them.  Returns (rc, data [rolls, stops, 26, horizon - 1])."""
    from rlmd_amd import _abi

    lib, f = _abi.lib(), np.float32
    inv = view.shape[0]
    cfg = np.array([[s * f(100), r, f(lf) * (f(1) - s * f(100) / f(100)), r != 0, s]
                    for r in np.array(ROLLS, f) for s in np.array(STOPS, f)], dtype=f)
    need = int(lib.rlmd_lev_brain_workspace_bytes(inv, len(cfg)))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    data = torch.zeros((len(ROLLS), len(STOPS), 26, max(hor - 1, 1)), dtype=torch.float32, device=DEV)
    r3 = np.array([float(r) if f64 else float(f(r)) for r in rets3], dtype=np.float64)
    rc = lib.rlmd_lev_brain(1 if f64 else 0, C.c_void_p(view.data_ptr()), inv, hor, view.stride(0), top, 100.0,
                            r3.ctypes.data, float(f(lf)), cfg.ctypes.data, len(cfg), _abi.ptr(ws), need - ws_short,
                            _abi.ptr(data), _abi.stream_ptr())
    torch.cuda.synchronize()
    return rc, data.cpu().numpy()


def brain_oracle(f64, codes, top, rets3, lf):
    r3 = list(rets3) if f64 else [np.float32(r) for r in rets3]
    return olev.brain_lev(codes, r3, top, 100.0, np.float32(lf), np.array(STOPS, np.float32),
                          np.array(ROLLS, np.float32), f64=f64)


@pytest.mark.parametrize("f64", [False, True], ids=["coin_f32", "dice_f64"])
@pytest.mark.parametrize("inv,hor", [(i, h) for i in (1, 3, 65) for h in (2, 33)])
def test_big_brain_shapes(f64, inv, hor):
    """2 stops x 2 retention ratios (0 and 0.9) at 1 / 3 / 65 investors, horizon 2
    and 33, top 0, 1 and N: the f32 select (3 passes) and the f64 one (6 passes,
    a 9-bit last digit) at the sizes where the targets share histograms."""
    codes, rets3, lf = brain_case(f64, inv, hor, 7 * inv + hor)
    dev = torch.from_numpy(codes.astype(np.uint8)).to(DEV)
    for top in (0, 1, inv):
        d = brain_device(f64, dev, inv, hor, top, rets3, lf)
        od = brain_oracle(f64, codes, top, rets3, lf)
        assert d.shape == od.shape
        same_finite_and_close(d, od, 2e-6, close=close26)


@pytest.mark.parametrize("f64", [False, True], ids=["coin_f32", "dice_f64"])
def test_big_brain_strided_rows(f64):
    """65 x 33 codes as columns 5-37 of a 65 x 40 buffer whose other columns hold 7."""
    codes, rets3, lf = brain_case(f64, 65, 33, 11)
    buf = np.full((65, 40), 7, dtype=np.uint8)
    buf[:, 5:38] = codes
    view = torch.from_numpy(buf).to(DEV)[:, 5:38]
    assert view.stride(0) == 40 and not view.is_contiguous()
    rc, d = brain_abi(f64, view, 33, 9, rets3, lf)
    assert rc == 0
    same_finite_and_close(d, brain_oracle(f64, codes, 9, rets3, lf), 2e-6, close=close26)


# ---- rlmd_lev_coin_sweep -------------------------------------------------------------
def check_coin(o, top, up, dn, grid, final_values=True):
    from rlmd_amd import lev

    inv, hor = o.shape
    d, dT = lev.coin_smart_lev(DEV, o, inv, hor, top, 100.0, up, dn, *grid, final_values=final_values)
    od, odT = olev.coin_smart_lev(o, top, 100.0, up, dn, *grid)
    d = d.cpu().numpy()
    assert d.shape == od.shape
    if final_values:
        np.testing.assert_array_equal(dT.cpu().numpy(), odT)
    else:
        assert dT is None
    same_finite_and_close(d, od, 1e-5)
    return d


def coin_outcomes(inv, hor, seed):
    return (np.random.default_rng(seed).random((inv, hor)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("n_lev", [1, 4, 5, 10, 11, 16, 17, 32])
def test_coin_sweep_leverage_counts(n_lev):
    """Every lev_prefix_kernel instantiation (4, 10, 16, 32 leverages, at and just
    past each limit) and <0> (final_values=False), whose table must be bit-equal."""
    grid = (0.0625, 0.0625 * n_lev, 0.0625)  # exact in binary: n_lev leverages up to 2
    assert len(olev.param_range(*grid)) == n_lev
    o = coin_outcomes(257, 33, n_lev)
    d = check_coin(o, 9, 0.5, -0.4, grid)
    d0 = check_coin(o, 9, 0.5, -0.4, grid, final_values=False)
    np.testing.assert_array_equal(d.view(np.uint32), d0.view(np.uint32))


@pytest.mark.parametrize("inv", [1, 5, 4096])
@pytest.mark.parametrize("hor", [2, 64, 65, 128, 129])
def test_coin_sweep_shapes(inv, hor):
    """Horizons around the 64-step chunks and 1 / 5 / 4096 investors (one hist
    workgroup holds 4096), top 0, 1 and N."""
    o = coin_outcomes(inv, hor, inv + hor)
    for top in (0, 1, inv):
        check_coin(o, top, 0.5, -0.4, (0.5, 1.0, 0.5))


def test_coin_sweep_zero_factor():
    """Returns (0.5, -0.5) at leverage 2: the down factor is 0, every investor
    that ever lost holds 0 (bin_value's special case), the rest 100 * 2^t."""
    o = coin_outcomes(257, 33, 3)
    o[:3] = 1  # three investors never lose
    for top in (1, 3, 50):
        check_coin(o, top, 0.5, -0.5, (2.0, 2.0, 1.0))


def test_coin_sweep_equal_factors():
    """Leverage 0 alone (param_range(0, 0, 0.1)): both factors are 1, every bin holds value_0."""
    assert olev.param_range(0, 0, 0.1) == [0.0]
    d = check_coin(coin_outcomes(257, 33, 4), 9, 0.5, -0.4, (0, 0, 0.1))
    assert (d[:, [0, 1, 2, 9, 10, 11], :] == 100.0).all() and (d[:, 3:9, :] == 0).all()


# ---- argument checks: an error code and a message, no launch ------------------------
def last_error():
    from rlmd_amd import _abi

    return _abi.lib().rlmd_last_error()


def test_sorted_workspace_one_byte_short():
    view = torch.from_numpy(outcomes("gbm", 65, 33, 1)).to(DEV)
    for entry in ("rlmd_lev_sweep_sorted", "rlmd_lev_final_sorted"):
        rc, _, _ = abi_sorted("gbm", view, 7, 100.0, (), GRID["gbm"], entry=entry, ws_short=1)
        assert rc != 0 and b"workspace" in last_error()


def test_sorted_horizon_one_only_on_the_final_entry():
    o = outcomes("dice", 65, 1, 2)
    view = torch.from_numpy(o.astype(np.uint8)).to(DEV)
    rc, _, _ = abi_sorted("dice", view, 7, 100.0, DICE, GRID["dice"])
    assert rc != 0 and b"bad sizes" in last_error()
    rc, st, vals = abi_sorted("dice", view, 7, 100.0, DICE, GRID["dice"], entry="rlmd_lev_final_sorted")
    assert rc == 0
    ost, ovals = olev.final_stats("dice", o, 7, 100.0, DICE, *GRID["dice"])
    np.testing.assert_array_equal(vals, ovals)
    same_finite_and_close(st[:, :12], ost[:, :12], 1e-5, close=close_final)


def test_sorted_leverage_count_is_bounded():
    view = torch.from_numpy(outcomes("gbm", 8, 4, 3)).to(DEV)
    rc, _, _ = abi_sorted("gbm", view, 1, 100.0, (), None, n_lev=1025)
    assert rc != 0 and b"n_lev" in last_error()
    rc, _, _ = abi_sorted("gbm", view, 1, 100.0, (), None, n_lev=1024)
    assert rc == 0


def test_brain_argument_checks():
    codes, rets3, lf = brain_case(False, 65, 33, 12)
    dev = torch.from_numpy(codes.astype(np.uint8)).to(DEV)
    assert brain_abi(False, dev, 33, 9, rets3, lf, ws_short=1)[0] != 0 and b"workspace" in last_error()
    assert brain_abi(False, dev, 1, 9, rets3, lf)[0] != 0 and b"bad sizes" in last_error()


def coin_abi(hor, ld, n_lev):
    from rlmd_amd import _abi

    lib = _abi.lib()
    inv = 64
    o = torch.ones((inv, ld), dtype=torch.uint8, device=DEV)
    need = int(lib.rlmd_lev_workspace_bytes(inv, hor))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    levs = np.linspace(0.05, 1.0, n_lev, dtype=np.float32)
    data = torch.zeros((n_lev, 13, hor - 1), dtype=torch.float32, device=DEV)
    rc = lib.rlmd_lev_coin_sweep(_abi.ptr(o), inv, hor, ld, 1, 100.0, 0.5, -0.4, levs.ctypes.data, n_lev, _abi.ptr(ws),
                                 need, _abi.ptr(data), None, _abi.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_coin_argument_checks():
    assert coin_abi(33, 64, 32) == 0
    assert coin_abi(33, 64, 33) != 0 and b"leverage count" in last_error()
    assert coin_abi(33, 48, 4) != 0 and b"padded" in last_error()  # ld >= horizon, a multiple of 16, not of 64
