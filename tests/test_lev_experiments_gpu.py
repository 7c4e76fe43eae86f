"""The leverage experiment drivers (rlmd_amd/lev_experiments.py) end to end at a
small size: 513 investors x 33 steps (GBM 257 x 33), top 3, coarse grids where
the default is large.  Each driver's files must exist with the reference's
shapes and equal oracle/lev.py's functions fed the oracle-regenerated outcomes
of the same seed, under the bounds tests/test_lev_gpu.py and
tests/test_lev_edges_gpu.py use for those functions: coin table 1e-5 and final
values bit-equal; categorical sorted sweeps 2e-6 and bit-equal; GBM 2e-5; final
statistics 1e-5; big brain 2e-6.
"""
import os

import numpy as np
import pytest
import torch

from oracle import lev as olev
from oracle import philox as ph
from tests.test_lev_cpu import close26, close_final, close_table, same_finite_and_close

pytestmark = pytest.mark.gpu

SEED, TAG = 420, 10
INV, HOR, TOP = 513, 33, 3
OUT = "./results/multiverse/"
L0, L1 = (0.05, 1.00, 0.05), (0.10, 1.00, 0.10)
S2, R2 = (0.10, 0.10, 0.10), (0.00, 0.00, 0.10)
S3 = (0.10, 0.50, 0.40)  # two stop levels


def uniforms(inv=INV, hor=HOR):
    return ph.uniform_draws(SEED, np.arange(inv), 0, TAG, hor)


def dice_codes(u):
    c = np.cumsum(np.array([1 / 6, 1 / 6, 1 - (1 / 6 + 1 / 6)]))
    return ((c[0] / c[2] <= u).astype(np.int64) + (c[1] / c[2] <= u).astype(np.int64))


def load(name):
    path = os.path.join(OUT, name + ".npy")
    assert os.path.exists(path), path
    return np.load(path)


def f32s(grid):
    return np.array(olev.param_range(*grid), np.float32)


def check_final(stats, want):
    ost, _ = want
    assert stats.shape == ost.shape
    same_finite_and_close(stats[:, :12], ost[:, :12], 1e-5, close=close_final)
    np.testing.assert_array_equal(stats[:, 12], ost[:, 12])


def test_coin_flip_experiment(dev, tmp_path, monkeypatch):
    from rlmd_amd import lev_experiments as le

    monkeypatch.chdir(tmp_path)
    r3 = (0.70, 0.95, 0.25)  # two retention ratios
    lines = []
    out = le.coin_flip(INVESTORS=INV, HORIZON=HOR, TOP=TOP, s3_l=S3[0], s3_h=S3[1], s3_i=S3[2], r3_l=r3[0],
                       r3_h=r3[1], r3_i=r3[2], ru_i=0.2, rd_i=0.2, path_results=OUT, seed=SEED, device=dev,
                       log=lines.append)
    o = (uniforms() < 0.5).astype(np.uint8)
    d, d_T = olev.coin_smart_lev(o, TOP, 100.0, 0.5, -0.4, *L1)
    got, got_T = load("coin_inv1_val"), load("coin_inv1_val_T")
    assert got.shape == (10, 13, HOR - 1) and got_T.shape == (10, INV) and got.dtype == got_T.dtype == np.float32
    np.testing.assert_array_equal(got_T, d_T)
    assert close_table(got, d, 1e-5).all()
    lf = np.float32(2.5)  # 1 / 0.4 - 1e-12 in f32
    rets = [np.float32(-0.4), np.float32(0.5), np.float32(0.5)]
    for name, stops, rolls in (("coin_inv2_val", S2, R2), ("coin_inv3_val", S3, r3)):
        want = olev.brain_lev(o.astype(np.int64), rets, TOP, 100.0, lf, f32s(stops), f32s(rolls))
        got = load(name)
        assert got.shape == want.shape == (len(f32s(rolls)), len(f32s(stops)), 26, HOR - 1)
        assert close26(got, want, 2e-6).all(), name
    rs, pus = olev.param_range(0.2, 0.8, 0.2), olev.param_range(0.25, 0.75, 0.25)
    g = load("coin_inv4_lev")
    assert g.shape == (3, len(rs), len(rs), 4) and g.dtype == np.float32
    kelly = np.array([[[[pu, ru, rd, pu / rd - (1 - pu) / ru] for rd in rs] for ru in rs] for pu in pus])
    np.testing.assert_array_equal(g, kelly.astype(np.float32))  # Python floats on the host, stored f32
    check_final(out["coin_final_stats"], olev.final_stats("coin", o, TOP, 100.0, (0.5, -0.4), *L0))
    for k in ("coin_inv1_val", "coin_inv1_val_T", "coin_inv2_val", "coin_inv3_val", "coin_inv4_lev"):
        np.testing.assert_array_equal(out[k], load(k))
    assert lines[0] == "Coin Flip Experiment Tests: Passed" and lines[-1].startswith("TOTAL TIME: ")
    assert sum("avg mean/med/mad/std" in ln for ln in lines) == 20  # one summary per investor-0 leverage


def test_dice_roll_experiment(dev, tmp_path, monkeypatch):
    from rlmd_amd import lev_experiments as le

    monkeypatch.chdir(tmp_path)
    r3 = (0.45, 0.95, 0.50)
    lines = []
    out = le.dice_roll(INVESTORS=INV, HORIZON=HOR, TOP=TOP, s3_l=S3[0], s3_h=S3[1], s3_i=S3[2], r3_l=r3[0],
                       r3_h=r3[1], r3_i=r3[2], path_results=OUT, seed=SEED, device=dev, log=lines.append)
    o = dice_codes(uniforms())
    rets = (0.5, -0.5, 0.05)
    d, d_T = olev.dice_smart_lev(o, TOP, 100.0, *rets, *L1)
    got, got_T = load("dice_inv1_val"), load("dice_inv1_val_T")
    assert got.shape == (10, 13, HOR - 1) and got_T.shape == (10, INV)
    np.testing.assert_array_equal(got_T, d_T)
    same_finite_and_close(got, d, 2e-6)
    lf = np.float32(2.0)  # 1 / 0.5 + 1e-12 in f32
    for name, stops, rolls in (("dice_inv2_val", S2, R2), ("dice_inv3_val", S3, r3)):
        want = olev.brain_lev(o, list(rets), TOP, 100.0, lf, f32s(stops), f32s(rolls), f64=True)
        got = load(name)
        assert got.shape == want.shape == (len(f32s(rolls)), len(f32s(stops)), 26, HOR - 1)
        assert close26(got, want, 2e-6).all(), name
    check_final(out["dice_final_stats"], olev.final_stats("dice", o, TOP, 100.0, rets, *L0))
    assert lines[0] == "Dice Roll Experiment Tests: Passed" and lines[-1].startswith("TOTAL TIME: ")


def test_dice_roll_sh_experiment(dev, tmp_path, monkeypatch):
    from rlmd_amd import lev_experiments as le

    monkeypatch.chdir(tmp_path)
    out = le.dice_roll_sh(INVESTORS=INV, HORIZON=HOR, TOP=TOP, path_results=OUT, seed=SEED, device=dev,
                          log=lambda s: None)
    o = dice_codes(uniforms())
    rets, grid = (0.5, -0.5, 0.05, -1, 5, -1), (0.73, 1.00, 0.03)
    d, d_T = olev.dice_sh_smart_lev(o, TOP, 100.0, *rets, *grid)
    got, got_T = load("dice_sh_inv1_val"), load("dice_sh_inv1_val_T")
    assert got.shape == d.shape == (len(olev.param_range(*grid)), 13, HOR - 1) and got_T.shape == d_T.shape
    np.testing.assert_array_equal(got_T, d_T)
    same_finite_and_close(got, d, 2e-6)
    check_final(out["dice_sh_final_stats"], olev.final_stats("dicesh", o, TOP, 100.0, rets, *grid))
    assert sorted(os.listdir(OUT)) == ["dice_sh_inv1_val.npy", "dice_sh_inv1_val_T.npy"]


def test_gbm_experiment(dev, tmp_path, monkeypatch):
    from rlmd_amd import lev_experiments as le

    monkeypatch.chdir(tmp_path)
    inv = 257
    out = le.gbm(INVESTORS=inv, HORIZON=HOR, TOP=TOP, path_results=OUT, seed=SEED, device=dev, log=lambda s: None)
    z = ph.normal_draws(SEED, np.arange(inv), 0, TAG, HOR)  # the same stream for each environment
    envs = (("gbm_op", 0.05, float(np.sqrt(0.2)), (-1.0, 1.0, 0.2), (-1.0, 1.0, 0.2)),
            ("gbm_snp", 0.0540025395205692, 0.1897916175617430, (0.4, 4.0, 0.4), (0.2, 2.0, 0.2)))
    for name, drift, vol, l0, l1 in envs:
        o = ((drift - vol ** 2 / 2) + vol * z).astype(np.float32)
        d, d_T = olev.gbm_smart_lev(o, TOP, 100.0, *l1)
        got, got_T = load(name + "_inv1_val"), load(name + "_inv1_val_T")
        assert got.shape == d.shape == (len(olev.param_range(*l1)), 13, HOR - 1) and got_T.shape == d_T.shape
        np.testing.assert_allclose(got_T, d_T, rtol=2e-5, atol=0)
        same_finite_and_close(got, d, 2e-5)
        check_final(out[name + "_final_stats"], olev.final_stats("gbm", o, TOP, 100.0, (), *l0))
    assert len(os.listdir(OUT)) == 4


def test_pair_form_is_bit_equal_to_the_matrix_form(dev):
    """coin_fixed_final_lev and coin_big_brain_lev read a (buf, horizon) pair in place
    (row stride = the 64-step padding); the plain 0/1 matrix goes through the copy."""
    from rlmd_amd import lev

    inv, hor = 513, 33
    buf, h = lev.sample_outcomes("coin", inv, hor, seed=SEED, device=dev)
    assert buf.stride(0) == 64
    plain = buf[:, :hor].cpu().numpy().astype(np.float32)
    a = lev.coin_fixed_final_lev(dev, (buf, h), TOP, 100.0, 0.5, -0.4, *L0)
    b = lev.coin_fixed_final_lev(dev, plain, TOP, 100.0, 0.5, -0.4, *L0)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    args = (inv, hor, TOP, 100.0, 0.5, -0.4, 2.5, 0.1, 0.5, 0.4, 0.0, 0.9, 0.3)
    x = lev.coin_big_brain_lev(dev, (buf, h), *args)
    y = lev.coin_big_brain_lev(dev, torch.from_numpy(plain), *args)
    np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError):
        lev.coin_big_brain_lev(dev, (buf, h), inv + 1, hor, *args[2:])
    with pytest.raises(ValueError):
        lev.coin_fixed_final_lev(dev, (buf.to(torch.float32), h), TOP, 100.0, 0.5, -0.4, *L0)
