"""rlmd_lev_outcomes (lev_gen.hip) / lev.sample_outcomes against the CPU oracle.

Every draw is Philox(seed, investor, stream, tag 10, j >> 1), so
oracle.philox.uniform_draws / normal_draws regenerate the matrix: the
categorical codes must be bit-equal (the kernel compares the 53-bit integer of
the uniform with integer thresholds, which is exact), the GBM log-returns within
one f32 ulp (the device's log / sincospi agree with NumPy's to ~1e-12, far
below an f32 ulp of these values, so only an element on a rounding boundary may
move, by one step).  The oracle's 257 x 129 draws are computed once and sliced:
a draw depends on its (investor, step) index alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import philox as ph

pytestmark = pytest.mark.gpu

TAG = 10  # RLMD_TAG_LEV_OUTCOME
SEED = 420
DIE = (1 / 6, 1 / 6, 2 / 3)
LOG_MEAN, VOL = 0.0540025395205692 - 0.1897916175617430 ** 2 / 2, 0.1897916175617430
INVESTORS = [1, 63, 65, 257]
HORIZONS = [1, 2, 15, 16, 17, 63, 64, 65, 129]


@functools.lru_cache(maxsize=None)
def uniforms(seed=SEED, stream=0, first=0, inv=257, hor=129):
    u = ph.uniform_draws(seed, first + np.arange(inv), stream, TAG, hor)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def normals(seed=SEED, stream=0, first=0, inv=257, hor=129):
    z = ph.normal_draws(seed, first + np.arange(inv), stream, TAG, hor)
    z.setflags(write=False)
    return z


def coin_codes(u, up_prob):
    return (u < up_prob).astype(np.uint8)  # 1 up, 0 down


def dice_codes(u, probs=DIE):
    c = np.cumsum(np.asarray(probs, dtype=np.float64))  # NumPy's legacy choice, as dice_index
    return ((c[0] / c[2] <= u).astype(np.uint8) + (c[1] / c[2] <= u).astype(np.uint8))


def gbm_values(z):
    return (LOG_MEAN + VOL * z).astype(np.float32)


def within_one_ulp(d, ref):
    """Element-wise: equal, or the f32 neighbour of the reference on either side."""
    return (d == ref) | (d == np.nextafter(ref, np.float32(np.inf))) | (d == np.nextafter(ref, np.float32(-np.inf)))


@pytest.mark.parametrize("hor", HORIZONS)
@pytest.mark.parametrize("inv", INVESTORS)
def test_codes_bit_equal_to_oracle(dev, inv, hor):
    """Odd horizons use half of the last Philox block; 15 / 16 / 17 straddle the run a
    thread owns, 63 / 64 / 65 the coin's 64-step padding."""
    from rlmd_amd import lev

    u = uniforms()[:inv, :hor]
    for up_prob in (0.5, 0.3):
        buf, h = lev.sample_outcomes("coin", inv, hor, seed=SEED, device=dev, up_prob=up_prob)
        assert h == hor and buf.dtype == torch.uint8 and buf.shape == (inv, (hor + 63) // 64 * 64)
        b = buf.cpu().numpy()
        np.testing.assert_array_equal(b[:, :hor], coin_codes(u, up_prob))
        assert not b[:, hor:].any(), "pad columns must be 0"
    d = lev.sample_outcomes("dice", inv, hor, seed=SEED, device=dev, probs=DIE)
    assert d.dtype == torch.uint8 and d.shape == (inv, hor) and d.is_contiguous()
    np.testing.assert_array_equal(d.cpu().numpy(), dice_codes(u))


@pytest.mark.parametrize("hor", [1, 2, 33, 129])
@pytest.mark.parametrize("inv", [1, 65, 257])
def test_gbm_within_one_ulp_of_oracle(dev, inv, hor):
    from rlmd_amd import lev

    o = lev.sample_outcomes("gbm", inv, hor, seed=SEED, device=dev, log_mean=LOG_MEAN, vol=VOL)
    assert o.dtype == torch.float32 and o.shape == (inv, hor) and o.is_contiguous()
    d, ref = o.cpu().numpy(), gbm_values(normals()[:inv, :hor])
    print(f"gbm {inv} x {hor}: {int((d != ref).sum())} of {d.size} elements differ from the oracle's f32 (by one ulp)")
    ok = within_one_ulp(d, ref)
    assert ok.all(), (np.argwhere(~ok)[:5], d[~ok][:5], ref[~ok][:5])


def _draw(dev, kind, inv, hor, **kw):
    from rlmd_amd import lev

    par = {"coin": {"up_prob": 0.3}, "dice": {"probs": DIE}, "gbm": {"log_mean": LOG_MEAN, "vol": VOL}}[kind]
    o = lev.sample_outcomes(kind, inv, hor, device=dev, **par, **kw)
    return (o[0] if kind == "coin" else o).cpu().numpy()


@pytest.mark.parametrize("kind", ["coin", "dice", "gbm"])
def test_pure_function_of_the_index(dev, kind):
    """The sharding contract: rows [100, 165) drawn with first_investor=100 are rows
    100..164 of the 257-row matrix; seed and stream select another matrix; a repeat is
    bit-equal."""
    whole = _draw(dev, kind, 257, 129, seed=SEED)
    shard = _draw(dev, kind, 65, 129, seed=SEED, first_investor=100)
    np.testing.assert_array_equal(shard.view(np.uint8), whole[100:165].view(np.uint8))
    np.testing.assert_array_equal(_draw(dev, kind, 257, 129, seed=SEED).view(np.uint8), whole.view(np.uint8))
    assert (_draw(dev, kind, 257, 129, seed=SEED, stream=1) != whole).any()
    assert (_draw(dev, kind, 257, 129, seed=SEED + 1) != whole).any()


def test_shard_and_stream_match_oracle(dev):
    """first_investor and stream reach the Philox counter words the oracle names."""
    got = _draw(dev, "dice", 65, 33, seed=7, stream=3, first_investor=100)
    np.testing.assert_array_equal(got, dice_codes(uniforms(7, 3, 100, 65, 33)))
    got = _draw(dev, "gbm", 65, 33, seed=7, stream=3, first_investor=100)
    assert within_one_ulp(got, gbm_values(normals(7, 3, 100, 65, 33))).all()


def _abi_call(kind, first, inv, hor, params, out_ptr, ld, seed=SEED, stream=0):
    from rlmd_amd import _abi

    par = np.ascontiguousarray(params, dtype=np.float64)
    rc = _abi.lib().rlmd_lev_outcomes(kind, seed, stream, first, inv, hor, par.ctypes.data, C.c_void_p(out_ptr), ld,
                                      _abi.stream_ptr())
    torch.cuda.synchronize()
    return rc


COIN3 = [0.3, 1.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("offset,ld,hor", [(32, 32, 18), (4, 20, 18), (3, 19, 18), (48, 64, 64), (5, 17, 17)])
def test_strided_u8_output_inside_a_larger_buffer(dev, offset, ld, hor):
    """ld > horizon at a byte offset of a 0xFF buffer: 16-byte, 4-byte and single-byte
    stores (the base and ld decide).  The call's investors x ld bytes hold the codes and
    a zero pad; every other byte keeps 0xFF."""
    inv = 67
    flat = torch.full((offset + inv * ld + 77,), 0xFF, dtype=torch.uint8, device=dev)
    assert _abi_call(0, 0, inv, hor, COIN3, flat.data_ptr() + offset, ld) == 0
    f = flat.cpu().numpy()
    assert (f[:offset] == 0xFF).all() and (f[offset + inv * ld:] == 0xFF).all()
    rows = f[offset:offset + inv * ld].reshape(inv, ld)
    np.testing.assert_array_equal(rows[:, :hor], coin_codes(uniforms()[:inv, :hor], 0.3))
    assert not rows[:, hor:].any()


@pytest.mark.parametrize("offset,ld,hor", [(4, 36, 33), (1, 35, 33), (8, 16, 16)])
def test_strided_f32_output_inside_a_larger_buffer(dev, offset, ld, hor):
    """The f32 kernel's 16-byte and single-element stores; pad columns 0, the rest of
    the buffer (NaN here) untouched."""
    inv = 67
    flat = torch.full((offset + inv * ld + 77,), float("nan"), dtype=torch.float32, device=dev)
    assert _abi_call(1, 0, inv, hor, [LOG_MEAN, VOL], flat.data_ptr() + 4 * offset, ld) == 0
    f = flat.cpu().numpy()
    assert np.isnan(f[:offset]).all() and np.isnan(f[offset + inv * ld:]).all()
    rows = f[offset:offset + inv * ld].reshape(inv, ld)
    assert within_one_ulp(rows[:, :hor], gbm_values(normals()[:inv, :hor])).all()
    assert (rows[:, hor:] == 0).all()


def test_long_rows_take_one_row_per_workgroup(dev):
    """ld >= 32768 (2048 runs): a workgroup holds one row and loops over its runs.  The
    oracle's blocks are evaluated in one vectorised Philox call per row (the same
    counters as uniform_draws, checked on the first columns)."""
    inv, hor = 3, 32768 + 37
    got = _draw(dev, "dice", inv, hor, seed=SEED)
    blocks = np.arange((hor + 1) // 2)
    u = np.empty((inv, 2 * blocks.size))
    for i in range(inv):
        v = ph.philox(SEED, i, 0, TAG, blocks)
        u[i, 0::2], u[i, 1::2] = ph.u01(v[0], v[1]), ph.u01(v[2], v[3])
    np.testing.assert_array_equal(u[:, :129], uniforms()[:inv])
    np.testing.assert_array_equal(got, dice_codes(u[:, :hor]))


@pytest.mark.parametrize("kind,first,inv,hor,ld,params,word", [
    (0, 0, 8, 16, 15, COIN3, b"ld"),                      # ld < horizon
    (0, 0, 8, 0, 16, COIN3, b"horizon"),                  # horizon 0
    (0, 0, 0, 16, 16, COIN3, b"investors"),               # no investors
    (2, 0, 8, 16, 16, COIN3, b"kind"),                    # a bad kind
    (0, 2 ** 32 - 7, 8, 16, 16, COIN3, b"2^32"),          # the investor counter word would wrap
    (0, -1, 8, 16, 16, COIN3, b"2^32"),
    (0, 0, 8, 16, 16, [0.6, 0.3, 0.0, 1.0, 2.0], b"thresholds"),
    (0, 0, 8, 16, 16, [0.3, 1.0, 256.0, 0.0, 0.0], b"codes"),
])
def test_bad_arguments_launch_nothing(dev, kind, first, inv, hor, ld, params, word):
    from rlmd_amd import _abi

    buf = torch.full((4096,), 0xFF, dtype=torch.uint8, device=dev)
    rc = _abi_call(kind, first, inv, hor, params, buf.data_ptr(), ld)
    assert rc != 0 and word in _abi.lib().rlmd_last_error(), _abi.lib().rlmd_last_error()
    assert (buf == 0xFF).all()


def test_null_pointers_are_rejected(dev):
    from rlmd_amd import _abi

    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    lib = _abi.lib()
    assert lib.rlmd_lev_outcomes(0, SEED, 0, 0, 2, 16, None, C.c_void_p(buf.data_ptr()), 16, _abi.stream_ptr()) != 0
    assert b"null" in lib.rlmd_last_error()
    assert _abi_call(0, 0, 2, 16, COIN3, None, 16) != 0 and b"null" in lib.rlmd_last_error()


def test_sample_outcomes_rejects_bad_kinds(dev):
    from rlmd_amd import _abi, lev

    with pytest.raises(ValueError):
        lev.sample_outcomes("cards", 4, 4, device=dev)
    with pytest.raises(_abi.RlmdError):
        lev.sample_outcomes("dice", 4, 4, device=dev, first_investor=2 ** 32 - 1)
