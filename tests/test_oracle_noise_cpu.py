"""The oracle's restatements of the production noise and replay sample against
the reference's contract — CPU only.

oracle.philox.policy_noise restates the device's policy_draw and
oracle.replay.sample_indices its index draw; the GPU tests pin the device to
them (tests/test_policy_noise_gpu.py, tests/test_learn_ring_gpu.py).  Nothing
else pins the restatements themselves, and what the reference promises is not
an algorithm but a distribution: i.i.d. standard normal (or Laplace-uniform)
noise, and B distinct uniform indices.  These tests check that contract, and
that differently keyed draws are far apart (so that a mis-keyed device draw
cannot hide inside a tolerance).
"""
import numpy as np
import pytest
from scipy import stats

from oracle import philox as px
from oracle import replay as orp

N_ROWS, A, SEED, CTR, TAG = 200_000, 4, 7, 3, px.TAG_EPS_NEXT


def test_policy_noise_normal_is_iid_standard_normal():
    z = px.policy_noise("N", SEED, np.arange(N_ROWS), CTR, TAG, A).astype(np.float64)
    assert z.shape == (N_ROWS, A)
    for j in range(A):
        c = z[:, j]
        m, v, m4 = c.mean(), c.var(), np.mean(c ** 4)
        p = stats.kstest(c, "norm").pvalue
        print(f"component {j}: mean {m:+.5f}, var {v:.5f}, E z^4 {m4:.4f}, KS p {p:.3f}")
        assert abs(m) <= 0.01 and abs(v - 1.0) <= 0.01 and abs(m4 - 3.0) <= 0.08
        assert p >= 0.01
    corr = np.corrcoef(z.T)
    off = np.abs(corr[~np.eye(A, dtype=bool)])
    print(f"largest |correlation| between components: {off.max():.5f}")
    assert off.max() <= 0.01
    # MVN draws the same standard normals (the scale head is applied afterwards)
    np.testing.assert_array_equal(px.policy_noise("MVN", SEED, np.arange(1000), CTR, TAG, A), z[:1000].astype(np.float32))


def test_policy_noise_laplace_uniform():
    w = px.policy_noise("L", SEED, np.arange(N_ROWS), CTR, TAG, A)
    assert w.dtype == np.float32
    lo = np.float32(np.finfo(np.float32).eps) - np.float32(1.0)
    assert np.all(w >= lo) and np.all(w < np.float32(1.0))
    w = w.astype(np.float64)
    for j in range(A):
        # U(-1, 1): sd of the mean is 1 / sqrt(3 n) = 1.3e-3; four of them
        p = stats.kstest(w[:, j], "uniform", args=(-1.0, 2.0)).pvalue
        print(f"component {j}: mean {w[:, j].mean():+.5f}, KS p {p:.3f}")
        assert abs(w[:, j].mean()) <= 4.0 / np.sqrt(3.0 * N_ROWS)
        assert p >= 0.01
    off = np.abs(np.corrcoef(w.T)[~np.eye(A, dtype=bool)])
    assert off.max() <= 0.01


@pytest.mark.parametrize("dist,least", [("N", 0.90), ("L", 0.89)])
def test_mis_keyed_noise_is_far_from_the_right_one(dist, least):
    """Two independent standard normals differ by more than 0.1 with probability
    1 - erf(0.05) = 0.9436, two independent U(-1, 1) with 0.95^2 = 0.9025."""
    rows = np.arange(N_ROWS)
    right = px.policy_noise(dist, SEED, rows, CTR, TAG, A)
    wrong = {"counter + 1": px.policy_noise(dist, SEED, rows, CTR + 1, TAG, A),
             "other tag": px.policy_noise(dist, SEED, rows, CTR, px.TAG_EPS_CUR, A),
             "rows + 1": px.policy_noise(dist, SEED, rows + 1, CTR, TAG, A),
             "components reversed": right[:, ::-1]}
    for name, w in wrong.items():
        far = np.mean(np.abs(w.astype(np.float64) - right) > 0.1)
        print(f"{dist} {name}: {far:.4f} of elements differ by more than 0.1")
        assert far >= least, name


def test_policy_noise_keying():
    rows = np.array([0, 1, 5, 2 ** 32 - 1])
    a = px.policy_noise("N", SEED, rows, CTR, TAG, 3)
    # the counter's low word only (the device passes a uint32), A = 3 is a prefix of A = 4
    np.testing.assert_array_equal(a, px.policy_noise("N", SEED, rows, CTR + 2 ** 32, TAG, 3))
    np.testing.assert_array_equal(a, px.policy_noise("N", SEED, rows, CTR, TAG, 4)[:, :3])
    # the three production keys of one agent seed are distinct, 64-bit, and the learner's is the seed
    keys = {px.act_key(12345), px.learn_key(12345), px.replay_key(12345)}
    assert len(keys) == 3 and px.learn_key(12345) == 12345 and all(0 <= k < 2 ** 64 for k in keys)
    assert px.learn_noise_ctr(0) == 1


@pytest.mark.parametrize("M,B,T", [(300, 37, 2000), (8192, 1024, 300), (8193, 1024, 300), (20000, 200, 1500)])
def test_sample_indices_are_distinct_and_uniform(M, B, T):
    """Both sides of the sort / hash switch (M <= 8192 | M > 8192) and the worst
    allowed collision rate B / M = 1 / 8.  Each index is included in a draw with
    probability p = B / M; over T independent draws its count c_i is Binomial(T,
    p), and (the counts summing to T B) sum (c_i - T p)^2 / (T p (1 - p)) is
    chi-squared with M - 1 degrees of freedom up to O(1 / T)."""
    counts = np.zeros(M, dtype=np.int64)
    for t in range(1, T + 1):
        idx = np.asarray(orp.sample_indices(42, t, M, B)).astype(np.int64)
        assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < M
        assert np.unique(idx).size == B
        counts[idx] += 1
    p = B / M
    chi2 = np.sum((counts - T * p) ** 2) / (T * p * (1 - p))
    z = (chi2 - (M - 1)) / np.sqrt(2.0 * (M - 1))
    print(f"M {M} B {B} T {T}: chi2 {chi2:.1f} on {M - 1} dof, standardised {z:+.2f}")
    assert abs(z) <= 4.0


def test_sample_indices_counter_high_word():
    for M in (300, 20000):
        lo = np.asarray(orp.sample_indices(42, 5, M, 37))
        hi = np.asarray(orp.sample_indices(42, 2 ** 33 + 5, M, 37))
        assert not np.array_equal(lo, hi)
