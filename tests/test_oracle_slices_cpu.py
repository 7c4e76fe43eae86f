"""The shared-slice market mode (slice_groups = G) of the CPU oracle — CPU only.

C4 is benched and trained with G = 1: every lane draws its episode start row
and its block shuffles from the Philox stream keyed on lane % G, the vectorised
form of the reference loop's one time_slice + shuffle_data per episode
(scripts/rl_market.py:202-214, tools/env_resources.py:229-291).  The episode
index stays the lane's own, so two lanes of a group trade the same slice only
while they are at the same episode index.  These tests pin the oracle's
restatement of that rule (oracle/envs.py OracleVecEnv(slice_groups=G)) against
its per-lane mode, which the golden traces pin to the reference; the GPU tests
(test_env_gpu.py, test_fused_env_gpu.py, test_train_gpu.py,
test_fullsize_gpu.py) then hold every market kernel to it.

The helpers below are shared with those GPU tests.
"""
import numpy as np
import pytest

from oracle import envs as oe
from oracle import philox as px

N, T, SEED = 200, 40, 99
SHAPES = [(oe.INV_A, 1, 1), (oe.INV_A, 3, 2), (oe.INV_C, 1, 1), (oe.INV_C, 3, 2)]  # (investor, obs_days, assets)


def slice_market_kw(golden, obs_days, assets, shuffle_days=5, days=12):
    """`days`-day episodes on stooq_usei[:600]'s first `assets` columns."""
    prices = np.ascontiguousarray(golden("market.npz")["prices"][:, :assets])
    return dict(prices=prices, obs_days=obs_days, time_length=days + obs_days - 1, shuffle_days=shuffle_days,
                sample_days=days + obs_days + 40)


def slice_actions(rng, n_lanes, action_dim):
    """Uniform in +-0.99, 5 % of the rows at 0.99 in every column (lev_max ends those
    lanes' episodes early, so a group's lanes leave the lock-step)."""
    a = rng.uniform(-0.99, 0.99, (n_lanes, action_dim)).astype(np.float32)
    a[rng.random(n_lanes) < 0.05] = np.float32(0.99)
    return a


def groups_desynced(episode, G):
    """True if two lanes of one group (lane % G) are at different episode indices."""
    episode = np.asarray(episode)
    key = np.arange(episode.size) % G
    return any(np.unique(episode[key == k]).size > 1 for k in range(min(G, episode.size)))


def assert_equal_index_shares_slice(ora, G, msg=""):
    """Lanes of one group at equal episode index: one start, one row map."""
    seen = {}
    for lane in range(ora.N):
        k = (lane % G, int(ora.episode[lane]))
        if k in seen:
            first = seen[k]
            assert ora.start[lane] == ora.start[first], f"{msg} lanes {first}, {lane} start"
            np.testing.assert_array_equal(ora.rowmap[lane], ora.rowmap[first], err_msg=f"{msg} lanes {first}, {lane}")
        else:
            seen[k] = lane


def assert_rowmap_shape(ora, lanes=None):
    """Every row map permutes start .. start + ext_len - 1 and maps each block of
    shuffle_days rows (the short last block too) onto itself."""
    L, D = ora.ext_len, ora.shuffle_days
    blocks = np.arange(L) // D
    for lane in (range(ora.N) if lanes is None else lanes):
        rel = ora.rowmap[lane] - ora.start[lane]
        np.testing.assert_array_equal(np.sort(rel), np.arange(L), err_msg=f"lane {lane}")
        np.testing.assert_array_equal(rel // D, blocks, err_msg=f"lane {lane}")
        assert 0 <= ora.start[lane] < ora.start_range


def _run(golden, inv, d, n, G, steps=T, check=None, **kw):
    """The 200-lane recipe; returns the per-step outputs and bookkeeping."""
    mkw = slice_market_kw(golden, d, n, **kw)
    ora = oe.OracleVecEnv(oe.MARKET, inv, N, n, seed=SEED, slice_groups=G, **mkw)
    rng = np.random.default_rng(5)
    log = []
    for t in range(steps):
        ns, r, dn, risk = ora.step(slice_actions(rng, N, ora.A))
        mask = dn[:, 0]
        s0 = ora.reset(mask) if mask.any() else None
        log.append((ns, r, dn, risk, s0, ora.start.copy(), ora.episode.copy(), [m for m in ora.rowmap]))
        if check is not None:
            check(ora, t)
    return ora, log


@pytest.mark.parametrize("inv,d,n", SHAPES)
@pytest.mark.parametrize("extra", [0, 7])
def test_groups_of_one_lane_equal_per_lane_mode(golden, inv, d, n, extra):
    """G >= N: lane % G is the lane, so everything equals G = 0 bit for bit."""
    _, a = _run(golden, inv, d, n, 0)
    _, b = _run(golden, inv, d, n, N + extra)
    assert len(a) == len(b) == T
    for t, (x, y) in enumerate(zip(a, b)):
        for i, name in enumerate(("next_state", "reward", "done", "risk")):
            np.testing.assert_array_equal(x[i], y[i], err_msg=f"t={t} {name}")
        assert (x[4] is None) == (y[4] is None)
        if x[4] is not None:
            np.testing.assert_array_equal(x[4], y[4], err_msg=f"t={t} reset state")
        np.testing.assert_array_equal(x[5], y[5], err_msg=f"t={t} start")
        np.testing.assert_array_equal(x[6], y[6], err_msg=f"t={t} episode")
        for lane in range(N):
            np.testing.assert_array_equal(x[7][lane], y[7][lane], err_msg=f"t={t} lane {lane} rows")


def test_nonpositive_groups_mean_per_lane(golden):
    """G <= 0 is per lane, as env.hip clamps it."""
    kw = slice_market_kw(golden, 1, 1)
    ref = oe.OracleVecEnv(oe.MARKET, oe.INV_A, N, 1, seed=SEED, **kw)
    for G in (0, -5):
        ora = oe.OracleVecEnv(oe.MARKET, oe.INV_A, N, 1, seed=SEED, slice_groups=G, **kw)
        np.testing.assert_array_equal(ora.start, ref.start)
        assert np.unique(ora.start).size > N // 4  # per-lane draws
        for lane in range(N):
            np.testing.assert_array_equal(ora.rowmap[lane], ref.rowmap[lane])


@pytest.mark.parametrize("inv,d,n", SHAPES)
@pytest.mark.parametrize("G", [1, 3, 64])
def test_equal_episode_index_shares_the_slice(golden, inv, d, n, G):
    """At every step and in every group, lanes at equal episode index have equal
    start and equal row maps; each (group, episode) slice is the one the per-lane
    mode gives lane `group` at that episode (the keying rule itself); lanes that
    ended early are on another slice than their group mates (asserted, so that a
    change of inputs cannot hollow this out); row maps keep their shape."""
    # the per-lane mode's slices of lanes 0 .. G-1, episode by episode
    kw = slice_market_kw(golden, d, n)
    per_lane = oe.OracleVecEnv(oe.MARKET, inv, min(G, N), n, seed=SEED, **kw)
    slices = []

    def slice_of(key, ep):
        while len(slices) <= ep:
            slices.append((per_lane.start.copy(), [m for m in per_lane.rowmap]))
            per_lane.reset()
        return slices[ep][0][key], slices[ep][1][key]

    desync = []

    def check(ora, t):
        assert_equal_index_shares_slice(ora, G, f"t={t}")
        assert_rowmap_shape(ora)
        for lane in range(N):
            start, rows = slice_of(lane % G, int(ora.episode[lane]))
            assert ora.start[lane] == start, f"t={t} lane {lane}"
            np.testing.assert_array_equal(ora.rowmap[lane], rows, err_msg=f"t={t} lane {lane}")
        desync.append(groups_desynced(ora.episode, G))

    ora, _ = _run(golden, inv, d, n, G, check=check)
    assert any(desync), "no group ever held lanes at different episode indices"
    assert ora.episode.max() > ora.episode.min()
    # different episodes of one key are different slices (the episode index is in the counter)
    s0, r0 = slice_of(0, 0)
    s1, r1 = slice_of(0, 1)
    assert s0 != s1 or not np.array_equal(r0 - s0, r1 - s1)


def _fisher_yates_16(seed, key, ep, blk):
    """A 16-row block's permutation written out: fifteen draws, word k of the
    stream is word k % 4 of Philox call blk * 4 + k // 4."""
    words = []
    for call in range(4):
        words += [int(w) for w in px.philox(seed, key, ep, px.TAG_MKT_PERM, blk * 4 + call)]
    p = list(range(16))
    for k, i in enumerate(range(15, 0, -1)):
        j = (words[k] * (i + 1)) >> 32
        p[i], p[j] = p[j], p[i]
    return p


@pytest.mark.parametrize("G", [1, 3])
def test_block_of_sixteen_rows(golden, G):
    """shuffle_days = 16, the limit env.hip accepts: fifteen draws from four Philox
    calls per block; 40-day episodes give blocks of 16, 16 and 9 rows."""
    def check(ora, t):
        assert_equal_index_shares_slice(ora, G, f"t={t}")
        assert_rowmap_shape(ora)

    ora, _ = _run(golden, oe.INV_A, 1, 1, G, steps=8, check=check, shuffle_days=16, days=40)
    assert ora.ext_len == 41
    moved = np.zeros(16, bool)
    for lane in range(N):
        key, ep = lane % G, int(ora.episode[lane])
        rel = ora.rowmap[lane] - ora.start[lane]
        for blk in range(2):
            want = _fisher_yates_16(SEED, key, ep, blk)
            assert rel[blk * 16:(blk + 1) * 16].tolist() == [blk * 16 + x for x in want]
            moved |= np.asarray(want) != np.arange(16)
        assert sorted(rel[32:].tolist()) == list(range(32, 41))
    assert moved.all()  # every position of a block gets shuffled somewhere


@pytest.mark.parametrize("G", [1, 3])
def test_last_block_of_one_row(golden, G):
    """shuffle_days = 2 with an odd ext_len (13): six pairs and a last block of one
    row, which stays where it is and draws nothing."""
    def check(ora, t):
        assert_equal_index_shares_slice(ora, G, f"t={t}")
        assert_rowmap_shape(ora)
        for lane in range(N):
            assert ora.rowmap[lane][12] == ora.start[lane] + 12

    ora, log = _run(golden, oe.INV_A, 1, 1, G, steps=14, check=check, shuffle_days=2)
    assert ora.ext_len == 13
    swapped = [rows[0] > rows[1] for entry in log for rows in entry[7]]
    assert any(swapped) and not all(swapped)
    assert oe.block_perm(SEED, 0, 0, 6, 1) == [0]


def test_row_maps_are_memoised_per_slice(golden):
    """One row map per (key, episode, start), shared by the group's lanes."""
    kw = slice_market_kw(golden, 1, 1)
    ora = oe.OracleVecEnv(oe.MARKET, oe.INV_A, N, 1, seed=SEED, slice_groups=3, **kw)
    assert len({id(m) for m in ora.rowmap}) == 3
    assert all(ora.rowmap[lane] is ora.rowmap[lane % 3] for lane in range(N))
    with pytest.raises(ValueError):
        ora.rowmap[0][0] = 0  # shared, hence read-only
