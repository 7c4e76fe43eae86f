"""HIP env kernels vs the CPU oracle (pinned to the reference) — GPU only.

Bar: done / learn_done flags bit-exact; f64 state / reward / risk to 1e-12
relative (libm ulps between the device and glibc exp/log/cos).
"""
import numpy as np
import pytest
import torch

from oracle import envs as oe
from tests.test_oracle_golden import env_keys, parse_env_key

pytestmark = pytest.mark.gpu
RTOL = 1e-12
# Philox-mode GBM: z comes from Box–Muller with device vs glibc log/cos (1 ulp);
# r = LOG_MEAN + VOL*z cancels near r = 0, so the error is absolute: 1e-16 in
# return units = 1e-34 in MAX_VALUE-normalised state units.
ATOL_STATE, ATOL_RISK = 1e-30, 1e-12


def _venv(fam, inv, n_lanes, n, **kw):
    from rlmd_amd.envs import VecEnv

    return VecEnv(fam, inv, n_lanes, n, **kw)


def test_golden_traces_injected_draws(golden, dev):
    """Every reference trace, replicated in 64 lanes, with the reference's draws."""
    g = golden("env_traces.npz")
    for key in env_keys(g):
        fam, inv, n = parse_env_key(key)
        L = 64
        env = _venv(fam, inv, L, n)
        acts = torch.from_numpy(g[key + "/actions"]).to(dev)
        draws = torch.from_numpy(g[key + "/draws"]).to(dev)
        state = env.reset().clone()
        for t in range(acts.shape[0]):
            np.testing.assert_allclose(state.cpu().numpy(), np.broadcast_to(g[key + "/state"][t], state.shape),
                                       rtol=RTOL, err_msg=f"{key} t={t} state")
            ns, r, d, risk = env.step(acts[t].expand(L, -1).contiguous(), draws[t].expand(L, -1).contiguous())
            ns, r, d, risk = (x.cpu().numpy() for x in (ns, r, d, risk))
            np.testing.assert_allclose(ns, np.broadcast_to(g[key + "/next_state"][t], ns.shape), rtol=RTOL,
                                       err_msg=f"{key} t={t}")
            np.testing.assert_allclose(r, np.broadcast_to(g[key + "/reward"][t], r.shape), rtol=RTOL)
            np.testing.assert_array_equal(d.astype(bool), np.broadcast_to(g[key + "/done"][t], d.shape),
                                          err_msg=f"{key} t={t}")
            np.testing.assert_allclose(risk, np.broadcast_to(g[key + "/risk"][t], risk.shape), rtol=RTOL,
                                       equal_nan=True, err_msg=f"{key} t={t} risk")
            state = torch.from_numpy(ns).to(dev)
            if d[0, 0]:
                state = env.reset().clone()


CASES = [(f, i, n) for f in (oe.COIN, oe.DICE, oe.GBM) for i in (oe.INV_A, oe.INV_B, oe.INV_C) for n in (1, 3, 9)]
CASES += [(oe.DICE_SH, i, 1) for i in (oe.INV_INSURED, oe.INV_A, oe.INV_B, oe.INV_C)]


@pytest.mark.parametrize("fam,inv,n", CASES)
def test_philox_lanes_match_oracle(fam, inv, n, dev):
    """1024 lanes, 40 steps of Philox draws with mask resets: HIP == oracle."""
    N, T, seed = 1024, 40, 1234 + 7 * fam + inv
    env = _venv(fam, inv, N, n, seed=seed)
    ora = oe.OracleVecEnv(fam, inv, N, n, seed=seed)
    rng = np.random.default_rng(seed)
    for t in range(T):
        a = rng.uniform(-0.99, 0.99, (N, env.action_dim)).astype(np.float32)
        a[rng.random(N) < 0.05] = np.float32(0.99)
        a[rng.random(N) < 0.05] = 0.0
        ns, r, d, risk = (x.cpu().numpy() for x in env.step(torch.from_numpy(a).to(dev)))
        ons, orr, od, orisk = ora.step(a)
        np.testing.assert_array_equal(d.astype(bool), od, err_msg=f"t={t}")
        np.testing.assert_allclose(ns, ons, rtol=RTOL, atol=ATOL_STATE, err_msg=f"t={t}")
        np.testing.assert_allclose(r, orr, rtol=RTOL)
        np.testing.assert_allclose(risk, orisk, rtol=RTOL, atol=ATOL_RISK, equal_nan=True)
        mask = od[:, 0]
        if mask.any():
            s_gpu = env.reset(torch.from_numpy(mask).to(dev)).cpu().numpy()
            s_ora = ora.reset(mask)
            np.testing.assert_allclose(s_gpu[mask], s_ora[mask], rtol=RTOL)
    w, tt = env.lane_state()
    np.testing.assert_allclose(w, ora.wealth, rtol=RTOL)
    np.testing.assert_array_equal(tt, ora.time)


@pytest.mark.parametrize("inv,d", [(i, d) for i in (oe.INV_A, oe.INV_B, oe.INV_C) for d in (1, 4)])
def test_market_episode_golden(golden, dev, inv, d):
    g = golden("market_env.npz")
    key = "Market_Inv%s_%s" % ("ABC"[inv], "D1" if d == 1 else "Dx")
    ext = g[key + "/extract"]
    env = _venv(oe.MARKET, inv, 8, ext.shape[1], prices=ext, obs_days=d,
                time_length=int(g[key + "/time_length"]), shuffle_days=1, sample_days=ext.shape[0] - 1)
    acts = g[key + "/actions"]
    state = env.reset().cpu().numpy()
    for t in range(acts.shape[0]):
        np.testing.assert_allclose(state[0], g[key + "/state"][t], rtol=RTOL)
        ns, r, dn, risk = (x.cpu().numpy() for x in env.step(torch.from_numpy(np.repeat(acts[t:t + 1], 8, 0)).to(dev)))
        np.testing.assert_allclose(ns, np.broadcast_to(g[key + "/next_state"][t], ns.shape), rtol=RTOL)
        np.testing.assert_allclose(r, np.broadcast_to(g[key + "/reward"][t], r.shape), rtol=RTOL)
        np.testing.assert_array_equal(dn.astype(bool), np.broadcast_to(g[key + "/done"][t], dn.shape))
        np.testing.assert_allclose(risk, np.broadcast_to(g[key + "/risk"][t], risk.shape), rtol=RTOL, equal_nan=True)
        state = ns


@pytest.mark.parametrize("inv,d", [(oe.INV_A, 1), (oe.INV_C, 3)])
def test_market_shuffled_lanes_match_oracle(golden, dev, inv, d):
    """Philox episode starts + in-block shuffles (interval 5) on real prices."""
    prices = golden("market.npz")["prices"]  # stooq_usei[:600]
    N, tl, seed = 256, 40, 99
    sample_days = tl + d + 30
    kw = dict(obs_days=d, time_length=tl, shuffle_days=5, sample_days=sample_days)
    env = _venv(oe.MARKET, inv, N, prices.shape[1], prices=prices, seed=seed, **kw)
    ora = oe.OracleVecEnv(oe.MARKET, inv, N, prices.shape[1], prices=prices, seed=seed, **kw)
    np.testing.assert_allclose(env.reset().cpu().numpy(), ora.reset(), rtol=RTOL)
    rng = np.random.default_rng(5)
    for t in range(60):
        a = rng.uniform(-0.99, 0.99, (N, env.action_dim)).astype(np.float32)
        ns, r, dn, risk = (x.cpu().numpy() for x in env.step(torch.from_numpy(a).to(dev)))
        ons, orr, od, orisk = ora.step(a)
        np.testing.assert_array_equal(dn.astype(bool), od)
        np.testing.assert_allclose(ns, ons, rtol=RTOL)
        np.testing.assert_allclose(r, orr, rtol=RTOL)
        mask = od[:, 0]
        if mask.any():
            s_gpu = env.reset(torch.from_numpy(mask).to(dev)).cpu().numpy()
            np.testing.assert_allclose(s_gpu[mask], ora.reset(mask)[mask], rtol=RTOL)


def _shared_slice_run(golden, dev, inv, d, n, G, shuffle_days=5, days=12):
    """The 200-lane, 40-step recipe of tests/test_oracle_slices_cpu.py on the
    stand-alone kernels (env_reset_kernel / env_step_kernel<MARKET>) with
    VecEnv(slice_groups=G), masked resets after every step; the device's own done
    flags drive its resets and the episode bookkeeping the desynchronisation
    condition is read from."""
    from tests.test_oracle_slices_cpu import N, SEED, T, groups_desynced, slice_actions, slice_market_kw

    kw = slice_market_kw(golden, d, n, shuffle_days=shuffle_days, days=days)
    env = _venv(oe.MARKET, inv, N, n, seed=SEED, slice_groups=G, **kw)
    ora = oe.OracleVecEnv(oe.MARKET, inv, N, n, seed=SEED, slice_groups=G, **kw)
    np.testing.assert_array_equal(env.lane_start(), ora.start)  # the constructor's reset
    np.testing.assert_allclose(env.reset().cpu().numpy(), ora.reset(), rtol=RTOL)
    np.testing.assert_array_equal(env.lane_start(), ora.start)
    rng = np.random.default_rng(5)
    ep_dev = np.ones(N, dtype=np.int64)  # the constructor's reset is episode 0
    desync, resets = [], 0
    for t in range(T):
        a = slice_actions(rng, N, env.action_dim)
        ns, r, dn, risk = (x.cpu().numpy() for x in env.step(torch.from_numpy(a).to(dev)))
        ons, orr, od, orisk = ora.step(a)
        np.testing.assert_array_equal(dn.astype(bool), od, err_msg=f"t={t}")
        np.testing.assert_allclose(ns, ons, rtol=RTOL, err_msg=f"t={t} state")
        np.testing.assert_allclose(r, orr, rtol=RTOL, err_msg=f"t={t} reward")
        np.testing.assert_allclose(risk, orisk, rtol=RTOL, equal_nan=True, err_msg=f"t={t} risk")
        mask = dn[:, 0].astype(bool)
        if mask.any():
            s_gpu = env.reset(torch.from_numpy(mask).to(dev)).cpu().numpy()
            np.testing.assert_allclose(s_gpu[mask], ora.reset(mask)[mask], rtol=RTOL, err_msg=f"t={t} reset")
            np.testing.assert_array_equal(env.lane_start(), ora.start, err_msg=f"t={t} start")
            ep_dev[mask] += 1
            resets += int(mask.sum())
        desync.append(groups_desynced(ep_dev, G))
    np.testing.assert_array_equal(ep_dev, ora.episode)
    w, tt = env.lane_state()
    np.testing.assert_allclose(w, ora.wealth, rtol=RTOL)
    np.testing.assert_array_equal(tt, ora.time)
    assert resets > N  # early ends (lev_max) and the 12-day limit
    return desync, env, ora


@pytest.mark.parametrize("G", [1, 3, 64, 200, 207])
@pytest.mark.parametrize("inv,d,n", [(oe.INV_A, 1, 1), (oe.INV_C, 3, 2)])
def test_market_shared_slice_lanes_match_oracle(golden, dev, inv, d, n, G):
    """slice_groups = G on the stand-alone reset and step kernels: slice_key() in
    env_reset_lane's start draw and market_row's block permutations.  G = 1 is C4's
    regime, 3 and 64 leave groups of several lanes (3 does not divide 64), 200 and
    207 are G = N and G > N (every lane its own key).  Lanes that end early move
    on to their key's next slice while their group mates stay (asserted)."""
    desync, env, ora = _shared_slice_run(golden, dev, inv, d, n, G)
    if G < 200:
        assert any(desync), "no group ever held lanes at different episode indices"
        starts = env.lane_start()
        for k in range(G):  # equal key and episode index: one start row
            for e in np.unique(ora.episode[k::G]):
                assert np.unique(starts[k::G][ora.episode[k::G] == e]).size == 1
    else:
        assert not any(desync)  # groups of one lane


@pytest.mark.parametrize("inv,d,n,shuffle_days,days", [(oe.INV_A, 1, 1, 16, 40), (oe.INV_C, 3, 2, 2, 12)])
def test_market_shared_slice_block_size_limits(golden, dev, inv, d, n, shuffle_days, days):
    """market_perm at its block sizes' limits, slice_groups = 1, stand-alone kernels:
    16 rows (the largest env.hip accepts: fifteen draws from four Philox calls, all
    sixteen 4-bit entries of the packed permutation; 41 rows = blocks 16, 16, 9) and
    2 rows with an odd extract (15 rows: a last block of one row, no draw)."""
    desync, env, ora = _shared_slice_run(golden, dev, inv, d, n, 1, shuffle_days=shuffle_days, days=days)
    assert ora.ext_len % 2 == 1 and ora.shuffle_days == shuffle_days
    assert any(desync)


def test_market_negative_slice_groups_mean_per_lane(golden, dev):
    """rlmd_env_create clamps slice_groups < 0 to 0: per-lane starts after a full reset."""
    from tests.test_oracle_slices_cpu import N, SEED, slice_market_kw

    kw = slice_market_kw(golden, 1, 1)
    starts = []
    for G in (0, -5):
        env = _venv(oe.MARKET, oe.INV_A, N, 1, seed=SEED, slice_groups=G, **kw)
        env.reset()
        starts.append(env.lane_start())
    np.testing.assert_array_equal(starts[0], starts[1])
    ora = oe.OracleVecEnv(oe.MARKET, oe.INV_A, N, 1, seed=SEED, slice_groups=-5, **kw)
    ora.reset()
    np.testing.assert_array_equal(starts[1], ora.start)
    assert np.unique(starts[1]).size > N // 4
