"""HIP learn() (SAC / TD3) vs the reference's learn() and the oracle — GPU only.

fp32 mode (exact-f32 MFMA operands): loss statistics within 1e-4 relative;
parameters after each update within 2e-6 absolute of the reference / oracle
(Adam steps are lr = 3e-4..1e-3, so < 1 % of one step) on >= 99.9 % of
entries and within 10 % of one Adam step on all: where |grad| ~ Adam's eps
(1e-8), update = lr*m/(sqrt(v)+eps) turns fp32 summation-order noise of a
cancelling gradient into a visible fraction of lr.
bf16 mode (bf16 MFMA operands, f32 accumulate, f32 master weights) against the
bf16 oracle (oracle/learn.py precision="bf16": the same rounding points as the
fused update kernels): statistics within 1e-4 relative, parameters within 2e-6
on >= 99.9 % of entries and within 10 % of one Adam step on all, over 4
consecutive updates.
The launch chain (row backward + weight-gradient GEMM + Adam launches) is not
only what RLMD_NO_FUSED_UPDATE=1 selects: every B > 512 takes it, and so does
every critic input wider than 8 (S + A > 8: market windows, two assets); with
S + A <= 8 and more than two actions (A > 2) the critic step stays fused and
only the actor step runs as the chain.  tests/test_learn_lattice_gpu.py holds
those shapes; the helpers below serve both files.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import learn as ol
from oracle import philox as px
from tests.test_oracle_learn import NETS, TNETS, build, sd

pytestmark = pytest.mark.gpu


def device_agent(algo, S, A, h1, h2, B, k, loss, init, precision="fp32", **kw):
    from rlmd_amd.agent import DeviceAgent

    return DeviceAgent(algo, S, A, h1, h2, B, k, loss=loss, precision=precision, init=init, **kw)


def golden_init(g, case):
    out = {}
    for nm, tn in zip(NETS, TNETS):
        out[nm] = [torch.from_numpy(v) for v in sd(g, case + "/init", nm).values()]
        out[tn] = [torch.from_numpy(v) for v in sd(g, case + "/init", tn).values()]
    return out


@pytest.mark.parametrize("case", ["case0", "case1", "case2", "case3", "case4", "case5", "case6"])
def test_learn_matches_reference_golden(golden, dev, case):
    g = golden("learn.npz")
    algo, (S, A, h1, h2, B, k), lay, n, _, _ = build(g, case)
    lt = str(g[case + "/loss_fn"])
    ag = device_agent(algo, S, A, h1, h2, B, k, lt, golden_init(g, case), policy_dist=str(g[case + "/s_dist"]))
    rep = {x: torch.from_numpy(g[f"{case}/replay/{x}"]) for x in ("state", "action", "reward", "next_state", "done")}
    for s in range(int(g[case + "/n_steps"])):
        idx = torch.from_numpy(g[f"{case}/step{s}/idx"])
        if algo == "SAC":
            ea, eb = (torch.from_numpy(g[f"{case}/step{s}/eps_{x}"]) for x in ("next", "cur"))
        else:
            ea, eb = torch.from_numpy(g[f"{case}/step{s}/eps_target"]), None
        st = ag.learn_batch(rep["state"][idx], rep["action"][idx], rep["reward"][idx], rep["next_state"][idx],
                            rep["done"][idx], ea, eb).double().cpu().numpy()
        ref_loss = g[f"{case}/step{s}/loss"]
        np.testing.assert_allclose(st[:11], ref_loss, rtol=1e-4, atol=1e-6, equal_nan=True, err_msg=f"step {s}")
        np.testing.assert_allclose(st[12:16], g[f"{case}/step{s}/loss_params"], rtol=1e-4, atol=1e-6)
        if algo == "SAC":
            np.testing.assert_allclose(st[11], g[f"{case}/step{s}/logtemp"], rtol=1e-5, atol=1e-7)
        ref_p = ol.flatten({nm: sd(g, f"{case}/step{s}", nm) for nm in NETS}, lay, n)
        ref_t = ol.flatten({nm: sd(g, f"{case}/step{s}", tn) for nm, tn in zip(NETS, TNETS)}, lay, n)
        np.testing.assert_allclose(ag.params.cpu().numpy(), ref_p, rtol=0, atol=2e-6, err_msg=f"step {s} params")
        np.testing.assert_allclose(ag.target.cpu().numpy(), ref_t, rtol=0, atol=2e-6, err_msg=f"step {s} targets")


def assert_stats_close(st, loss_o, lt_o, lp_o, rtol, msg, logtemp=False):
    """One update's statistics row (loss[11] | logtemp | loss_params[4]) against the
    oracle's: rtol as given (2e-4 fp32, 1e-4 bf16), atol 1e-6; logtemp: also SAC's
    log temperature."""
    ref = np.concatenate([np.asarray(loss_o, np.float64), np.asarray(lp_o, np.float64)])
    got = np.concatenate([st[:11], st[12:16]])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
    print(f"{msg} statistics: max relative difference {np.nanmax(rel):.3g}")
    np.testing.assert_allclose(st[:11], loss_o, rtol=rtol, atol=1e-6, equal_nan=True, err_msg=msg)
    np.testing.assert_allclose(st[12:16], lp_o, rtol=rtol, atol=1e-6, err_msg=f"{msg} loss_params")
    if logtemp:
        np.testing.assert_allclose(st[11], lt_o, rtol=1e-5, atol=1e-7, err_msg=f"{msg} logtemp")


def assert_params_close(got, ref, lr, msg, max_lr_frac=0.1):
    # Adam divides by sqrt(v): a near-zero gradient whose fp32 summation order
    # differs can move one element by a visible fraction of lr, so the bound on
    # the worst element is a fraction of lr and the bulk must agree to 2e-6.
    # lr: one learning rate, or one per entry (actor and critics stepped apart).
    diff = np.abs(got - ref)
    frac = np.mean(diff <= 2e-6)
    print(f"{msg}: within 2e-6 {frac:.6f}, max {diff.max():.3g}, max / lr {np.max(diff / lr):.4f}")
    assert frac >= 0.999, f"{msg}: only {frac:.6f} within 2e-6 (max {diff.max():.3g})"
    assert np.all(diff <= max_lr_frac * lr), f"{msg}: max diff {diff.max():.3g} > {max_lr_frac:.0%} of lr"


FULL = [("SAC", 5, 1, 256, 256, 512, 256), ("TD3", 6, 2, 400, 300, 200, 100), ("SAC", 6, 2, 256, 256, 512, 256)]

# DeviceAgent keywords -> OracleLearner's names for the same settings
ORACLE_KW = {"initial_logtemp": "logtemp", "cauchy_scale": "cauchy", "actor_update_interval": "actor_interval",
             "temp_update_interval": "temp_interval"}


def oracle_kw(agent_kw):
    return {ORACLE_KW.get(k, k): v for k, v in agent_kw.items()}


def lr_of(algo, lay, n, agent_kw):
    """The learning rate of every parameter entry: one number when actor and
    critics share it, else a vector over the flat layout."""
    base = 3e-4 if algo == "SAC" else 1e-3
    la, lc = agent_kw.get("lr_actor") or base, agent_kw.get("lr_critic") or base
    if la == lc:
        return la
    lr = np.full(n, lc, dtype=np.float64)
    lr[:lay["critic_1"][0][2]] = la
    return lr


def set_cu_budget(ag, n_cu):
    """rlmd_agent_set_cu_budget: the CUs the learner's launches may count on (the
    column splits of fwd_rows / qeval_rows stay off when their grids exceed it)."""
    from rlmd_amd import _abi

    _abi.check(_abi.lib().rlmd_agent_set_cu_budget(ag.h, int(n_cu)))


def _random_batch(rng, B, S, A):
    s = torch.from_numpy((rng.random((B, S)) * 3e-14).astype(np.float32))
    a = torch.from_numpy(rng.uniform(-0.99, 0.99, (B, A)).astype(np.float32))
    r = torch.from_numpy(rng.uniform(0.5, 1.5, B).astype(np.float32))
    s2 = torch.from_numpy((rng.random((B, S)) * 3e-14).astype(np.float32))
    d = torch.from_numpy(rng.random(B) < 0.1)
    return s, a, r, s2, d


def philox_noise(algo, s_dist, seed, updates_done, B, A, swap=False):
    """(eps_a, eps_b) the device draws for itself in the update after
    `updates_done` updates of an agent built with `seed` (learn_batch / learn
    without injected noise), restated by oracle.philox.policy_noise: eps_a is the
    next-action noise (SAC, tag EPS_NEXT) or the target smoothing noise (TD3, tag
    TD3_TARGET, always normal), eps_b the current-action noise (EPS_CUR).
    swap: eps_a drawn under EPS_CUR's tag instead (a control)."""
    dist = s_dist if algo == "SAC" else "N"
    key, ctr, rows = px.learn_key(seed), px.learn_noise_ctr(updates_done), np.arange(B)
    tag_a = px.TAG_EPS_CUR if swap else (px.TAG_EPS_NEXT if algo == "SAC" else px.TAG_TD3_TARGET)
    return (torch.from_numpy(px.policy_noise(dist, key, rows, ctr, tag_a, A)),
            torch.from_numpy(px.policy_noise(dist, key, rows, ctr, px.TAG_EPS_CUR, A)))


@functools.lru_cache(maxsize=4)
def _fp32_reference(algo, S, A, h1, h2, B, k, loss, s_dist, dup, steps, okw, philox_seed=None, swap=False):
    """The autograd oracle's run of one case, computed once and shared by the
    tests that send the same case down different device paths: (initial
    parameters, layout, [per update: the mini-batch and noise, the oracle's
    statistics, its parameters and targets after the update]).  philox_seed: the
    noise is what an agent of that seed draws for itself (philox_noise) in updates
    0 .. steps - 1 of its life, not the generator's."""
    from rlmd_amd.agent import reference_init

    init = reference_init(algo, S, A, h1, h2, seed=11)
    lay, n = ol.layout(algo, S, A, h1, h2)
    p = ol.flatten({nm: dict(zip([x[0] for x in lay[nm]], [t.numpy() for t in init[nm]])) for nm in NETS}, lay, n)
    t = ol.flatten({nm: dict(zip([x[0] for x in lay[nm]], [t.numpy() for t in init[tn]]))
                    for nm, tn in zip(NETS, TNETS)}, lay, n)
    ora = ol.OracleLearner(algo, S, A, h1, h2, B, k, loss, p, t, s_dist=s_dist, **dict(okw))
    rng = np.random.default_rng(3)
    lo = np.finfo(np.float32).eps - 1.0
    draw = (lambda: rng.uniform(lo, 1.0, (B, A))) if s_dist == "L" else (lambda: rng.standard_normal((B, A)))
    out = []
    for step in range(steps):
        s, a, r, s2, d = _random_batch(rng, B, S, A)
        if philox_seed is not None:
            ea, eb = philox_noise(algo, s_dist, philox_seed, step, B, A, swap)
        else:
            ea = torch.from_numpy(draw().astype(np.float32))
            eb = torch.from_numpy(draw().astype(np.float32))
        if dup:  # rows 2i + 1 repeat rows 2i: equal losses and actor objectives, ranked by row
            for x in (s, a, r, s2, d, ea, eb):
                x[1::2] = x[0::2]
        loss_o, lt_o, lp_o = ora.learn(s.numpy(), a.numpy(), r.numpy(), s2.numpy(), d.numpy(), ea.numpy(),
                                       eb.numpy() if algo == "SAC" else None)
        out.append(((s, a, r, s2, d, ea, eb), loss_o, lt_o, lp_o, ora.P.numpy().copy(), ora.T.numpy().copy()))
    return init, lay, n, out


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL)
@pytest.mark.parametrize("loss", ["MSE", "HUB", "MAE", "HSC"])
def test_full_size_fp32_matches_oracle(dev, algo, S, A, h1, h2, B, k, loss, max_lr_frac=0.1, s_dist="N", dup=False,
                                       steps=4, agent_kw=None, cu_budget=None, check_logtemp=False,
                                       philox_seed=None, noise_swap=False):
    """agent_kw: DeviceAgent settings away from their defaults (the oracle takes
    the same under its own names); cu_budget: rlmd_agent_set_cu_budget before
    the first update; check_logtemp: also compare SAC's log temperature.
    philox_seed: the agent is built with this seed and draws its own noise
    (learn_batch without eps, the training loop's branch); the oracle is fed the
    restated draw (philox_noise; noise_swap: its control)."""
    agent_kw = agent_kw or {}
    philox = philox_seed is not None
    init, lay, n, ref = _fp32_reference(algo, S, A, h1, h2, B, k, loss, s_dist, dup, steps,
                                        tuple(sorted(oracle_kw(agent_kw).items())), philox_seed, noise_swap)
    ag = device_agent(algo, S, A, h1, h2, B, k, loss, init, policy_dist=s_dist,
                      **(dict(agent_kw, seed=philox_seed) if philox else agent_kw))
    if cu_budget is not None:
        set_cu_budget(ag, cu_budget)
    lr = lr_of(algo, lay, n, agent_kw)
    for step, ((s, a, r, s2, d, ea, eb), loss_o, lt_o, lp_o, P_o, T_o) in enumerate(ref):
        if philox:  # the counter the reference's noise was drawn for
            assert ag.scalars()["learn_step_cntr"] == step
            ea = eb = None
        st = ag.learn_batch(s, a, r, s2, d, ea, eb if algo == "SAC" else None).double().cpu().numpy()
        assert_stats_close(st, loss_o, lt_o, lp_o, 2e-4, f"step {step}", check_logtemp and algo == "SAC")
        assert_params_close(ag.params.cpu().numpy(), P_o, lr, f"step {step} params", max_lr_frac)
        assert_params_close(ag.target.cpu().numpy(), T_o, lr, f"step {step} targets", max_lr_frac)


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL[:2])
def test_tied_rows_match_oracle(dev, algo, S, A, h1, h2, B, k):
    """Mini-batches of repeated rows: every critic loss and actor objective value
    occurs twice, so the top-k selections break ties by row (the oracle's stable
    argsort, the kernels' (value, row) keys, rlmd_block.h block_rank)."""
    test_full_size_fp32_matches_oracle(dev, algo, S, A, h1, h2, B, k, "MSE", dup=True)


@pytest.mark.parametrize("loss", ["CAU", "TCAU", "CIM", "MSE2", "MSE4", "MSE6"])
def test_remaining_losses_fp32(dev, loss):
    test_full_size_fp32_matches_oracle(dev, "SAC", 5, 1, 256, 256, 512, 256, loss)


@pytest.mark.parametrize("splits", ["4", "1"])
@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL[:2])
def test_fused_optimiser_epilogue(dev, monkeypatch, algo, S, A, h1, h2, B, k, splits):
    """RLMD_FUSE_ADAM=1: the weight-gradient GEMM's last arriving split steps the
    parameters (write-through slabs + arrival tickets; with one split straight from
    the accumulators); same numerics as adam_kernel up to the K-sum order."""
    monkeypatch.setenv("RLMD_FUSE_ADAM", "1")
    monkeypatch.setenv("RLMD_FUSE_SPLITS", splits)
    monkeypatch.setenv("RLMD_NO_FUSED_UPDATE", "1")  # the critic step through the GEMM too
    test_full_size_fp32_matches_oracle(dev, algo, S, A, h1, h2, B, k, "MSE")


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL[:2])
@pytest.mark.parametrize("loss", ["MSE", "HUB"])
def test_launch_chain_critic_step_matches_oracle(dev, monkeypatch, algo, S, A, h1, h2, B, k, loss):
    """RLMD_NO_FUSED_UPDATE=1: the critic step as row backward + weight-gradient
    GEMM + Adam launches (the path B > 512 and S + A > 8 take) against the same oracle."""
    monkeypatch.setenv("RLMD_NO_FUSED_UPDATE", "1")
    test_full_size_fp32_matches_oracle(dev, algo, S, A, h1, h2, B, k, loss)


@pytest.mark.parametrize("s_dist", ["L", "MVN"])
def test_full_size_policy_dists(dev, s_dist):
    """Laplace / MVN samplers through the whole update at full size (SAC 256/256)."""
    test_full_size_fp32_matches_oracle(dev, "SAC", 6, 2, 256, 256, 512, 256, "MSE", s_dist=s_dist)


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
def test_batch_1024_separate_actor_loss(dev, algo):
    """B > 512 routes the actor loss through actor_loss_kernel instead of abwd_rows."""
    # 1024-row sums: twice the reduction length of the 512-row cases
    test_full_size_fp32_matches_oracle(dev, algo, 5, 1, 256, 256, 1024, 512, "MSE", max_lr_frac=0.2)


def ill_conditioned(ora):
    """The elements the bf16 oracle's last update stepped with |g| < 1e-6."""
    return np.abs(np.nan_to_num(ora.last_grad.numpy(), nan=1.0)) < 1e-6


def assert_bf16_state_close(ag, ora, ill, lr, msg, max_lr_frac=0.1):
    """Device parameters and targets against the bf16 oracle's.  Bulk: >= 99.9 % of
    all entries within 2e-6; well-conditioned entries (|g| >= 1e-6 in the updates
    since the two were equal, `ill` marks the others): all within 10 % of one
    Adam step."""
    for nm, got, ref in (("params", ag.params, ora.P), ("targets", ag.target, ora.T)):
        dp = np.abs(got.cpu().numpy() - ref.numpy())
        frac = np.mean(dp <= 2e-6)
        print(f"{msg} {nm}: within 2e-6 {frac:.6f}, max {dp.max():.3g}, "
              f"max well-conditioned {dp[~ill].max():.3g}, ill-conditioned {ill.mean():.5f}")
        assert frac >= 0.999, f"{msg} {nm}: only {frac:.6f} within 2e-6"
        assert np.all((dp <= max_lr_frac * lr) | ill), f"{msg} {nm}: {dp[~ill].max():.3g} > {max_lr_frac:.0%} of lr"


def bf16_vs_oracle(algo, S, A, h1, h2, B, k, loss, steps=4, seed=5, path="fused", actor_path=None, agent_kw=None,
                   cu_budget=None, max_lr_frac=0.1, philox_seed=None):
    """The headline precision's learner against the bf16 oracle (oracle/learn.py
    precision="bf16"), state rows O(1) so that the bf16 operands carry signal.
    Every oracle update starts from the device's state (parameters, targets,
    Adam moments, Cauchy scales, log alpha): bf16 rounding makes a run chaotic in
    the few elements whose gradient is ~ Adam's eps, so each update is checked on
    its own arithmetic, over consecutive updates (Adam step counts, Polyak and
    TD3's delayed actor steps).  actor_path: the oracle's form of the actor half
    when it differs from the critic's (A > 2 on the fused critic step);
    agent_kw / cu_budget / philox_seed as in test_full_size_fp32_matches_oracle
    (the noise counter read from the device's learn_step_cntr before each update)."""
    from rlmd_amd.agent import reference_init

    init = reference_init(algo, S, A, h1, h2, seed=seed)
    lay, n = ol.layout(algo, S, A, h1, h2)
    p = ol.flatten({nm: dict(zip([x[0] for x in lay[nm]], [t.numpy() for t in init[nm]])) for nm in NETS}, lay, n)
    t = ol.flatten({nm: dict(zip([x[0] for x in lay[nm]], [t.numpy() for t in init[tn]]))
                    for nm, tn in zip(NETS, TNETS)}, lay, n)
    ora = ol.OracleLearner(algo, S, A, h1, h2, B, k, loss, p, t, precision="bf16", path=path,
                           actor_path=actor_path, **oracle_kw(agent_kw or {}))
    philox = philox_seed is not None
    ag = device_agent(algo, S, A, h1, h2, B, k, loss, init, precision="bf16",
                      **(dict(agent_kw or {}, seed=philox_seed) if philox else (agent_kw or {})))
    if cu_budget is not None:
        set_cu_budget(ag, cu_budget)
    rng = np.random.default_rng(seed + 100)
    lr = lr_of(algo, lay, n, agent_kw or {})
    # elements stepped with an ill-conditioned gradient (|g| < 1e-6, within 100x
    # of Adam's eps): there a one-ulp difference in one of the B summands (an
    # operand an f32 ulp from a bf16 rounding boundary rounds the other way in
    # one of the two) changes m / (sqrt(v) + eps) by a large fraction of a step
    for step in range(steps):
        sc = ag.scalars()
        ora.load_state(ag.params.cpu(), ag.target.cpu(), ag.adam_m.cpu(), ag.adam_v.cpu(), sc["cauchy"],
                       sc["log_alpha"])
        s, a, r, s2, d = _random_batch(rng, B, S, A)
        s = torch.from_numpy(rng.normal(0, 1, (B, S)).astype(np.float32))
        s2 = torch.from_numpy(rng.normal(0, 1, (B, S)).astype(np.float32))
        ea = torch.from_numpy(rng.standard_normal((B, A)).astype(np.float32))
        eb = torch.from_numpy(rng.standard_normal((B, A)).astype(np.float32))
        if philox:
            ea, eb = philox_noise(algo, "N", philox_seed, sc["learn_step_cntr"], B, A)
            st = ag.learn_batch(s, a, r, s2, d, None, None).double().cpu().numpy()
        else:
            st = ag.learn_batch(s, a, r, s2, d, ea, eb if algo == "SAC" else None).double().cpu().numpy()
        lo, lt_o, lp_o = ora.learn(s.numpy(), a.numpy(), r.numpy(), s2.numpy(), d.numpy(), ea.numpy(),
                                   eb.numpy() if algo == "SAC" else None)
        assert_stats_close(st, lo, lt_o, lp_o, 1e-4, f"step {step}", algo == "SAC")
        assert_bf16_state_close(ag, ora, ill_conditioned(ora), lr, f"{algo} {loss} step {step}", max_lr_frac)


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL[:2])
@pytest.mark.parametrize("loss", ["MSE", "HUB", "MAE", "HSC"])
def test_bf16_matches_bf16_oracle(dev, algo, S, A, h1, h2, B, k, loss):
    """C2's SAC 256/256 (B = 512) and C3's TD3 400/300 (B = 200) in bf16 through
    the fused update kernels (critic_update_kernel / actor_update_kernel)."""
    bf16_vs_oracle(algo, S, A, h1, h2, B, k, loss)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_narrow_tiles_ragged_edges(dev, precision):
    """The fused update kernels' 32 x 32 tile form (256 < B <= 512) where its bound
    checks bite: widths 48 / 40 are no multiples of 32 (partial tiles, zero padding
    in the copies), and B = 272 is 17 full 16-row blocks, so wave 4's 64-row slice
    holds one block and waves 5-7 none."""
    case = ("SAC", 5, 1, 48, 40, 272, 136, "MSE")
    if precision == "fp32":
        test_full_size_fp32_matches_oracle(dev, *case)
    else:
        bf16_vs_oracle(*case)


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k", FULL[:2])
@pytest.mark.parametrize("loss", ["MSE", "HUB"])
def test_bf16_launch_chain_matches_bf16_oracle(dev, monkeypatch, algo, S, A, h1, h2, B, k, loss):
    """RLMD_NO_FUSED_UPDATE=1 (the path every B > 512 and every S + A > 8 takes; A > 2
    takes its actor half): cbwd_rows / abwd_rows
    + the weight-gradient GEMM + Adam, against the bf16 oracle's chain rounding."""
    monkeypatch.setenv("RLMD_NO_FUSED_UPDATE", "1")
    bf16_vs_oracle(algo, S, A, h1, h2, B, k, loss, path="chain")


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
def test_nan_guard_sets_status(dev, algo):
    """The reference's NaN guards (tests/test_live_learning.py:29-255) as the
    sticky status word of rlmd_status_poll: a NaN reward in one mini-batch
    makes the critic target NaN (bit 0, *_critic_stability) and the critic
    statistics NaN (bit 1, critic_learning's exit() condition).  Finite batches
    before it leave the word 0; later batches do not clear it."""
    from rlmd_amd import _abi
    from rlmd_amd.agent import reference_init

    S, A, h1, h2, B, k = 5, 1, 64, 48, 64, 32
    ag = device_agent(algo, S, A, h1, h2, B, k, "MSE", reference_init(algo, S, A, h1, h2, seed=3))
    rng = np.random.default_rng(0)

    def batch(nan_row=None):
        s = torch.from_numpy(rng.normal(size=(B, S)).astype(np.float32))
        a = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, A)).astype(np.float32))
        r = torch.from_numpy(rng.normal(1.0, 0.1, B).astype(np.float32))
        if nan_row is not None:
            r[nan_row] = float("nan")
        s2 = torch.from_numpy(rng.normal(size=(B, S)).astype(np.float32))
        d = torch.zeros(B, dtype=torch.uint8)
        e = torch.from_numpy(rng.normal(size=(B, A)).astype(np.float32))
        return s, a, r, s2, d, e, (e.clone() if algo == "SAC" else None)

    for _ in range(3):
        ag.learn_batch(*batch())
    assert ag.status() == (0, -1)
    st = ag.learn_batch(*batch(nan_row=7)).cpu().numpy()
    assert np.isnan(st[0])
    flags, upd = ag.status()
    assert flags & _abi.STATUS_NAN_BATCH and flags & _abi.STATUS_NAN_STATS, flags
    assert upd >= 0
    ag.learn_batch(*batch())
    assert ag.status()[0] == flags  # sticky
    assert ag.scalars()["nan_flag"] == flags


@pytest.mark.parametrize("loss", ["CAU", "TCAU"])
def test_fused_actor_statistics_use_prestep_scalars(dev, monkeypatch, loss):
    """The fused actor step runs its two critic-statistics workgroups beside the
    workgroups that write log_alpha (temperature step) and the Nagy Cauchy scales
    in the same launch.  The scalars live in update-parity slots of LearnState
    (update n reads slot (n - 1) & 1 and writes slot n & 1), so the statistics
    read the starting values without ordering against their writers; their
    statistics, the Cauchy scales (the next
    update's CAU / TCAU loss scale) and log alpha must match the launch chain
    (RLMD_NO_FUSED_ACTOR=1: statistics in abwd_rows' own workgroup, temperature in
    adam_kernel after it) over consecutive SAC updates with a temperature step."""
    from rlmd_amd.agent import reference_init

    S, A, h1, h2, B, k = 5, 1, 256, 256, 512, 256
    init = reference_init("SAC", S, A, h1, h2, seed=21)
    rng = np.random.default_rng(8)
    batches = []
    for _ in range(6):
        s, a, r, s2, d = _random_batch(rng, B, S, A)
        r = r * 3.0  # targets well away from q: the Nagy update moves the scale
        batches.append((s, a, r, s2, d, torch.from_numpy(rng.standard_normal((B, A)).astype(np.float32)),
                        torch.from_numpy(rng.standard_normal((B, A)).astype(np.float32))))
    out = {}
    for mode in ("fused", "chain"):
        if mode == "chain":
            monkeypatch.setenv("RLMD_NO_FUSED_ACTOR", "1")
        ag = device_agent("SAC", S, A, h1, h2, B, k, loss, init)
        rows = []
        for bt in batches:
            st = ag.learn_batch(*bt).double().cpu().numpy().copy()
            sc = ag.scalars()
            rows.append((st, sc["cauchy"], sc["log_alpha"]))
        out[mode] = rows
    for i, ((sf, cf, af), (sc_, cc, ac)) in enumerate(zip(out["fused"], out["chain"])):
        np.testing.assert_allclose(sf[:16], sc_[:16], rtol=1e-5, atol=1e-7, equal_nan=True, err_msg=f"update {i}")
        np.testing.assert_allclose(cf, cc, rtol=1e-5, err_msg=f"update {i} Cauchy scales")
        np.testing.assert_allclose(af, ac, rtol=1e-5, atol=1e-7, err_msg=f"update {i} log alpha")
    # the scales moved: the Nagy update is exercised, not held at its initial 1.0
    assert abs(out["fused"][-1][1][0] - 1.0) > 1e-3
