"""The policy's own Philox noise — acting and the learner's update — against
its restatement (oracle.philox.policy_noise) — GPU only.

Every other numeric test of acting and of the update injects its noise.  The
training loop never does: the acting kernels and the row kernels draw with
rlmd_policy.h policy_draw.  Here the production branches run and the oracle is
fed the restated draw: key, row, counter, tag and component of every element
are pinned (tests/test_oracle_noise_cpu.py shows that a draw keyed differently
is off by more than 0.1 in 94 % of its elements, and that the restatement is
the i.i.d. standard normal the reference asks for).

The device's Box-Muller is f32 with the hardware log / sin / cos, the
restatement f64 rounded once.  NOISE_DEV bounds the difference on a unit
normal; it is measured in test_td3_acting_noise_read_out against the
restatement and set to 8 x the worst value seen there (DESIGN.md "parity
tolerances"), below the cap of 1e-3.  The acting comparisons widen the act
tolerance (rtol 1e-5, atol 1e-6) by NOISE_DEV x the largest d action / d noise
of the case (sigma x max_action for SAC, the policy noise for TD3) and no
further; the Laplace uniform is restated bit for bit and gets no widening.
The learner comparisons use the bounds of tests/test_learn_gpu.py unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import learn as ol
from oracle import philox as px
from tests.test_learn_gpu import test_full_size_fp32_matches_oracle as fp32_vs_oracle
from tests.test_learn_lattice_gpu import run as learner_vs_oracle
from tests.test_train_gpu import _flat_init, read_ring

pytestmark = pytest.mark.gpu

SEED = 12345  # the agents' Philox seed
ROWS = 4099  # ragged against every block size used
COUNTERS = [7, 2 ** 31 + 3]
NOISE_DEV_CAP = 1e-3
# 8 x the worst |device - restatement| measured over test_td3_acting_noise_read_out's
# eight cases (1.33e-6 .. 1.56e-6 at |z| up to 4.2, mean 9e-8): the hardware
# transcendentals may differ by a few ulp between driver versions and |z| reaches 5.8
NOISE_DEV = 8 * 1.56e-6
assert NOISE_DEV <= NOISE_DEV_CAP


def _agent_and_oracle(dev, algo, S, A, h1, h2, precision, dist="N", init_seed=2):
    from rlmd_amd.agent import DeviceAgent, reference_init

    init = reference_init(algo, S, A, h1, h2, seed=init_seed)
    ag = DeviceAgent(algo, S, A, h1, h2, 512, 256, init=init, precision=precision, policy_dist=dist, seed=SEED,
                     device=dev)
    p, t = _flat_init(algo, S, A, h1, h2, init)
    return ag, ol.OracleLearner(algo, S, A, h1, h2, 512, 256, "MSE", p, t, s_dist=dist)


def _observations(S, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((ROWS, S)).astype(np.float32))


def _act_noise(dist, seed, ctr, n, A):
    return torch.from_numpy(px.policy_noise(dist, px.act_key(seed), np.arange(n), ctr, px.TAG_ACT_NOISE, A))


def noise_gain(ora, actor, obs, dist):
    """The largest |d action / d noise| over the rows: TD3 policy_noise (already
    times max_action); SAC N sigma max_action, MVN sqrt(sigma) max_action."""
    if ora.algo == "TD3":
        return ora.policy_noise
    with torch.no_grad():
        h, _ = ol.mlp(actor, obs, "pi")
        scale = F.linear(h, actor["log_scale.weight"], actor["log_scale.bias"]).clamp(ora.ls_min, ora.ls_max).exp()
    return float((scale.sqrt() if dist == "MVN" else scale).max()) * ora.max_action


def assert_act_close(got, ref, widen, msg):
    """The project's act tolerance (rtol 1e-5, atol 1e-6), atol widened by `widen`."""
    err = (got.double() - ref.double()).abs()
    bound = 1e-6 + widen + 1e-5 * ref.double().abs()
    print(f"{msg}: max |diff| {err.max().item():.3g} (atol 1e-6 + {widen:.3g}), rows outside "
          f"{(err > bound).any(1).float().mean().item():.4f}")
    assert bool((err <= bound).all()), f"{msg}: max |diff| {err.max().item():.3g}"


@pytest.mark.parametrize("ctr", COUNTERS)
@pytest.mark.parametrize("precision,S,A,h1,h2", [("fp32", 6, 2, 400, 300), ("fp32", 5, 1, 64, 48),
                                                 ("bf16", 6, 2, 400, 300), ("bf16", 12, 3, 400, 300)])
def test_td3_acting_noise_read_out(dev, precision, S, A, h1, h2, ctr):
    """TD3 acts with clamp(det + policy_noise z): where the clamp is inactive the
    device's z is (sto - det) / policy_noise, read out directly and compared with
    the restatement: the one place where the f32 Box-Muller's own error shows.
    The f32 sum det + noise rounds at half an ulp of 1 (6e-8), 6e-7 on z.
    fp32: actor_head_kernel (64/48: after the generic GEMMs); bf16 6/2: the fused
    acting kernel, 12/3 its wide-action instantiation (the second Philox block)."""
    ag, ora = _agent_and_oracle(dev, "TD3", S, A, h1, h2, precision)
    obs = _observations(S)
    z_ref = _act_noise("N", SEED, ctr, ROWS, A)
    with torch.no_grad():
        ref_det = ora.policy(ora.nets(ora.P)["actor"], obs, None, stochastic=False)[0]
        det = ag.act(obs, mode=1).cpu()
        sto = ag.act(obs, mode=0, noise_ctr=ctr).cpu()
    # the oracle's policy on the CPU: at the reference's init the clamp is rarely active
    free_ref = ((ref_det + z_ref * ora.policy_noise).abs() < ora.max_action)
    assert free_ref.float().mean().item() >= 0.95
    free = (det + (sto - det)).abs() < ora.max_action
    assert free.float().mean().item() >= 0.95
    z_dev = (sto.double() - det.double()) / ora.policy_noise
    dev_err = (z_dev - z_ref.double()).abs()[free]
    print(f"TD3 {precision} {S}/{A} {h1}/{h2} ctr {ctr}: unclamped {free.float().mean().item():.4f}, "
          f"noise deviation max {dev_err.max().item():.3g}, mean {dev_err.mean().item():.3g}, "
          f"max |z| {z_ref.abs().max().item():.2f}")
    assert dev_err.max().item() <= NOISE_DEV
    # the clamped elements sit on the bound the restated noise pushes them to
    clamped = ~free
    if clamped.any():
        assert torch.equal(sto[clamped].sign(), (ref_det + z_ref * ora.policy_noise)[clamped].sign())


ACT_CASES = [("SAC", 5, 1, 256, 256, "bf16", "N"), ("SAC", 6, 2, 256, 256, "bf16", "N"),
             ("SAC", 5, 3, 256, 256, "bf16", "N"), ("SAC", 16, 4, 256, 256, "bf16", "N"),
             ("SAC", 17, 3, 64, 48, "bf16", "N"), ("SAC", 6, 2, 256, 256, "fp32", "N"),
             ("SAC", 6, 2, 256, 256, "fp32", "L"), ("SAC", 6, 2, 256, 256, "bf16", "L"),
             ("SAC", 6, 2, 256, 256, "fp32", "MVN"), ("SAC", 6, 2, 256, 256, "bf16", "MVN"),
             ("TD3", 5, 1, 256, 256, "bf16", "N")]


@pytest.mark.parametrize("ctr", COUNTERS)
@pytest.mark.parametrize("algo,S,A,h1,h2,precision,dist", ACT_CASES)
def test_philox_acting_equals_injected_restatement(dev, algo, S, A, h1, h2, precision, dist, ctr):
    """act(obs, noise_ctr = c) against act(obs, eps = policy_noise(c)) on the same
    agent: the injected path is pinned to the oracle elsewhere
    (tests/test_train_gpu.py) and the two differ only in where the noise comes
    from.  bf16 256/256 with A = 1..4: the fused kernel and its wide-action
    instantiation; 17/3 64/48 the generic path; fp32 actor_head_kernel.
    Control: the noise of c + 1 misses the same bound in more than half the rows."""
    ag, ora = _agent_and_oracle(dev, algo, S, A, h1, h2, precision, dist)
    obs = _observations(S, seed=1)
    d = dist if algo == "SAC" else "N"
    with torch.no_grad():
        phil = ag.act(obs, mode=0, noise_ctr=ctr).cpu()
        inj = ag.act(obs, mode=0, eps=_act_noise(d, SEED, ctr, ROWS, A)).cpu()
        wrong = ag.act(obs, mode=0, eps=_act_noise(d, SEED, ctr + 1, ROWS, A)).cpu()
    widen = 0.0 if d == "L" else NOISE_DEV * noise_gain(ora, ora.nets(ora.P)["actor"], obs, d)
    assert_act_close(phil, inj, widen, f"{algo} {S}/{A} {h1}/{h2} {precision} {dist} ctr {ctr}")
    off = ((phil.double() - wrong.double()).abs() > 1e-6 + widen + 1e-5 * wrong.double().abs()).any(1)
    print(f"control (noise of ctr + 1): {off.float().mean().item():.4f} of rows outside the bound")
    assert off.float().mean().item() > 0.5


@pytest.mark.parametrize("algo,env,inv,fused", [("SAC", "gbm", "A", 1), ("SAC", "gbm", "A", 0), ("TD3", "gbm", "A", 1),
                                                ("TD3", "gbm", "A", 0), ("SAC", "dice_sh", "B", 1)])
def test_train_step_acts_with_restated_noise(dev, algo, env, inv, fused):
    """Inside rlmd_train_step (the fused act + env launch, and acting then env):
    the actions a step stores in the ring are the policy's on the step's
    observations with the noise of key act_key(seed), row = lane, counter =
    cum_step before the step.  dice_sh B has three actions (the MA = 4
    instantiation of the fused body)."""
    from rlmd_amd.agent import reference_init
    from rlmd_amd.trainer import VecTrainer

    N = 256
    tr = VecTrainer(env, inv, N, algo=algo, k_updates=0, warmup_steps=0, smoothing_window=0, precision="bf16",
                    seed=11, init_seed=11, replay_capacity=N * 8, device=dev)
    tr.set_fused(fused)
    S, A = tr.env.state_dim, tr.env.action_dim
    assert A == (3 if env == "dice_sh" else 1)
    h1, h2 = tr.agent.h1, tr.agent.h2
    p, t = _flat_init(algo, S, A, h1, h2, reference_init(algo, S, A, h1, h2, seed=11))
    ora = ol.OracleLearner(algo, S, A, h1, h2, tr.batch, tr.topk, "MSE", p, t)
    actor = ora.nets(ora.P)["actor"]
    for t_ in range(4):
        obs = tr.obs.clone()
        cs = tr.cum_step
        assert cs == t_
        tr.step()
        assert tr.last_fused() == bool(fused)
        stored = torch.from_numpy(read_ring(tr, t_ * N, N)[1])
        with torch.no_grad():
            ref = tr.agent.act(obs, mode=0, eps=_act_noise("N", 11, cs, N, A)).cpu()
            wrong = tr.agent.act(obs, mode=0, eps=_act_noise("N", 11, cs + 1, N, A)).cpu()
        widen = NOISE_DEV * noise_gain(ora, actor, obs.cpu(), "N")
        assert_act_close(stored, ref, widen, f"{algo} {env} fused {fused} step {t_}")
        assert ((stored - wrong).abs() > 1e-6 + widen + 1e-5 * wrong.abs()).any(1).float().mean().item() > 0.5


# (algo, S, A, h1, h2, B, k), the bf16 oracle's actor half
LEARN_CASES = [(("SAC", 5, 1, 64, 64, 48, 24), None), (("SAC", 6, 2, 256, 256, 200, 100), None),
               (("SAC", 5, 3, 64, 64, 48, 24), "chain"), (("SAC", 4, 4, 64, 64, 272, 136), "chain"),
               (("TD3", 6, 2, 400, 300, 200, 100), None)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case,actor_path", LEARN_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_learner_draws_restated_noise(dev, precision, case, actor_path):
    """learn_batch(..., None, None): the update draws its own noise (fwd_rows,
    qeval_rows' policy jobs), 4 consecutive updates, against the oracle fed
    policy_noise with key learn_key(seed), rows 0..B-1, counter
    learn_noise_ctr(learn_step_cntr before the update, read from the device) and
    tags EPS_NEXT / EPS_CUR (SAC), TD3_TARGET (TD3), under the bounds of
    tests/test_learn_gpu.py.
    SAC 5/1 B 48: A = 1, noise_pre + the no-load sample_rows, three full row blocks.
    SAC 6/2 256/256 B 200: A = 2, cos and sin of one Philox block; the last row
    block ragged (200 = 12 x 16 + 8).
    SAC 5/3: A > 2, the in-loop draw and the second Philox block, chain actor step.
    SAC 4/4 B 272: both components of block 1.
    TD3 6/2 400/300 B 200: the target smoothing noise and its clip; the actor
    interval is crossed."""
    learner_vs_oracle(dev, precision, case, path="fused", actor_path=actor_path, philox_seed=SEED)


@pytest.mark.parametrize("s_dist", ["L", "MVN"])
def test_learner_draws_restated_noise_policy_dists(dev, s_dist):
    fp32_vs_oracle(dev, "SAC", 6, 2, 256, 256, 200, 100, "MSE", s_dist=s_dist, check_logtemp=True, philox_seed=SEED)


def test_learner_noise_control_swapped_tags(dev):
    """The oracle fed EPS_CUR's draw as the next-action noise misses the statistics
    bound at once: the tags matter."""
    with pytest.raises(AssertionError, match="Not equal to tolerance"):
        fp32_vs_oracle(dev, "SAC", 6, 2, 256, 256, 200, 100, "MSE", philox_seed=SEED, noise_swap=True)
