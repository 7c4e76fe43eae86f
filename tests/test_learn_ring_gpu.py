"""The ring-fed learner, rlmd_agent_learn(rb, K) and the training step's learn
call, against the oracle — GPU only.

Every other numeric learner test injects its mini-batch (learn_batch).  The
training loop samples: agent_learn_k draws K index sets with key
replay_key(seed) and counters learn_step_cntr + i, launches
replay_sample_kernel over K x G workgroups (the trainer's later steps: draws
ahead and gathers inside fwd_rows), and each update draws its own policy noise
with counter learn_step_cntr + i + 1.  Here that path runs and is rebuilt on the
CPU: oracle.replay.sample_indices picks the host copies' rows,
oracle.philox.policy_noise the noise, OracleLearner the update.  The rewards
encode the ring row, so a gather from the wrong row or into the wrong slab
changes the critic statistics outright.  Bounds: those of
tests/test_learn_gpu.py (statistics rtol 2e-4 fp32 / 1e-4 bf16, atol 1e-6;
parameters 99.9 % within 2e-6 and the worst (bf16: worst well-conditioned)
within 10 % of lr).  fp32: the autograd oracle runs on from the initial
parameters through both calls.  bf16: those bounds are for one update from
the device's own state (bf16_vs_oracle's docstring: a bf16 run is chaotic in
the elements whose gradient is ~ Adam's eps, and Adam's first steps move every
element by lr sign(g)), and a K-update call gives no state between its
updates.  So a second agent of the same key and parameters runs the same
updates one call each, every one against the bf16 oracle started from that
agent's state, and the K-update call must equal the chain of single calls bit
for bit: statistics rows, parameters, targets and Adam moments (the sample
counters are the same, and TD3's pairing of the next target pass into the
current forward is bit-neutral, tests/test_target_pair_gpu.py).  Measured
without that, the bf16 oracle running a call's K updates on its own from the
state before the call: TD3 400/300 K = 4, first call: 99.848 % of the
parameters within 2e-6, the worst well-conditioned entry 0.7 lr away; K = 3:
first call 99.992 % (the worst ill-conditioned entry 1.8 lr away), second call
(Adam past its first steps) 100 % and 5e-7; SAC 256/256 and the trainer-level
case below stay within the bounds on their own.
"""
import numpy as np
import pytest
import torch

from oracle import learn as ol
from oracle import philox as px
from oracle.replay import MultiStepRing, sample_indices
from tests.test_learn_gpu import (_random_batch, assert_bf16_state_close, assert_params_close, assert_stats_close,
                                  device_agent, ill_conditioned, lr_of, philox_noise)
from tests.test_train_gpu import _flat_init, read_ring

pytestmark = pytest.mark.gpu

SEED = 12345


def _oracle(algo, S, A, h1, h2, B, k, init, precision):
    p, t = _flat_init(algo, S, A, h1, h2, init)
    return ol.OracleLearner(algo, S, A, h1, h2, B, k, "MSE", p, t, precision=precision)


def _oracle_call(ora, algo, seed, cntr0, K, M, B, A, rows_of):
    """The K updates of one learn call on the oracle: update i samples with counter
    cntr0 + i and draws its noise for learn_step_cntr cntr0 + i.  rows_of(idx) ->
    (s, a, r, s2, done, eff or None).  Returns the K statistics and the union of
    the updates' ill-conditioned elements (bf16 oracle; None for autograd)."""
    out, ill = [], None
    for i in range(K):
        idx = np.asarray(sample_indices(px.replay_key(seed), cntr0 + i, M, B)).astype(np.int64)
        assert np.unique(idx).size == B
        s, a, r, s2, d, eff = rows_of(idx)
        ea, eb = philox_noise(algo, "N", seed, cntr0 + i, B, A)
        out.append(ora.learn(s, a, r, s2, d, ea.numpy(), eb.numpy() if algo == "SAC" else None, eff=eff))
        if ora.explicit:
            ill = ill_conditioned(ora) if ill is None else ill | ill_conditioned(ora)
    return out, ill


def _check_call(ag, ora, algo, precision, stats, ref, ill, lr, msg):
    st = stats.double().cpu().numpy()
    for i, (loss_o, lt_o, lp_o) in enumerate(ref):
        assert_stats_close(st[i], loss_o, lt_o, lp_o, 2e-4 if precision == "fp32" else 1e-4, f"{msg} update {i}",
                           algo == "SAC")
    if precision == "fp32":
        assert_params_close(ag.params.cpu().numpy(), ora.P.numpy(), lr, f"{msg} params")
        assert_params_close(ag.target.cpu().numpy(), ora.T.numpy(), lr, f"{msg} targets")
    else:
        assert_bf16_state_close(ag, ora, ill, lr, msg)


def _sync_bf16(ora, ag):
    sc = ag.scalars()
    ora.load_state(ag.params.cpu(), ag.target.cpu(), ag.adam_m.cpu(), ag.adam_v.cpu(), sc["cauchy"], sc["log_alpha"])


RING_CASES = [("SAC", 5, 1, 256, 256, 512, 256, "bf16", 3, 3000), ("SAC", 5, 1, 256, 256, 512, 256, "bf16", 3, 9000),
              ("SAC", 5, 1, 256, 256, 512, 256, "fp32", 3, 3000), ("SAC", 5, 1, 256, 256, 512, 256, "fp32", 3, 9000),
              ("TD3", 6, 2, 400, 300, 200, 100, "bf16", 3, 9000), ("TD3", 6, 2, 400, 300, 200, 100, "bf16", 4, 9000),
              ("SAC", 6, 2, 64, 64, 48, 24, "fp32", 2, 48)]


@pytest.mark.parametrize("algo,S,A,h1,h2,B,k,precision,K,M", RING_CASES)
def test_learn_from_ring_matches_oracle(dev, algo, S, A, h1, h2, B, k, precision, K, M):
    """agent.learn(replay, K) twice (the counters continue at K) on a ring of M
    random rows.  SAC 256/256 B 512: G = 8 gather parts per mini-batch, M = 3000
    the sort regime of the draw, 9000 the hash regime.  TD3 400/300 B 200 (G = 1):
    the target pass of update i + 1 rides in update i's forward and draws with
    counter + 1; K = 3 and 4 end the call on either side of the actor interval.
    M = 48 = B: every draw is a permutation of the whole ring."""
    from rlmd_amd.agent import ReplayMemory, reference_init

    init = reference_init(algo, S, A, h1, h2, seed=7)
    ag = device_agent(algo, S, A, h1, h2, B, k, "MSE", init, precision=precision, seed=SEED)
    ora = _oracle(algo, S, A, h1, h2, B, k, init, precision)
    rng = np.random.default_rng(M + K)
    s, a, _, s2, d = (x.numpy() for x in _random_batch(rng, M, S, A))
    if precision == "bf16":  # O(1) state rows, as bf16_vs_oracle's
        s, s2 = (rng.normal(0, 1, (M, S)).astype(np.float32) for _ in range(2))
    r = (0.5 + np.arange(M) / M).astype(np.float32)  # the row index, in _random_batch's range
    assert np.unique(r).size == M
    replay = ReplayMemory(M, S, A, device=dev)
    replay.store_exp(s, a, r, s2, d)
    assert replay.mem_idx == M
    lay, n = ol.layout(algo, S, A, h1, h2)
    lr = lr_of(algo, lay, n, {})
    rows_of = lambda idx: (s[idx], a[idx], r[idx], s2[idx], d[idx], None)
    single = None
    if precision == "bf16":  # a second agent of the same key and parameters, fed one update per call
        single = device_agent(algo, S, A, h1, h2, B, k, "MSE", init, precision=precision, seed=SEED)
    for call in range(2):
        msg = f"{algo} {precision} M {M} K {K} call {call}"
        cntr0 = ag.scalars()["learn_step_cntr"]
        assert cntr0 == call * K
        stats = ag.learn(replay, K).clone()
        if precision == "fp32":
            ref, _ = _oracle_call(ora, algo, SEED, cntr0, K, M, B, A, rows_of)
            _check_call(ag, ora, algo, precision, stats, ref, None, lr, msg)
            continue
        rows = []
        for i in range(K):  # the same updates one call each, every one against the oracle from its own state
            assert single.scalars()["learn_step_cntr"] == cntr0 + i
            _sync_bf16(ora, single)
            rows.append(single.learn(replay, 1).clone())
            ref, ill = _oracle_call(ora, algo, SEED, cntr0 + i, 1, M, B, A, rows_of)
            _check_call(single, ora, algo, precision, rows[-1], ref, ill, lr, f"{msg} update {i} alone")
        np.testing.assert_array_equal(stats.cpu().numpy(), torch.cat(rows).cpu().numpy(), err_msg=f"{msg} statistics")
        for name in ("params", "target", "adam_m", "adam_v"):
            assert torch.equal(getattr(ag, name), getattr(single, name)), f"{msg}: {name} differ from K single calls"
    assert ag.status()[0] == 0


def test_learn_from_multistep_ring_matches_oracle(dev):
    """An n = 3 ring (dynamics "M", 8 lanes, frequent dones): the sample kernel's
    gather_row histories and eff (gamma^eff in the target) against
    MultiStepRing.gather at the restated indices.  TD3 5/1 64/48 B 200, fp32."""
    from rlmd_amd.agent import ReplayMemory, reference_init

    algo, S, A, h1, h2, B, k, K = "TD3", 5, 1, 64, 48, 200, 100, 2
    lanes, steps, n_steps = 8, 60, 3
    init = reference_init(algo, S, A, h1, h2, seed=9)
    ag = device_agent(algo, S, A, h1, h2, B, k, "MSE", init, precision="fp32", seed=SEED)
    ora = _oracle(algo, S, A, h1, h2, B, k, init, "fp32")
    replay = ReplayMemory(lanes * 64, S, A, device=dev, multi_steps=n_steps, lanes=lanes, dynamics="M", gamma=0.99)
    ring = MultiStepRing(lanes * 64, S, A, lanes, n_steps, "M", 0.99)
    rng = np.random.default_rng(4)
    for t in range(steps):
        s = rng.standard_normal((lanes, S)).astype(np.float32)
        a = rng.uniform(-1, 1, (lanes, A)).astype(np.float32)
        r = rng.uniform(0.5, 1.5, lanes).astype(np.float32)
        s2 = rng.standard_normal((lanes, S)).astype(np.float32)
        d = rng.random(lanes) < (0.3 if t % 7 else 0.9)
        replay.store_exp(s, a, r, s2, d)
        ring.insert(s, a, r, s2, d)
    M = lanes * steps
    assert replay.mem_idx == M
    seen = []

    def rows_of(idx):
        rew, st, ac, s2_, dn, eff = ring.gather(idx)
        seen.append(eff)
        return st, ac, rew, s2_, dn, eff.astype(np.int32)

    lay, n = ol.layout(algo, S, A, h1, h2)
    for call in range(2):
        cntr0 = ag.scalars()["learn_step_cntr"]
        assert cntr0 == call * K
        stats = ag.learn(replay, K).clone()
        ref, _ = _oracle_call(ora, algo, SEED, cntr0, K, M, B, A, rows_of)
        _check_call(ag, ora, algo, "fp32", stats, ref, None, lr_of(algo, lay, n, {}), f"n-step call {call}")
    assert set(np.unique(np.concatenate(seen))) == {1, 2, 3}  # every history length was sampled


def test_train_step_learns_from_restated_samples(dev):
    """The trainer's learn call and its hoisted roles: 1,024 GBM lanes, SAC 256/256
    bf16, K = 2.  Nine steps without updates take the ring past 8,192 rows; the
    first learning step then launches the sampler and draws the next step's index
    sets ahead, the second gathers by those indices inside fwd_rows
    (hoist_counts (1, 1)).  rlmd_train_step inserts the step's rows before it
    learns, so M is the population after the insert (asserted through mem_idx).
    The four updates are rebuilt from the ring's rows as read back; the bf16 oracle
    starts from reference_init(seed = 5) and runs on its own."""
    from rlmd_amd.agent import reference_init
    from rlmd_amd.trainer import VecTrainer

    N, K, cap, seed = 1024, 2, 16384, 5
    tr = VecTrainer("gbm", "A", N, algo="SAC", k_updates=K, replay_capacity=cap, seed=seed, init_seed=seed,
                    warmup_steps=0, smoothing_window=0, precision="bf16", device=dev)
    S, A, B, k = tr.env.state_dim, tr.env.action_dim, tr.batch, tr.topk
    ora = _oracle("SAC", S, A, 256, 256, B, k, reference_init("SAC", S, A, 256, 256, seed=seed), "bf16")
    for _ in range(9):
        tr.step(0)
    assert tr.replay.mem_idx == 9 * N and tr.agent.scalars()["learn_step_cntr"] == 0
    lay, n = ol.layout("SAC", S, A, 256, 256)
    ill = np.zeros(n, dtype=bool)
    for step in range(2):
        cntr0 = tr.agent.scalars()["learn_step_cntr"]
        assert cntr0 == step * K
        tr.step(K)
        M = tr.replay.mem_idx  # the step's own rows are in the ring when it learns
        assert M == (10 + step) * N and M <= cap
        s, a, r, s2, d = read_ring(tr, 0, M)
        rows_of = lambda idx: (s[idx], a[idx], r[idx], s2[idx], d[idx].astype(bool), None)
        ref, ill_step = _oracle_call(ora, "SAC", seed, cntr0, K, M, B, A, rows_of)
        ill |= ill_step
        st = tr.stats[:K].double().cpu().numpy()
        for i, (loss_o, lt_o, lp_o) in enumerate(ref):
            assert_stats_close(st[i], loss_o, lt_o, lp_o, 1e-4, f"train step {step} update {i}", True)
    assert tr.agent.hoist_counts() == (1, 1)
    assert_bf16_state_close(tr.agent, ora, ill, lr_of("SAC", lay, n, {}), "after two learning steps")
