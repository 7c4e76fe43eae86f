"""The replay sample hoisted off the training step's chain (learn.hip
agent_learn_k, RLMD_SAMPLE_HOIST): the step's last learner launch draws the NEXT
step's K index sets (the draw is a function of seed, counter, ring population
and batch only — replay.hip / rlmd_replay_dev.h), and a step whose key matches
gathers by index inside update 0's fwd_rows launch instead of launching
replay_sample_kernel.  Only where the work runs changes: every case trains twice,
RLMD_SAMPLE_HOIST=0 against 1 (read at agent creation), and requires bit-identical
parameters, targets, the K statistics rows of every step (without the NaN
placeholder slots bench.py's last_step_outputs leaves out), final observations
and ring contents.  The sampled indices themselves (kb_idx)
are not reachable from Python; every later kernel of an update reads the rows
gathered through them, so a wrong index shows in the statistics of that step.

rlmd_agent_hoist_counts says which path the calls took.  Condition of the first
case: at least 12 of its 24 learn calls must be hoisted (the ring passes 8,192
rows, the sort path's bound, after step 8).
Reference: tools/replay.py:334-376 (sample_exp), algos/algo_sac.py:300-615."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LANES = 1024
CAP = 16 * LANES  # 16,384 > 8,192: the hash path once the ring holds more than 8 steps


def _trainer(dev, algo="SAC", env="gbm", k=3, cap=CAP, ms=1):
    from rlmd_amd.trainer import VecTrainer

    return VecTrainer(env, "A", n_lanes=LANES, algo=algo, k_updates=k, replay_capacity=cap, seed=5, init_seed=5,
                      warmup_steps=2, smoothing_window=4, precision="bf16", multi_steps=ms, device=dev)


def _cols(tr):
    return [c for c in range(16) if c not in ((6, 7) if tr.agent.algo == "SAC" else (6, 7, 10, 11))]


def _step(tr, stats, k=None):
    tr.step(k)
    stats.append(tr.stats[:tr.cfg.k_updates][:, _cols(tr)].cpu().numpy().copy())


def _result(tr, stats):
    torch.cuda.synchronize()
    rows = np.arange(min(tr.replay.mem_idx, tr.replay.capacity))
    ring = [x.cpu().numpy().copy() for x in tr.replay.gather(rows)]
    out = {"params": tr.agent.params.cpu().numpy().copy(), "target_params": tr.agent.target.cpu().numpy().copy(),
           "obs": tr.obs.cpu().numpy().copy()}
    for i, s in enumerate(stats):
        out[f"learn_stats[{i}]"] = s
    for name, x in zip(("s", "a", "r", "s2", "done", "eff"), ring):
        out["ring." + name] = x
    return out


def _both(monkeypatch, run):
    """run() -> (result dict, (hoisted, fallen back)) with the switch off, then on."""
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("RLMD_SAMPLE_HOIST", sw)
        res[sw] = run()
    off, on = res["0"], res["1"]
    assert off[0].keys() == on[0].keys()
    for name in off[0]:
        np.testing.assert_array_equal(on[0][name], off[0][name], err_msg=name)
    assert np.isfinite(on[0]["params"]).all()
    return off[1], on[1], on[0]


def _plain(dev, steps, **kw):
    def run():
        tr, stats = _trainer(dev, **kw), []
        for _ in range(steps):
            _step(tr, stats)
        return _result(tr, stats), tr.agent.hoist_counts()

    return run


def test_ring_growth_fill_and_wrap(dev, monkeypatch):
    # M grows 1,024 a step, reaches the capacity at step 16, then wraps; steps 1-8
    # (M <= 8,192) launch the sampler, step 8 draws for step 9
    off, on, res = _both(monkeypatch, _plain(dev, 24))
    assert off == (0, 24)
    assert on[0] + on[1] == 24
    assert on[0] >= 12, f"hoisted {on[0]} of 24 calls"
    assert on == (16, 8)
    assert np.isfinite(res["learn_stats[23]"][:, :6]).all()  # real updates ran


def test_k_changing_between_calls(dev, monkeypatch):
    ks = [3] * 10 + [1, 3, 8, 8, 3, 3]

    def run():
        tr, stats = _trainer(dev, k=max(ks)), []  # the statistics tensor holds the largest K
        for k in ks:
            _step(tr, stats, k)
        return _result(tr, stats), tr.agent.hoist_counts()

    off, on, _ = _both(monkeypatch, run)
    assert off == (0, len(ks))
    # hoisted: steps 9 and 10 (K = 3 again, M > 8,192), the second K = 8, the last K = 3;
    # every call after a change of K launches the sampler
    assert on == (4, len(ks) - 4)


def test_host_write_and_direct_learn_fall_back(dev, monkeypatch):
    def run():
        tr, stats, seen = _trainer(dev), [], []
        for _ in range(11):
            _step(tr, stats)
        seen.append(tr.agent.hoist_counts())  # steps 9-11 hoisted
        tr.agent.params.add_(0.0)  # a host write (same values): the version counter moves
        _step(tr, stats)
        seen.append(tr.agent.hoist_counts())
        _step(tr, stats)
        seen.append(tr.agent.hoist_counts())
        tr.agent.learn(tr.replay, k=3)  # outside the trainer: counters move, nothing drawn ahead
        seen.append(tr.agent.hoist_counts())
        _step(tr, stats)
        seen.append(tr.agent.hoist_counts())
        _step(tr, stats)
        seen.append(tr.agent.hoist_counts())
        out = _result(tr, stats)
        out["direct_stats"] = tr.agent.stats[:3][:, _cols(tr)].cpu().numpy().copy()
        return out, seen

    off, on, _ = _both(monkeypatch, run)
    assert [h for h, _ in off] == [0] * 6
    # after the write: sampler; next step: hoisted again; direct learn: sampler; the
    # step after it (nothing was drawn for it): sampler; then hoisted again
    assert on == [(3, 8), (3, 9), (4, 9), (4, 10), (4, 11), (5, 11)]


def test_sort_path_ring_is_not_hoisted(dev, monkeypatch):
    off, on, _ = _both(monkeypatch, _plain(dev, 8, cap=4096))  # M <= 8,192 always
    assert off == (0, 8) and on == (0, 8)


@pytest.mark.parametrize("k", [4, 3])
def test_td3_pairing_and_last_launch(dev, monkeypatch, k):
    # TD3 400/300, B = 200 / k = 100 (one gather part per mini-batch, target pairing on).
    # K = 4: every call ends on an actor step (actor_update draws); K = 3: the last
    # launch alternates between critic_update and actor_update
    off, on, res = _both(monkeypatch, _plain(dev, 14, algo="TD3", env="dice_sh", k=k))
    assert off == (0, 14)
    assert on == (6, 8)  # steps 9-14
    assert np.isfinite(res["learn_stats[13]"][:, :6]).all()


def test_multistep_ring_falls_back(dev, monkeypatch):
    # n = 3 histories (gather_row) are not covered by the gather inside fwd_rows
    off, on, _ = _both(monkeypatch, _plain(dev, 12, ms=3))
    assert off == (0, 12) and on == (0, 12)
