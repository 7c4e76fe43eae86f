"""The row kernels' exact-shape form against their run-time form, bit for bit — GPU only.

At bf16 hidden widths 256 / 256 fwd_rows and qeval_rows run instantiations whose
layer-2 MFMA loops (rows.hip frag_load / frag_mfma, the epilogues' band loops)
have their live bands per wave and their K-step count at compile time
(rows_exact: unsplit, and under the critics' column split).  Only control flow
differs: every accumulator still takes its K-steps in ascending order from
zero.  RLMD_ROWS_EXACT=0 (read at agent creation, as RLMD_SAMPLE_HOIST is: the
sides run in one process, each agent created under its setting) sends every shape
down the run-time form.

Per case: a ring of FILL seeded rows, two rlmd_agent_learn calls of K = 2, once
per setting; the parameters, the targets, both calls' statistics rows and the
device scalars must agree bit for bit.  rlmd_agent_rows_exact_counts says which
form the launches took: the 256 / 256 cases the exact one, the 224-wide ones
(14 bands; 7 K-steps) the run-time one under either setting.  The last case is
the staging-by-index instantiation (GATHER): trainer steps whose sample was
drawn ahead.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILL = 256
CALLS = 2
K = 2

# name: (h1, h2, batch, cu_budget, takes the exact form)
CASES = {
    "split": (256, 256, 48, None, True),     # the critics' column split on (both kernels)
    "nosplit": (256, 256, 48, 8, True),      # a CU budget the doubled grids do not fit
    "last_block_8": (256, 256, 40, None, True),
    "h2_224": (256, 224, 48, None, False),   # 14 output bands: waves 6, 7 own one band
    "h1_224": (224, 256, 48, None, False),   # 7 K-steps of layer 2
}


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _equal(on, off):
    assert on.keys() == off.keys()
    for name in on:
        np.testing.assert_array_equal(_bits(on[name]), _bits(off[name]), err_msg=name)
    assert np.isfinite(on["params"]).all()


def _learn(dev, case):
    from rlmd_amd import _abi
    from rlmd_amd.agent import DeviceAgent, ReplayMemory

    h1, h2, batch, budget, _ = CASES[case]
    S, A = 5, 1
    ag = DeviceAgent("SAC", S, A, h1, h2, batch, batch // 2, precision="bf16", seed=11, init_seed=11, device=dev)
    if budget is not None:
        _abi.check(_abi.lib().rlmd_agent_set_cu_budget(ag.h, int(budget)))
    rng = np.random.default_rng(2024)
    rb = ReplayMemory(2 * FILL, S, A, device=dev)
    rb.store_exp(rng.standard_normal((FILL, S)).astype(np.float32),
                 rng.uniform(-0.99, 0.99, (FILL, A)).astype(np.float32),
                 (0.1 * rng.standard_normal(FILL)).astype(np.float32),
                 rng.standard_normal((FILL, S)).astype(np.float32), (rng.random(FILL) < 0.05).astype(np.uint8))
    out = {}
    for c in range(CALLS):
        stats = ag.learn(rb, k=K).cpu().numpy().copy()
        assert np.all(np.isfinite(stats[:, 0])), "the updates did not learn"
        out[f"call{c}_stats"] = stats
        out[f"call{c}_params"] = ag.params.cpu().numpy().copy()
        out[f"call{c}_target"] = ag.target.cpu().numpy().copy()
    sc = ag.scalars()
    out["scalars"] = np.array([sc["log_alpha"], sc["learn_step_cntr"], sc["nan_flag"]], dtype=np.float64)
    out["params"] = out[f"call{CALLS - 1}_params"]
    torch.cuda.synchronize()
    return out, ag.rows_exact_counts()


def _both(monkeypatch, run):
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("RLMD_ROWS_EXACT", sw)
        res[sw] = run()
    _equal(res["1"][0], res["0"][0])
    return res["0"][1], res["1"][1]


@pytest.mark.parametrize("case", list(CASES))
def test_learn_bits(dev, monkeypatch, case):
    off, on = _both(monkeypatch, lambda: _learn(dev, case))
    print(case, "launches (exact, run-time): switch off", off, "on", on)
    # SAC steps the actor with every update: one fwd_rows and one qeval_rows launch each
    assert off == (0, 2 * CALLS * K)
    assert on == ((2 * CALLS * K, 0) if CASES[case][4] else (0, 2 * CALLS * K))


def test_gather_bits(dev, monkeypatch):
    """fwd_rows staging by index: 4,096 lanes a step, so the ring passes the sort
    path's 8,192 rows with step 3 — step 2's last launch draws for it."""
    from rlmd_amd.trainer import VecTrainer

    def run():
        tr = VecTrainer("gbm", "A", n_lanes=4096, algo="SAC", k_updates=K, replay_capacity=16384, seed=5, init_seed=5,
                        warmup_steps=2, smoothing_window=4, precision="bf16", batch=48, topk=24, device=dev)
        out = {}
        for i in range(4):
            tr.step()
            out[f"stats[{i}]"] = tr.stats[:K].cpu().numpy().copy()
        torch.cuda.synchronize()
        out["params"] = tr.agent.params.cpu().numpy().copy()
        out["target"] = tr.agent.target.cpu().numpy().copy()
        out["obs"] = tr.obs.cpu().numpy().copy()
        sc = tr.agent.scalars()
        out["scalars"] = np.array([sc["log_alpha"], sc["learn_step_cntr"], sc["nan_flag"]], dtype=np.float64)
        return out, (tr.agent.rows_exact_counts(), tr.agent.hoist_counts())

    (off, hoff), (on, hon) = _both(monkeypatch, run)
    print("gather: launches", off, on, "hoisted calls", hoff, hon)
    assert hoff == hon and hon[0] >= 2, "two consecutive steps gather by index under both settings"
    assert off == (0, 2 * 4 * K) and on == (2 * 4 * K, 0)
