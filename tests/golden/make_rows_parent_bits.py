"""Records tests/golden/rows_parent_bits.npz: what the learner's row kernels
(rows.hip's fwd_rows / qeval_rows) and the update kernels behind them produce,
bit for bit, from the library of the commit BEFORE a change to them.  tests/
test_rows_bits_gpu.py replays record() on the in-tree library and compares.

Run on the GPU with the parent commit's library (tools/ab_build.py, or a build
of the parent checkout):

    RLMD_LIB_PATH=<parent librlmd_amd.so> python tests/golden/make_rows_parent_bits.py

Per case: a ring of FILL seeded transitions, then two rlmd_agent_learn calls of
K = 2 updates each.  Kept: the parameters and the targets after each call (as
SHA-256 digests, plus every STRIDE-th value for a readable failure), both
calls' statistics rows (all 16 columns: loss[11] | logtemp | loss_params[4];
the critic losses are functions of q and the target q, the actor loss of q on
the new action and logp, none of which the ABI exposes themselves) and the
device scalars (log_alpha, the learn counter, the NaN flag).

Cases (name: what the row kernels run):
  sac_c2        SAC 256/256, S 5, A 1, B 512, bf16: the benchmark's instantiation
  sac_fp32      the same in fp32 at B 48 (the f32 MFMA layer 2, three row blocks)
  sac_a2        SAC, two actions (GBM n_gambles 2: the env's S and A), four head slots
  td3_400       TD3 400/300, S 6, A 2, B 200: H1p 416, four bands per wave, the
                streamed K loop, a last row block of 8 rows
  sac_h160      SAC 150/96, B 40: H1p 160 (three threads per column in the
                elementwise map), a last row block of 8 rows
  sac_s12       SAC 256/256, S 12: layer-1 inputs past the 8 preloaded ones
  sac_c2_nosplit  sac_c2 with a CU budget too small for the critics' column
                split (rlmd_agent_set_cu_budget): the unsplit nb0 = 0 path
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "rows_parent_bits.npz")

# name: (algo, S, A, h1, h2, batch, topk, precision, cu_budget); S = A = 0: GBM's with two gambles
CASES = {
    "sac_c2": ("SAC", 5, 1, 256, 256, 512, 256, "bf16", None),
    "sac_fp32": ("SAC", 5, 1, 256, 256, 48, 24, "fp32", None),
    "sac_a2": ("SAC", 0, 0, 256, 256, 512, 256, "bf16", None),
    "td3_400": ("TD3", 6, 2, 400, 300, 200, 100, "bf16", None),
    "sac_h160": ("SAC", 5, 1, 150, 96, 40, 20, "bf16", None),
    "sac_s12": ("SAC", 12, 1, 256, 256, 64, 32, "bf16", None),
    "sac_c2_nosplit": ("SAC", 5, 1, 256, 256, 512, 256, "bf16", 8),
}
FILL = 2048
CALLS = 2
K = 2
STRIDE = 257


def _digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), dtype=np.uint8)


def _case(dev, case):
    import torch

    from rlmd_amd import _abi
    from rlmd_amd.agent import DeviceAgent, ReplayMemory

    algo, S, A, h1, h2, batch, topk, prec, budget = CASES[case]
    if S == 0:
        from rlmd_amd.envs import VecEnv

        env = VecEnv("gbm", "A", 1, 2, seed=7, device=dev)
        S, A = env.state_dim, env.action_dim
        assert A == 2
    ag = DeviceAgent(algo, S, A, h1, h2, batch, topk, precision=prec, seed=11, init_seed=11, device=dev)
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
        p, t = ag.params.cpu().numpy(), ag.target.cpu().numpy()
        out.update({f"call{c}_stats": stats, f"call{c}_params": _digest(p), f"call{c}_target": _digest(t),
                    f"call{c}_params_s": p[::STRIDE].copy(), f"call{c}_target_s": t[::STRIDE].copy()})
    sc = ag.scalars()
    out["scalars"] = np.array([sc["log_alpha"], sc["learn_step_cntr"], sc["nan_flag"]], dtype=np.float64)
    torch.cuda.synchronize()
    return out


def record(dev):
    """{key: array} of everything the fixture holds, from the library now loaded."""
    out = {}
    for case in CASES:
        out.update({f"{case}__{k}": v for k, v in _case(dev, case).items()})
    return out


if __name__ == "__main__":
    import torch

    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec = record(torch.device("cuda:0"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, len(rec), "arrays", os.path.getsize(out), "bytes; library:",
          os.environ.get("RLMD_LIB_PATH", "in-tree"))
