"""Records tests/golden/act_parent_bits.npz: what the acting kernels (act.hip's
fused_act_kernel, env.hip's act_env_kernel) and two train steps produce, bit for
bit, from the library of the commit BEFORE a change to them.  tests/
test_act_bits_gpu.py replays record() on the in-tree library and compares.

Run on the GPU with the parent commit's library (tools/ab_build.py, or a build
of the parent checkout):

    RLMD_LIB_PATH=<parent librlmd_amd.so> python tests/golden/make_act_parent_bits.py

Cases: SAC with one and two actions (GBM, n_gambles 1 / 2) and TD3 (Dice_SH,
two actions), at 65 lanes (a full 64-row block plus a one-row block) and at one
lane.  Per case: the acting kernel alone in mode 0 with drawn noise, mode 0
with injected noise and mode 1; three policy steps of the training loop with the
acting + env fusion on and off (ring rows and next observations); at 65 lanes
the parameters and targets after two train steps at K = 2 (as SHA-256 digests).
At 65,600 lanes (1,025 blocks: the four-workgroups-per-CU instantiations with
their per-row values parked in LDS) the same acting calls and steps, as digests.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "act_parent_bits.npz")

# name: (env, investor, n_gambles, algo)
CASES = {"sac_a1": ("gbm", "A", 1, "SAC"), "sac_a2": ("gbm", "A", 2, "SAC"), "td3_a2": ("dice_sh", "A", 1, "TD3")}
LANES = (65, 1)
BIG = 65600  # SAC, one action: the benchmark's instantiation
STEPS = 3
FILL = 8  # policy steps before the two train steps: 520 rows > the 512-row batch


def _trainer(dev, case, n, steps, k=0):
    from rlmd_amd.trainer import VecTrainer

    env, inv, ng, algo = CASES[case]
    return VecTrainer(env=env, investor=inv, n_lanes=n, n_gambles=ng, algo=algo, k_updates=k, seed=7, init_seed=7,
                      warmup_steps=0, smoothing_window=0, replay_capacity=n * steps, precision="bf16", device=dev)


def _read_ring(tr, start, n):
    import torch

    from rlmd_amd import _abi

    S, A, dev = tr.replay.S, tr.replay.A, tr.device
    s, a, r = torch.empty(n, S, device=dev), torch.empty(n, A, device=dev), torch.empty(n, device=dev)
    s2, d = torch.empty(n, S, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    P = _abi.ptr
    _abi.check(_abi.lib().rlmd_replay_read(tr.replay.h, start, n, P(s), P(a), P(r), P(s2), P(d), _abi.stream_ptr()))
    return {k: v.cpu().numpy() for k, v in zip(("s", "a", "r", "s2", "d"), (s, a, r, s2, d))}


def _acting(dev, case, n):
    """The acting kernel alone on the reset observations: drawn noise, injected noise, deterministic."""
    import torch

    tr = _trainer(dev, case, n, STEPS)
    A = tr.env.action_dim
    eps = torch.from_numpy(np.random.default_rng(123).standard_normal((n, A)).astype(np.float32))
    obs = tr.obs.clone()
    out = {"act_m0": tr.agent.act(obs, mode=0, noise_ctr=3), "act_eps": tr.agent.act(obs, mode=0, noise_ctr=3, eps=eps),
           "act_m1": tr.agent.act(obs, mode=1)}
    return {k: v.cpu().numpy() for k, v in out.items()}


def _steps(dev, case, n, fused):
    tr = _trainer(dev, case, n, STEPS)
    tr.set_fused(fused)
    for _ in range(STEPS):
        tr.step()
        assert tr.last_fused() == bool(fused)
    out = {"ring_" + k: v for k, v in _read_ring(tr, 0, n * STEPS).items()}
    out["obs"] = tr.obs.cpu().numpy()
    return out


def _train(dev, case, n):
    tr = _trainer(dev, case, n, FILL + 2, k=2)
    for _ in range(FILL):
        tr.step(k_updates=0)
    for _ in range(2):
        tr.step(k_updates=2)
    assert np.all(np.isfinite(tr.stats.cpu().numpy()[:, 0])), "the train steps did not learn"
    # a few hundred thousand floats per net set: kept as digests
    return {"params": _digest(tr.agent.params.cpu().numpy()), "target": _digest(tr.agent.target.cpu().numpy())}


def _digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), dtype=np.uint8)


def record(dev):
    """{key: array} of everything the fixture holds, from the library now loaded."""
    out = {}
    for case in CASES:
        for n in LANES:
            pre = f"{case}__n{n}__"
            out.update({pre + k: v for k, v in _acting(dev, case, n).items()})
            for fused in (1, 0):
                out.update({f"{pre}fused{fused}__{k}": v for k, v in _steps(dev, case, n, fused).items()})
        out.update({f"{case}__n65__train__{k}": v for k, v in _train(dev, case, 65).items()})
    pre = f"sac_a1__n{BIG}__"
    out.update({pre + k: _digest(v) for k, v in _acting(dev, "sac_a1", BIG).items()})
    for fused in (1, 0):
        out.update({f"{pre}fused{fused}__{k}": _digest(v) for k, v in _steps(dev, "sac_a1", BIG, fused).items()})
    return out


if __name__ == "__main__":
    import torch

    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec = record(torch.device("cuda:0"))
    np.savez_compressed(out, **rec)
    print("wrote", out, len(rec), "arrays", os.path.getsize(out), "bytes; library:",
          os.environ.get("RLMD_LIB_PATH", "in-tree"))
