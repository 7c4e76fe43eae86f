"""The learner's dispatch branches against the oracle, one case per branch — GPU only.

librlmd_amd picks its update kernels by shape (learn.hip rlmd_agent_create /
learn_body, rows.hip launch_prec, update.hip critic_update_launch /
actor_update_launch).  With X = S + A, H1p / H2p the widths padded to 32 and
n_cu the CU budget:
  path    B <= 512 and X <= 8: the critic step is one launch ("fused"), else the
          launch chain (cbwd_rows + weight-gradient GEMM + Adam); the actor step
          is one launch only if also A <= 2, else abwd_rows + GEMM + Adam;
  WIDE    B <= 256: the fused steps' 32 x 64 tile form, else 32 x 32;
  split   fsplit (fwd_rows) = 2 iff fused critic, H2p % 64 == 0 and
          2 ceil(B / 16) ny <= n_cu (ny = 5 forward jobs on an actor step, 4
          without); qsplit (qeval_rows) = 2 iff fused actor, H2p % 64 == 0 and
          ceil(B / 16) (2 nq + heads) <= n_cu (nq = 2 critics / heads = 2 A for
          SAC, 1 / A for TD3);
  NBW     max(H1p, H2p) <= 128: 1, <= 256: 2, else 4 column blocks per wave;
  layer 1 an fc1 input up to W1P = 8 wide sits in registers, a wider one runs
          the tail loop; the batched LDS reads need a row pitch that is a
          multiple of 4 (the pitch is max(X, 8) for actor and critics alike);
  loss    B > 512: actor_loss_kernel instead of abwd_rows' loss workgroup.
Every case below names the values it is there for.  Each runs 4 updates (6
where update intervals are involved): fp32 against the autograd oracle, bf16
against the bf16 oracle from the device's state with O(1) state rows, under
the bounds of tests/test_learn_gpu.py (its docstring, DESIGN.md "parity
tolerances"): statistics rtol 2e-4 (fp32) / 1e-4 (bf16), atol 1e-6; at least
99.9 % of the parameters within 2e-6; the worst (bf16: worst well-conditioned)
within 10 % of the entry's learning rate, 20 % at B = 513 as at B = 1024.  Every
net here has at least 14,000 parameters, so 99.9 % leaves 14 entries or more.
"""
import pytest

from tests.test_learn_gpu import bf16_vs_oracle, test_full_size_fp32_matches_oracle as fp32_vs_oracle

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16"]


def _id(v):
    """SAC-5-3-64x64-B48 for a case tuple; other parameters keep pytest's ids."""
    if isinstance(v, tuple):
        algo, S, A, h1, h2, B, _ = v
        return f"{algo}-{S}-{A}-{h1}x{h2}-B{B}"
    return None


def run(dev, precision, case, loss="MSE", path="fused", actor_path=None, max_lr_frac=0.1, **kw):
    """One case in one precision; path / actor_path name the bf16 oracle's form
    (the fp32 oracle is autograd: one form for every path)."""
    if precision == "fp32":
        fp32_vs_oracle(dev, *case, loss, max_lr_frac=max_lr_frac, check_logtemp=True, **kw)
    else:
        bf16_vs_oracle(*case, loss, path=path, actor_path=actor_path, max_lr_frac=max_lr_frac, **kw)


# ---- fused critic step, launch-chain actor step (A > 2, X <= 8, B <= 512)
FUSED_CHAIN = [("SAC", 5, 3, 64, 64, 48, 24), ("TD3", 4, 4, 64, 64, 272, 136)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case,loss", [(FUSED_CHAIN[0], "MSE"), (FUSED_CHAIN[1], "MSE"), (FUSED_CHAIN[0], "TCAU")], ids=_id)
def test_fused_critic_chain_actor(dev, precision, case, loss):
    """The C investors' and Dice_SH B / C's pairing: X = 8 <= 8 and B <= 512 keep
    critic_update_kernel, A = 3 / 4 > 2 sends the actor step through qeval_rows
    (no dq/da, no head jobs) + abwd_rows (its A > 2 branches: the save rows and
    head weights read in loops) + the GEMM + adam_kernel.
    SAC 5/3 64/64 B 48: WIDE (B <= 256), H2p 64, 2 * 3 * 5 = 30 <= 256: fsplit 2,
    qsplit 1 (no fused actor), NBW 1; the actor's fc1 (5 wide) in registers.
    TD3 4/4 64/64 B 272: the 32 x 32 form, 2 * 17 * 5 = 170 <= 256: fsplit 2; 17
    row blocks, the last wave slices of the tiles empty.
    bf16: the oracle's path="fused" critic half with actor_path="chain"."""
    run(dev, precision, case, loss, path="fused", actor_path="chain")


# ---- the launch chain by input width (X > 8)
CHAIN_WIDTH = [("SAC", 8, 1, 64, 64, 48, 24), ("SAC", 16, 4, 64, 64, 272, 136)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case,loss", [(CHAIN_WIDTH[0], "MSE"), (CHAIN_WIDTH[1], "MSE"), (CHAIN_WIDTH[1], "TCAU")], ids=_id)
def test_chain_by_input_width(dev, precision, case, loss):
    """X > 8 takes the launch chain for both steps without any switch set.
    SAC 8/1: X = 9, row pitch 9 (no multiple of 4): the actor's fc1 is exactly
    W1P = 8 wide (registers only, the unbatched loop), the critics' 9 wide (a tail
    of one element).  SAC 16/4: X = 20, the actor's tail 8 elements, the critics'
    12; A = 4 in abwd_rows; B = 272 = 17 row blocks.  No splits (not fused)."""
    run(dev, precision, case, loss, path="chain")


# ---- hidden widths
WIDTHS = [("SAC", 5, 1, 64, 96, 48, 24), ("TD3", 6, 2, 96, 160, 272, 136), ("SAC", 6, 2, 64, 128, 272, 136),
          ("SAC", 5, 1, 512, 512, 32, 16)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case,loss", [(c, "MSE") for c in WIDTHS] + [(WIDTHS[1], "TCAU")], ids=_id)
def test_hidden_widths(dev, precision, case, loss):
    """All fused (X <= 8, A <= 2, B <= 512), h1 < h2 in the first three.
    64/96 B 48: H2p = 96, 96 % 64 != 0: critic_update_kernel<WIDE = true, SPLIT =
    false> (fsplit = qsplit = 1), ti = 3 fc2 tile rows by tj = 1 tile column (64
    wide), NBW 1 from H2p = max(H1p, H2p).
    96/160 B 272: H2p = 160 (ti = 5, an odd count; 160 % 64 != 0: no split), H1p =
    96 (tj = 3), the 32 x 32 form, NBW 2 from H2p alone; 160 columns over 512
    threads give the row kernels' elementwise map 6 rows per thread, the one
    padded width whose row count is no power of two.
    64/128 B 272: H2p = 128, 2 * 17 * 5 = 170 and 17 * (2 * 2 + 4) = 136 <= 256:
    fsplit = qsplit = 2 with h1 < h2, NBW 1.
    512/512 B 32: the documented maximum (launch_rows' LDS budget check), NBW 4 and
    the streaming K loop, WIDE, both splits on."""
    run(dev, precision, case, loss)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_first_width_of_160(dev, monkeypatch, precision, fused):
    """SAC 6/2 150/96 B 272: H1p = 160 on the FIRST hidden layer, the mirror of
    96/160 above.  rows.hip elem_map spreads a [16 x Hp] block over 512 threads as
    512 / Hp threads per column; at Hp = 160 that is 3, and 16 rows over 3 threads
    were 6, 6 and 4 rows each, where layer 1's packed stores (the [h1 > 0] mask
    words of m1_index, the row-packed h1 of store_rp_rows) take 1, 2, 4, 8 or 16
    rows from a multiple of that count: mask bytes landed in the neighbouring
    column's word and most of the packed h1 was never written.  Every other padded
    width up to 512 gives a power of two.  elem_map now rounds the count up to one
    (two threads of 8 rows at 160).  Both paths read those stores: the fused steps
    the packed h1 (dW2) and the masks (the policy's head bases), the launch chain
    the masks (cbwd_rows / abwd_rows dh1).  NBW 2, H2p 96: no split."""
    if not fused:
        monkeypatch.setenv("RLMD_NO_FUSED_UPDATE", "1")
    run(dev, precision, ("SAC", 6, 2, 150, 96, 272, 136), path="fused" if fused else "chain")


# ---- batch boundaries
def _batch_case(algo, B):
    S, A = (5, 1) if algo == "SAC" else (6, 2)
    k = {2: 2, 16: 16, 513: 256}.get(B, B // 2)
    return (algo, S, A, 64, 64, B, k)


@pytest.mark.parametrize("algo", ["SAC", "TD3"])
@pytest.mark.parametrize("B,precision,loss", [(B, "fp32", "MSE") for B in (2, 16, 17, 256, 257, 513)] +
                         [(B, "bf16", "MSE") for B in (256, 257, 513)] + [(257, "fp32", "TCAU")])
def test_batch_boundaries(dev, algo, B, precision, loss):
    """SAC 5/1 and TD3 6/2 at 64/64 (H2p 64: the splits fit at every B <= 512).
    B = 2 (k = 2): the ABI minimum, 14 of the one row block's 16 rows padding and
    no top-k (k = B).  B = 16 (k = 16): one full block, k = B.  B = 17 (k = 8):
    one block plus one row.  B = 256 | 257 (k = 128): the last WIDE batch and the
    first of the 32 x 32 form.  B = 513 (k = 256): the first batch past the fused
    steps: the launch chain with critic_loss_kernel<1024> and actor_loss_kernel,
    33 row blocks; its sums are as long as B = 512's, the bound 20 % of lr as
    for B = 1024."""
    run(dev, precision, _batch_case(algo, B), loss, path="chain" if B > 512 else "fused",
        max_lr_frac=0.2 if B > 512 else 0.1)


# ---- the CU budget
BUDGET = [("SAC", 5, 1, 256, 256, 512, 256), ("TD3", 6, 2, 400, 300, 200, 100), ("SAC", 5, 1, 48, 40, 272, 136)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case,loss,budget", [(c, "MSE", 64) for c in BUDGET] + [(BUDGET[0], "TCAU", 64),
                                                                                  (BUDGET[0], "MSE", 1)],
                         ids=_id)
def test_cu_budget_turns_splits_off(dev, precision, case, loss, budget):
    """rlmd_agent_set_cu_budget(64) before the first update: a four-seed share of
    256 CUs (SeedGroup, bench.py --full); 1 is the floor.  Against the same oracle
    as the full device.
    256/256 B 512: qsplit 32 * (2 * 2 + 2) = 192 <= 256 is 2 on the full device and
    1 under 64 (fsplit 2 * 32 * 5 = 320 is off either way): the unsplit fused actor
    step.  400/300 B 200: fsplit 2 * 13 * 5 = 130 and qsplit 13 * (2 + 2) = 52 <= 256
    on, 130 > 64 off but qsplit 52 <= 64 still on; under 1 both off.  48/40 B 272:
    fsplit 170, qsplit 17 * 6 = 102: both off under 64."""
    run(dev, precision, case, loss, cu_budget=budget)


# ---- configuration that reaches the kernels
CONFIG = {
    "no_topk": dict(actor_topk=False),
    "intervals": dict(temp_update_interval=2, actor_update_interval=2),
    "scalars": dict(gamma=0.9, tau=0.05, lr_actor=1e-3, lr_critic=5e-4, lr_temp=1e-3, reward_scale=2.0,
                    max_action=0.8, initial_logtemp=-1.0, cauchy_scale=0.5),
}
# the reference's TD3 has no temperature and no reward scale
TD3_SKIPS = ("lr_temp", "reward_scale", "initial_logtemp")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("algo,name", [("SAC", "no_topk"), ("TD3", "no_topk"), ("SAC", "intervals"),
                                       ("SAC", "scalars"), ("TD3", "scalars")])
def test_configuration_reaches_kernels(dev, monkeypatch, precision, fused, algo, name):
    """Settings DeviceAgent plumbs into AgentCfg, at SAC 5/1 / TD3 6/2 64/64 B 48
    k 24 (WIDE, both splits on), through the fused steps and through the launch
    chain (RLMD_NO_FUSED_UPDATE=1).
    no_topk: actor_topk = False (actor_percentile == 100): the actor loss over all
    B rows, no ranking.
    intervals: SAC with actor and temperature steps every second update, 6
    updates: the critic step's own statistics workgroups on updates 1, 3, 5, the
    parity slots of LearnState (log alpha, Cauchy scales) carried over updates
    without a temperature step, Adam's bias corrections at cnt / interval.
    scalars: gamma, tau, the three learning rates, reward_scale, max_action,
    initial_logtemp and cauchy_scale away from their defaults with the CAU loss
    (whose scale starts at cauchy_scale); lr in the bound is the entry's own
    (actor 1e-3, critics 5e-4)."""
    if not fused:
        monkeypatch.setenv("RLMD_NO_FUSED_UPDATE", "1")
    kw = dict(CONFIG[name])
    if algo == "TD3":
        for key in TD3_SKIPS:
            kw.pop(key, None)
    case = (algo, 5, 1, 64, 64, 48, 24) if algo == "SAC" else (algo, 6, 2, 64, 64, 48, 24)
    run(dev, precision, case, "CAU" if name == "scalars" else "MSE", path="fused" if fused else "chain",
        steps=6 if name == "intervals" else 4, agent_kw=kw)
