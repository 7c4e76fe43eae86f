"""The acting kernels and two train steps against the parent commit, bit for bit
— GPU only.

tests/golden/act_parent_bits.npz was recorded by tests/golden/
make_act_parent_bits.py from the library of the commit before the acting body
(rlmd_act_rows.h) drew its policy noise on the sampling wave only and carried
its head slots at compile time, and before the row kernels moved any work: the
same record() on the in-tree library must reproduce every array's bits.

Shapes: 65 lanes (a full 64-row block plus a one-row block) and one lane; SAC
with one and two actions (GBM, n_gambles 1 / 2: the half- and full-width
epilogues) and TD3 (Dice_SH, two actions, 400/300); the acting kernel alone in
mode 0 with drawn noise, mode 0 with injected noise and mode 1; the training
loop's policy steps with the acting + env fusion on and off (actions, ring rows,
next observations); parameters and targets after two train steps at 65 lanes,
K = 2.  65,600 lanes (the four-workgroups-per-CU instantiations, as digests).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_act_parent_bits.py")


def _gen():
    spec = importlib.util.spec_from_file_location("make_act_parent_bits", _GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(golden, got, prefix):
    ref = golden("act_parent_bits.npz")
    keys = [k for k in ref.files if k.startswith(prefix)]
    assert sorted(keys) == sorted(prefix + k for k in got), "the fixture's arrays and record()'s differ"
    for k in keys:
        np.testing.assert_array_equal(_bits(got[k[len(prefix):]]), _bits(ref[k]), err_msg=k)


@pytest.mark.parametrize("n", G.LANES)
@pytest.mark.parametrize("case", list(G.CASES))
def test_acting_kernel_bits(golden, dev, case, n):
    """fused_act_kernel: drawn noise, injected noise, deterministic."""
    got = G._acting(dev, case, n)
    assert not np.array_equal(got["act_m0"], got["act_m1"]) and not np.array_equal(got["act_m0"], got["act_eps"])
    _same(golden, {k[4:]: v for k, v in got.items()}, f"{case}__n{n}__act_")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", G.LANES)
@pytest.mark.parametrize("case", list(G.CASES))
def test_policy_step_bits(golden, dev, case, n, fused):
    """act_env_kernel (fused 1) / fused_act_kernel + env_train_kernel (fused 0): ring rows and next observations."""
    _same(golden, G._steps(dev, case, n, fused), f"{case}__n{n}__fused{fused}__")


@pytest.mark.parametrize("case", list(G.CASES))
def test_train_step_bits(golden, dev, case):
    """Two train steps at K = 2 (fwd_rows, qeval_rows, the update kernels): parameters and targets."""
    _same(golden, G._train(dev, case, 65), f"{case}__n65__train__")


def test_four_per_cu_bits(golden, dev):
    """65,600 lanes: the parked four-workgroups-per-CU instantiations of both acting kernels."""
    pre = f"sac_a1__n{G.BIG}__"
    _same(golden, {k[4:]: G._digest(v) for k, v in G._acting(dev, "sac_a1", G.BIG).items()}, pre + "act_")
    for fused in (1, 0):
        _same(golden, {k: G._digest(v) for k, v in G._steps(dev, "sac_a1", G.BIG, fused).items()},
              f"{pre}fused{fused}__")
