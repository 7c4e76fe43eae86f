"""The learner's row kernels against the parent commit, bit for bit — GPU only.

tests/golden/rows_parent_bits.npz was recorded by tests/golden/
make_rows_parent_bits.py from the library of the commit before fwd_rows /
qeval_rows computed layer 1 on the f32 MFMA and converted to bf16 with the packed
hardware instruction: the same record() on the in-tree library must reproduce
every array's bits.

Per case two rlmd_agent_learn calls of K = 2 updates from a seeded ring; compared:
the parameters and targets after each call, both calls' statistics rows, the
device scalars.  Cases (make_rows_parent_bits.CASES): the benchmark's SAC
256/256 bf16 instantiation at B 512 with the critics' column split on and off,
fp32 at B 48, two actions, TD3 400/300 at B 200 (H1p 416, a last row block of 8
rows), H1p 160 at B 40, a 12-float state.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_GEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_rows_parent_bits.py")


def _gen():
    spec = importlib.util.spec_from_file_location("make_rows_parent_bits", _GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


@pytest.mark.parametrize("case", list(G.CASES))
def test_learn_bits(golden, dev, case):
    """fwd_rows, qeval_rows and the update kernels: two calls of K = 2 updates."""
    ref = golden("rows_parent_bits.npz")
    got = G._case(dev, case)
    pre = case + "__"
    keys = [k for k in ref.files if k.startswith(pre)]
    assert sorted(keys) == sorted(pre + k for k in got), "the fixture's arrays and record()'s differ"
    # the sampled values first: a readable difference before the digests'
    for k in sorted(keys, key=lambda k: (not k.endswith("_s"), k)):
        np.testing.assert_array_equal(_bits(got[k[len(pre):]]), _bits(ref[k]), err_msg=k)
