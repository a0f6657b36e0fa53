"""GPU: every kernel of csrc/loss.hip gives the BITS recorded in tests/golden/g16_loss_bits.npz.

The kernels are deterministic (fp32 terms, fp64 adds in a fixed order, no floating-point atomics),
so their output is a function of the input and the add order alone; the fixture holds what the
commit before the shared sum-count hand-off and table fold computed on the MI355X
(tests/golden/gen_golden_loss_bits.py).  Inputs come from the integer formula of
tests/loss_bits_cases.py, where each case's reason is written down; the comparison is torch.equal on
integer views, so -0.0 / +0.0 and every NaN payload count too.

A bit that differs means a reordered add or a changed contraction in the kernels: the fixture is
not re-recorded for it.
"""
import os

import numpy as np
import pytest
import torch

import loss_bits_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with np.load(os.path.join(golden_dir, "g16_loss_bits.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _bits(v):
    v = v.detach().cpu().contiguous()
    return v.view(torch.int32 if v.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("group", list(cases.GROUPS))
def test_bits_of_the_parent(group, recorded):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dstagnn_drought_amd import _lib
    got = cases.GROUPS[group](_lib.load(), torch.device("cuda:0"))
    want = {k: v for k, v in recorded.items() if k.startswith(cases.PREFIX[group])}
    assert sorted(got) == sorted(want)
    bad = []
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), k
        if not torch.equal(_bits(g), _bits(w)):
            bad.append(f"{k}: {int((_bits(g) != _bits(w)).sum())} of {w.numel()} differ")
    assert not bad, "\n".join(bad)


def test_grid_cap_gradient(recorded):
    """n = 1025 tiles of mae: dy against sign(y - t) * scale, the scale from the RECORDED stat (the
    product is exact, so the 16 MB array is not in the fixture)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dstagnn_drought_amd import _lib
    dy, want = cases.grid_cap_dy(_lib.load(), torch.device("cuda:0"), recorded["cap/mae/stat"])
    assert torch.equal(dy.view(torch.int32), want.view(torch.int32))
