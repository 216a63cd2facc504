"""The double-where head reference of tests/eq_head_ref.py (the second-order oracle of the per-channel zero-norm
cases in tests/test_gpu_eq_head_widths.py) on the CPU: it IS kernels.eq_head_composite in both derivative orders
where no single channel's norm vanishes, and it stays finite where one does -- where the composite's double
differentiation, like the reference's torch.norm, is NaN."""
import pytest
import torch

import eq_head_ref as R
from test_eq_head import _head
from torchmdnet import kernels

F64 = torch.float64


def _params(H, zero_channels=False):
    head = _head(H, F64)
    if zero_channels:
        R.zero_channels(head)
    return kernels.eq_head_params(head.output_network)


@pytest.mark.parametrize("H", [4, 20, 24])
def test_double_where_reference_is_the_composite(H):
    ps = _params(H)
    x, vec, gy, cx, cv = R.inputs(5, H, F64, zero=2)  # the zero-vector atom: masked by both in the same way
    y0, f0, s0 = R.reference(ps, x, vec, gy, cx, cv)
    y1, f1, s1 = R.reference(ps, x, vec, gy, cx, cv, composite=R.composite_dw)
    assert torch.allclose(y1, y0, rtol=1e-12, atol=1e-12)
    for name, a, b in zip(R.FIRST + R.SECOND, f1 + list(s1), f0 + list(s0)):
        if b is None:
            assert a is None, name
            continue
        assert torch.isfinite(a).all(), name
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("H", [20, 24])
def test_double_where_reference_is_finite_at_a_zero_channel(H):
    ps = _params(H, zero_channels=True)
    x, vec, gy, cx, cv = R.inputs(5, H, F64, zero=2)
    y0, f0, s0 = R.reference(ps, x, vec, gy, cx, cv)
    y1, f1, s1 = R.reference(ps, x, vec, gy, cx, cv, composite=R.composite_dw)
    # first order: the composite is finite there and the two agree
    assert torch.allclose(y1, y0, rtol=1e-12, atol=1e-12)
    for name, a, b in zip(R.FIRST, f1, f0):
        assert torch.isfinite(b).all(), name
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), name
    # second order: the composite is NaN (why it cannot be the oracle there), the double where is not
    assert not all(bool(torch.isfinite(t).all()) for t in s0 if t is not None)
    for name, a in zip(R.SECOND, s1):
        assert a is None or bool(torch.isfinite(a).all()), name
    # the dead channels' weight rows get nothing of either order
    assert not bool(f1[2][1].any()) and not bool(s1[3][1].any())  # block 1 vec1_proj.weight row 1
    assert not bool(f1[8][0].any()) and not bool(s1[9][0].any())  # block 2 vec1_proj.weight row 0
