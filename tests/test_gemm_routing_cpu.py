"""The dense-GEMM router (kernels.gemm_group / kernels.gemm_ex_launch) on CPU operands: the grouped and x3
envelopes refuse them before the native library is touched, so gemm_group gives the library result
and the epilogue entry launches nothing."""
import pytest
import torch


@pytest.fixture
def no_native(monkeypatch):
    from torchmdnet import _native, kernels

    def touched(*a, **k):
        raise AssertionError("the native library was touched for a CPU operand")
    for name in ("load", "stream"):
        monkeypatch.setattr(_native, name, touched)
    return kernels


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("trans_b", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("beta", [False, True])
def test_gemm_group_cpu_is_the_library(no_native, dtype, trans_b, with_bias, beta):
    kernels = no_native
    g = torch.Generator().manual_seed(3)
    M, N, K = 37, 48, 32
    A = torch.randn(M, K, generator=g, dtype=dtype)
    B = torch.randn((N, K) if trans_b else (K, N), generator=g, dtype=dtype)
    bias = torch.randn(N, generator=g, dtype=dtype) if with_bias else None
    C0 = torch.randn(M, N, generator=g, dtype=dtype)
    C = C0.clone()
    kernels.gemm_group([(A, B, trans_b, bias, C, beta)])
    Bop = B.t() if trans_b else B
    if beta:
        ref = C0.clone().addmm_(A, Bop)
        if with_bias:
            ref.add_(bias)
    else:
        ref = torch.addmm(bias, A, Bop) if with_bias else torch.mm(A, Bop)
    assert torch.equal(C, ref)
    # and that expression is the product: against fp64
    ref64 = A.double() @ Bop.double() + (bias.double() if with_bias else 0) + (C0.double() if beta else 0)
    tol = 1e-5 if dtype == torch.float32 else 1e-13
    assert float((C.double() - ref64).abs().max()) <= tol * float(ref64.abs().max())


def test_gemm_group_cpu_pair_and_record(no_native):
    """A group of two, one given as the record and one as a plain 6-tuple."""
    kernels = no_native
    g = torch.Generator().manual_seed(4)
    A, W1, W2 = torch.randn(5, 16, generator=g), torch.randn(7, 16, generator=g), torch.randn(16, 9, generator=g)
    C1, C2 = torch.empty(5, 7), torch.empty(5, 9)
    kernels.gemm_group([kernels.Gemm(A, W1, True, None, C1, False), (A, W2, False, None, C2, False)])
    assert torch.equal(C1, torch.mm(A, W1.t())) and torch.equal(C2, torch.mm(A, W2))


@pytest.mark.parametrize("rows", [37, 16384 + 37])
def test_gemm_ex_refuses_cpu_operands(no_native, rows):
    kernels = no_native
    A, W, b = torch.randn(rows, 32), torch.randn(48, 32), torch.randn(48)
    C, pre = torch.full((rows, 48), 7.0), torch.full((rows, 48), 7.0)
    assert kernels.gemm_ex_launch(kernels.Gemm(A, W, True, b, C, False, act=1, pre=pre)) is False
    assert bool((C == 7.0).all()) and bool((pre == 7.0).all())
