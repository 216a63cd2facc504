"""The dense-GEMM front door (kernels.gemm_group / kernels.gemm_ex_launch / kernels.mlp_act's decision): which of
the three back ends -- the grouped split-K kernel, the x3 kernel above GEMM_MAX_ROWS rows, the library --
a problem reaches, the value it gets there, and that a refused problem launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M_SMALL = 37


def _m_big():
    from torchmdnet import kernels
    return kernels.GEMM_MAX_ROWS + 37


def _prob(M, K, N, tb, bias, beta, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    o = dict(device=DEV, dtype=dtype, generator=g)
    A = torch.randn(M, K, **o)
    B = (torch.randn(N, K, **o) if tb else torch.randn(K, N, **o)) / K ** 0.5
    b = torch.randn(N, **o) if bias else None
    C0 = torch.randn(M, N, **o)
    return [A, B, tb, b, C0.clone(), beta], C0


def _lib(p, C0):
    """The library expression gemm_group's fallback evaluates (same calls, same operands)."""
    A, B, tb, b, _, beta = p
    Bop = B.t() if tb else B
    if beta:
        out = C0.clone().addmm_(A, Bop)
        return out.add_(b) if b is not None else out
    return torch.addmm(b, A, Bop) if b is not None else torch.mm(A, Bop)


def _ref64(p, C0):
    A, B, tb, b, _, beta = p
    ref = A.double() @ (B.t() if tb else B).double()
    if b is not None:
        ref = ref + b.double()
    return ref + C0.double() if beta else ref


def _check(route, p, C0):
    C, ref = p[4], _ref64(p, C0)
    scale = float(ref.abs().max())
    e = float((C.double() - ref).abs().max())
    if route == "grouped":  # test_grouped_gemm_matches_torch's bar
        assert e / scale < 2e-6, (e, scale)
    elif route == "x3":  # test_gemm_x3_large_rows_match_fp64_like_library's bar
        A, B, tb, b, _, beta = p
        lib = A @ (B.t() if tb else B)
        lib = lib + b if b is not None else lib
        lib = lib + C0 if beta else lib
        e_lib = float((lib.double() - ref).abs().max())
        assert e <= 2 * e_lib + 4 * 2.0 ** -24 * scale, (e, e_lib, scale)
    else:
        assert torch.equal(C, _lib(p, C0))


@pytest.fixture
def routes(monkeypatch):
    """Wraps the three launch entries; records (entry, problems) of every call that launched."""
    from torchmdnet import kernels
    seen = []
    grouped, x3, lib = kernels.gemm_launch, kernels.gemm_x3, kernels.gemm_lib

    def w_grouped(ps):
        ok = grouped(ps)
        if ok:
            seen.append(("grouped", len(ps)))
        return ok

    def w_x3(*a):
        ok = x3(*a)
        if ok:
            seen.append(("x3", 1))
        return ok

    def w_lib(p):
        seen.append(("lib", 1))
        return lib(p)
    monkeypatch.setattr(kernels, "gemm_launch", w_grouped)
    monkeypatch.setattr(kernels, "gemm_x3", w_x3)
    monkeypatch.setattr(kernels, "gemm_lib", w_lib)
    return seen


def _offset_a(M, K, N):
    p, C0 = _prob(M, K, N, True, True, False, 11)
    buf = torch.empty(M * K + 1, device=DEV)
    buf[1:].copy_(p[0].reshape(-1))
    p[0] = buf[1:].view(M, K)  # one float past a 16-byte boundary
    return [(p, C0)]


def _strided_b(M, K, N):
    p, C0 = _prob(M, K, N, True, False, False, 12)
    wide = torch.zeros(N, 2 * K, device=DEV)
    wide[:, ::2] = p[1]
    p[1] = wide[:, ::2]  # column stride 2
    return [(p, C0)]


def _cases():
    S, Bg = M_SMALL, _m_big()
    return {
        # NT with bias and NN accumulating, both within the grouped kernel: one launch
        "grouped_pair": ([_prob(S, 32, 48, True, True, False, 1), _prob(3 * S, 96, 16, False, False, True, 2)],
                         [("grouped", 2)], ["grouped", "grouped"]),
        "big_pair": ([_prob(Bg, 32, 48, True, True, False, 3), _prob(Bg, 96, 16, False, False, True, 4)],
                     [("x3", 1), ("x3", 1)], ["x3", "x3"]),
        "both_sides": ([_prob(S, 16, 96, True, True, False, 5), _prob(Bg, 32, 16, True, False, False, 6)],
                       [("grouped", 1), ("x3", 1)], ["grouped", "x3"]),
        "k72_small": ([_prob(S, 72, 48, True, True, False, 7)], [("lib", 1)], ["lib"]),
        "k48_big": ([_prob(Bg, 48, 32, True, True, False, 8)], [("lib", 1)], ["lib"]),
        "fp64_small": ([_prob(S, 32, 48, True, True, False, 9, torch.float64)], [("lib", 1)], ["lib"]),
        "fp64_big": ([_prob(Bg, 32, 48, False, False, True, 10, torch.float64)], [("lib", 1)], ["lib"]),
        "offset_a_small": (_offset_a(S, 32, 48), [("lib", 1)], ["lib"]),
        "offset_a_big": (_offset_a(Bg, 32, 48), [("lib", 1)], ["lib"]),
        "strided_b_small": (_strided_b(S, 32, 48), [("lib", 1)], ["lib"]),
        "strided_b_big": (_strided_b(Bg, 32, 48), [("lib", 1)], ["lib"]),
    }


@pytest.mark.parametrize("case", ["grouped_pair", "big_pair", "both_sides", "k72_small", "k48_big", "fp64_small",
                                  "fp64_big", "offset_a_small", "offset_a_big", "strided_b_small", "strided_b_big"])
def test_gemm_group_route_and_value(case, routes):
    from torchmdnet import kernels
    probs, expect, kinds = _cases()[case]
    kernels.gemm_group([tuple(p) for p, _ in probs])
    assert routes == expect
    for (p, C0), kind in zip(probs, kinds):
        _check(kind, p, C0)


SENTINEL = -77.0


def _refused(M, which):
    """(Gemm, C, pre) of an epilogue problem (K = 32, N = 48) one operand of which is outside both envelopes."""
    from torchmdnet import kernels
    g = torch.Generator(device=DEV).manual_seed(21)
    A = torch.randn(M, 32, device=DEV, generator=g)
    W = torch.randn(48, 32, device=DEV, generator=g)
    b = torch.randn(48, device=DEV, generator=g)
    C = torch.full((M, 48), SENTINEL, device=DEV)
    if which == "rscale":  # a strided row scale
        pre = torch.full((M, 48), SENTINEL, device=DEV)
        rs = torch.rand(2 * M, device=DEV, generator=g)[::2]
        return kernels.Gemm(A, W, True, b, C, False, act=1, pre=pre, rscale=rs), C, pre
    # pre a column slice of a wider buffer, dpre dense: two row strides
    pre = torch.full((M, 64), SENTINEL, device=DEV)
    dpre = torch.randn(M, 48, device=DEV, generator=g)
    return kernels.Gemm(A, W, True, b, C, False, pre=pre[:, :48], dpre=dpre), C, pre


@pytest.mark.parametrize("which", ["rscale", "pre_stride"])
@pytest.mark.parametrize("big", [True, False])
def test_gemm_ex_refusal_launches_nothing(big, which, routes):
    """The epilogue entry outside the envelope returns False and writes nothing.  Before the envelopes were
    stated once, the two large-row cases raised ("refused a checked problem": the pre-check lacked the x3
    kernel's rscale and common-row-stride conditions) and the small-row strided rscale was read as dense, so
    the launch went ahead on wrong data."""
    from torchmdnet import kernels
    p, C, pre = _refused(_m_big() if big else M_SMALL, which)
    assert kernels.gemm_ex_launch(p) is False
    torch.cuda.synchronize()
    assert routes == []
    assert bool((C == SENTINEL).all()) and bool((pre == SENTINEL).all())


# (rows, layer widths) -> whether kernels.mlp_act takes the fused path; recorded once from the code before the
# shape-level predicates replaced mlp_act's own "mod = 32 if big else 16" test.  The small rows are those of
# test_gpu_mlp.py's test_mlp_act_matches_composite / test_mlp_act_falls_back_outside_envelope.
MLP_DECISIONS = [
    (3360, (32, 128, 256, 384), True),
    (168, (128, 128, 128), True),
    (168, (384, 128), True),
    (37, (16, 48, 32), True),
    (50, (20, 32, 16), False),
    ("big", (32, 64, 32), True),
    ("big", (16, 48, 32), False),
]


@pytest.mark.parametrize("rows,dims,fused", MLP_DECISIONS)
def test_mlp_act_decision(rows, dims, fused, monkeypatch):
    from torchmdnet import kernels

    class Taken:
        apply = staticmethod(lambda *a: "fused")
    monkeypatch.setattr(kernels, "_MLPAct", Taken)
    M = _m_big() if rows == "big" else rows
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(M, dims[0], device=DEV, generator=g)
    ws = [torch.randn(dims[i + 1], dims[i], device=DEV, generator=g) for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], device=DEV, generator=g) for i in range(len(dims) - 1)]
    sc = torch.rand(M, device=DEV, generator=g)
    out = kernels.mlp_act(x, ws, bs, torch.nn.SiLU(), sc)
    assert (isinstance(out, str) and out == "fused") == fused
