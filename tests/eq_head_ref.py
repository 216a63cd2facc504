"""Float64 references of the EquivariantScalar head for tests/test_gpu_eq_head_widths.py, its child-process worker
and tests/test_eq_head_ref.py: ``kernels.eq_head_composite`` evaluated in float64 on the CPU at the inputs and
weights as given (the float32-rounded ones when the kernel under test is fp32), differentiated by autograd to
first order (seed g_y: g_x, g_vec and the 12 weight gradients) and to second order (cotangents c_x, c_vec on
(g_x, g_vec): d_x, d_vec, d_gy and the 12 weight terms), plus ``composite_dw``, the same head with a norm whose
derivatives of every order are 0 at a zero channel.
"""
import torch
import torch.nn.functional as F

from torchmdnet import kernels

FIRST = ("g_x", "g_vec") + tuple(f"g_p{i}" for i in range(12))
SECOND = ("d_x", "d_vec", "d_gy") + tuple(f"d_p{i}" for i in range(12))


def norm_dw(vb):
    """|vb| over the axis dim (-2), per channel, as a double where: the square root never sees a zero, so a
    zero channel gets the value 0 and derivatives 0 of every order (the convention of csrc/eq_head.hip's HVP:
    "the norm's tangent and its gradient's tangent are 0 where the norm is 0")."""
    n2 = (vb * vb).sum(dim=-2)
    live = n2 > 0
    return torch.where(live, torch.sqrt(torch.where(live, n2, torch.ones_like(n2))), torch.zeros_like(n2))


def composite_dw(x, vec, params):
    """kernels.eq_head_composite with norm_dw in place of kernels.masked_norm."""
    for blk, scalar_act in ((0, True), (1, False)):
        w1, w2, u1w, u1b, u2w, u2b = params[6 * blk:6 * blk + 6]
        vec1 = norm_dw(torch.matmul(vec, w1.t()))
        vec2 = torch.matmul(vec, w2.t())
        o = F.linear(F.silu(F.linear(torch.cat([x, vec1], dim=-1), u1w, u1b)), u2w, u2b)
        xo, vo = torch.split(o, w2.shape[0], dim=-1)
        vec = vo.unsqueeze(1) * vec2
        x = F.silu(xo) if scalar_act else xo
    return x + vec.sum() * 0


def inputs(N, H, dtype, zero, seed=1):
    """x [N, H], vec [N, 3, H] on the CPU; atom ``zero`` has zero vector features (an isolated atom)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, generator=g, dtype=dtype)
    vec = torch.randn(N, 3, H, generator=g, dtype=dtype)
    vec[zero] = 0
    gy = torch.randn(N, 1, generator=g, dtype=dtype)
    cx = torch.randn(N, H, generator=g, dtype=dtype)
    cv = torch.randn(N, 3, H, generator=g, dtype=dtype)
    return x, vec, gy, cx, cv


def zero_channels(head):
    """Row 1 of block 1's vec1_proj.weight and row 0 of block 2's: one dead channel per block among live ones."""
    with torch.no_grad():
        head.output_network[0].vec1_proj.weight[1].zero_()
        head.output_network[1].vec1_proj.weight[0].zero_()
    return head


def reference(params, x, vec, gy, cx=None, cv=None, composite=None):
    """Float64 CPU reference.  Returns (y, first, second): ``first`` the 14 tensors named FIRST, ``second`` the
    15 named SECOND (None without cotangents; an entry is None where autograd finds no dependence)."""
    composite = composite or kernels.eq_head_composite
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    ps = [d(p).requires_grad_(True) for p in params]
    x, vec, gy = d(x).requires_grad_(True), d(vec).requires_grad_(True), d(gy).requires_grad_(True)
    y = composite(x, vec, ps)
    first = torch.autograd.grad(y, [x, vec] + ps, gy, create_graph=cx is not None)
    second = None
    if cx is not None:
        l2 = (first[0] * d(cx)).sum() + (first[1] * d(cv)).sum()
        second = torch.autograd.grad(l2, [x, vec, gy] + ps, allow_unused=True)
    return y.detach(), [t.detach() for t in first], second


def close(a, ref, dtype, what, worst=None):
    """The project's bars (tests/test_gpu_cfconv.py): float64 allclose(1e-9, 1e-9), float32 max|d| <= 1e-4
    max|ref|; a reference that is identically zero (or None) wants exact zeros or None.  Prints both figures;
    ``worst`` (a one-item list) keeps the largest float32 ratio seen."""
    if ref is None or not bool(ref.any()):
        assert a is None or not bool(a.any()), f"{what}: reference identically zero"
        print(f"{what}: identically zero")
        return
    assert a is not None, what
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert bool(torch.isfinite(a).all()), f"{what}: not finite"
    err, top = float((a - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max|d| = {err:.3e}, max|ref| = {top:.3e}, ratio {err / top:.2e}")
    if dtype == torch.float64:
        assert torch.allclose(a, ref, rtol=1e-9, atol=1e-9), (what, err)
    else:
        if worst is not None:
            worst[0] = max(worst[0], err / top)
        assert err <= 1e-4 * top, (what, err, top)
