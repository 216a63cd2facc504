"""``kernels.cfconv_fused`` (tmdnet_cfconv_fused_image / _fwd / _bwd) against a float64 composite: torch basis ->
the two ``F.linear`` s of the filter network -> ``kernels.cfconv_composite``, differentiated by autograd for the
gradients of ``h``, the distances and the cutoff values.

Graphs (N <= 70) from explicit symmetric edge lists without self loops: one with row lengths 0, 1, 15, 16, 17, 33,
64 and 65 (the 16-edge tile's edges), one with static-capacity padding slots (``src = -1``).  ``r`` in
(0.3, cutoff) and ``C`` are drawn per PAIR and copied to both directions: the kernel's source pass relies on it.

Shapes (F, R): (16, 1), (32, 16), (48, 50), (64, 64), (128, 50), (128, 64) -- F not a multiple of 32, R below /
at / between the 32-wide k steps; every activation x basis at (32, 16) and (128, 50); add and mean everywhere.

Tolerance (the project's, tests/test_gpu_cfconv.py): float32 max|d| <= 1e-4 max|ref|."""
import math

import pytest
import torch
import torch.nn.functional as F_

from torchmdnet import _native as nat
from torchmdnet import kernels
from torchmdnet.kernels import EdgeGraph

pytestmark = pytest.mark.gpu

DEV = "cuda"
CU = 5.0
SSP, SILU = 1, 0
GAUSS, EXPNORM = nat.RBF_GAUSS, nat.RBF_EXPNORM

CASES = [(16, 1, SSP, GAUSS, 0.0), (48, 50, SILU, EXPNORM, 0.0), (64, 64, SSP, GAUSS, 0.0),
         (128, 64, SILU, EXPNORM, 0.2)]
CASES += [(F, R, a, b, 0.0) for (F, R) in ((32, 16), (128, 50)) for a in (SSP, SILU) for b in (GAUSS, EXPNORM)]


def _rows_pairs():
    """70 atoms; row lengths: 0: 65, 1: 64, 2: 33, 3: 17, 4: 16, 5: 15, 68: 1, 69: 0."""
    pairs = [(0, j) for j in range(1, 66)]
    pairs += [(1, j) for j in range(2, 65)]
    pairs += [(2, j) for j in range(3, 34)]
    pairs += [(3, j) for j in range(4, 18)]
    pairs += [(4, j) for j in range(5, 17)]
    pairs += [(5, j) for j in range(6, 16)]
    pairs += [(68, 65)]
    return sorted(set(pairs)), 70


def _small_pairs():
    return [(0, 1), (1, 2), (2, 3), (0, 3), (4, 5), (0, 2), (5, 6)], 8   # atom 7: an empty row


def _build(pairs, n, pad=0, seed=0, dev=DEV):
    """The CSR graph and per-pair r, C copied to both directions (float64, in the graph's edge order)."""
    gen = torch.Generator().manual_seed(seed)
    P = len(pairs)
    a = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    assert bool((a[0] != a[1]).all())
    ei = torch.stack([torch.cat([a[0], a[1]]), torch.cat([a[1], a[0]])]).to(dev)
    rp = 0.3 + (CU - 0.35) * torch.rand(P, generator=gen, dtype=torch.float64)
    cp = 0.05 + torch.rand(P, generator=gen, dtype=torch.float64)
    g, perm = EdgeGraph.from_edge_index(ei, n)
    assert g.symmetric
    r, C = torch.cat([rp, rp]).to(dev)[perm], torch.cat([cp, cp]).to(dev)[perm]
    if pad:  # static-capacity padding: slots beyond row_ptr[N] that no row references
        neg = torch.full((pad,), -1, dtype=torch.int32, device=dev)
        g.src, g.dst, g.transpose = torch.cat([g.src, neg]), torch.cat([g.dst, neg]), torch.cat([g.transpose, neg])
        g.static = True
        r = torch.cat([r, r.new_full((pad,), 1.0)])
        C = torch.cat([C, C.new_full((pad,), 0.5)])
    return g, r, C


GRAPHS = {"rows": lambda: _build(*_rows_pairs()), "padded": lambda: _build(*_small_pairs(), pad=7)}


def test_rows_graph_has_the_tile_edges():
    g, _, _ = GRAPHS["rows"]()
    lens = set((g.row_ptr[1:] - g.row_ptr[:-1]).tolist())
    assert {0, 1, 15, 16, 17, 33, 64, 65} <= lens, lens
    assert g.n_nodes <= 70 and bool((g.src != g.dst).all())


def _basis_params(R, basis, cl):
    if basis == GAUSS:
        mu = torch.linspace(cl, CU, R, dtype=torch.float64)
        coeff = -0.5 / ((CU - cl) / max(R - 1, 1)) ** 2
        return mu, torch.full((R,), coeff, dtype=torch.float64)
    start = math.exp(-CU + cl)
    return (torch.linspace(start, 1, R, dtype=torch.float64),
            torch.full((R,), (2 / R * (1 - start)) ** -2, dtype=torch.float64))


def _basis(r, mu, beta, basis, cl):
    d = r.unsqueeze(-1)
    if basis == GAUSS:
        return torch.exp(beta * (d - mu) ** 2)
    c0 = 0.5 * (torch.cos(d * math.pi / CU) + 1.0) * (d < CU).to(d.dtype)
    alpha = 5.0 / (CU - cl)
    return c0 * torch.exp(-beta * (torch.exp(alpha * (-d + cl)) - mu) ** 2)


def _act(x, act):
    return F_.silu(x) if act == SILU else F_.softplus(x) - kernels.SSP_SHIFT


def _inputs(g, F, R, basis, cl, seed=1):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    t = dict(h=mk(g.n_nodes, F), go=mk(g.n_nodes, F), w1=mk(F, R) / math.sqrt(R), b1=0.5 * mk(F),
             w2=mk(F, F) / math.sqrt(F), b2=0.5 * mk(F))
    t["mu"], t["beta"] = _basis_params(R, basis, cl)
    return {k: v.to(DEV) for k, v in t.items()}


def _reference(g, r, C, t, act, basis, cl, aggr):
    leaves = [x.clone().requires_grad_(True) for x in (t["h"], r, C)]
    h, rr, CC = leaves
    f = _basis(rr, t["mu"], t["beta"], basis, cl)
    w = F_.linear(_act(F_.linear(f, t["w1"], t["b1"]), act), t["w2"], t["b2"])
    out = kernels.cfconv_composite(h, w, CC, g.src.long(), g.dst.long(), g.n_nodes, aggr)
    return out, torch.autograd.grad(out, leaves, t["go"])


def _fused(g, r, C, t, act, basis, cl, aggr, create_graph=False):
    f32 = {k: v.float() for k, v in t.items()}
    leaves = [x.float().requires_grad_(True) for x in (t["h"], r, C)]
    out = kernels.cfconv_fused(leaves[0], leaves[1], leaves[2], g, f32["w1"], f32["b1"], f32["w2"], f32["b2"],
                               (f32["mu"], f32["beta"]), cl, CU, basis, act, aggr)
    grads = torch.autograd.grad(out, leaves, f32["go"], create_graph=create_graph)
    return out, grads, leaves, f32


def _close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    d = float((a - b).abs().max()) if a.numel() else 0.0
    ref = float(b.abs().max()) if b.numel() else 0.0
    print(f"{what}: max|d| = {d:.3e}, max|ref| = {ref:.3e}")
    assert d <= 1e-4 * max(ref, 1e-30), what


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("name", ["rows", "padded"])
@pytest.mark.parametrize("F,R,act,basis,cl", CASES,
                         ids=[f"F{c[0]}-R{c[1]}-{'ssp' if c[2] else 'silu'}-{'gauss' if c[3] == GAUSS else 'expnorm'}"
                              for c in CASES])
def test_fused_matches_float64_composite(F, R, act, basis, cl, name, aggr):
    g, r, C = GRAPHS[name]()
    t = _inputs(g, F, R, basis, cl)
    ref_out, ref_grads = _reference(g, r, C, t, act, basis, cl, aggr)
    out, grads, leaves, f32 = _fused(g, r, C, t, act, basis, cl, aggr)
    tag = f"{name} {aggr} F={F} R={R}"
    _close(out, ref_out, "out " + tag)
    real = int(g.row_ptr[-1])
    for what, a, b in zip(("gh", "gdist", "gcut"), grads, ref_grads):
        edge = what != "gh"
        _close(a[:real] if edge else a, b[:real] if edge else b, f"{what} {tag}")
        if edge:
            assert a.shape[0] == g.n_edges
            assert bool((a[real:] == 0).all()), f"{what}: padding slots not zero"
    empty = (g.row_ptr[1:] == g.row_ptr[:-1])
    assert bool(empty.any()) and bool((out[empty] == 0).all()), "an empty row's out is not exactly zero"
    # bitwise reproducible, inputs untouched
    out2, grads2, leaves2, f32b = _fused(g, r, C, t, act, basis, cl, aggr)
    assert torch.equal(out, out2)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    for a, b in zip(leaves, (t["h"], r, C)):
        assert torch.equal(a.detach(), b.float()), "an input was modified"
    for k, v in f32.items():
        assert torch.equal(v, t[k].float()), f"{k} was modified"


def test_second_backward_raises():
    g, r, C = GRAPHS["padded"]()
    t = _inputs(g, 32, 16, GAUSS, 0.0)
    out, grads, leaves, _ = _fused(g, r, C, t, SSP, GAUSS, 0.0, "add", create_graph=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        torch.autograd.grad((grads[1] ** 2).sum(), leaves[0])


def test_envelope_and_device_refusals():
    g, r, C = GRAPHS["padded"]()
    t = _inputs(g, 32, 16, GAUSS, 0.0)
    f32 = {k: v.float() for k, v in t.items()}
    args = lambda h, w1, w2, aggr="add": (h, r.float(), C.float(), g, w1, f32["b1"], w2, f32["b2"],  # noqa: E731
                                          (f32["mu"], f32["beta"]), 0.0, CU, GAUSS, SSP, aggr)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        kernels.cfconv_fused(*args(f32["h"].cpu(), f32["w1"], f32["w2"]))
    with pytest.raises(RuntimeError, match="float32"):
        kernels.cfconv_fused(*args(t["h"], f32["w1"], f32["w2"]))
    with pytest.raises(ValueError, match="aggr"):
        kernels.cfconv_fused(*args(f32["h"], f32["w1"], f32["w2"], aggr="max"))
    with pytest.raises(ValueError, match="num_filters"):
        kernels.cfconv_fused(*args(f32["h"][:, :24].contiguous(), f32["w1"][:24], f32["w2"][:24, :24]))
    # the C entry points refuse the same shapes with nothing launched
    lib = nat.load()
    assert lib.tmdnet_cfconv_fused_image_bytes(24, 16) == 0 and lib.tmdnet_cfconv_fused_image_bytes(128, 65) == 0
    assert lib.tmdnet_cfconv_fused_image_bytes(256, 50) == 0
