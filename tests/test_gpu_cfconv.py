"""``kernels.cfconv`` (tmdnet_cfconv_fwd / _bwd / _bwd2) against its float64 composite, on graphs built with
``EdgeGraph.from_edge_index`` from explicit symmetric edge lists.

Graphs (N <= 70): one with row lengths 0, 1, 4, 5, 64 and 65; one with a self loop; one with static-capacity
padding.  Widths 1, 7, 66, 128, 256, 320 (one channel group, several, a partly filled last one, V = 1 / 2 / 4).
``w`` and ``C`` are drawn per directed edge (not pair-symmetric).

Tolerances (the project's, tests/test_gpu_pair_priors.py): float64 rtol = atol = 1e-9; float32
max|d| <= 1e-4 max|ref|.  For max in float32 the winner may differ from float64's where two messages lie within
rounding: the returned ``arg`` must point at a message within 4 * 2^-24 * max|m| of the float64 row maximum (two
roundings per product; in float64 it must point at the row maximum itself), and values and gradients are compared
with the composite evaluated at the kernel's own ``arg``."""
import numpy as np
import pytest
import torch

from torchmdnet import kernels
from torchmdnet.kernels import EdgeGraph

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = [1, 7, 66, 128, 256, 320]
AGGRS = ["add", "mean", "max"]


def _sym(pairs):
    pairs = sorted(set((min(a, b), max(a, b)) for a, b in pairs if a != b))
    return [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]


def _rows_graph():
    """70 atoms; row lengths: atom 69: 0; 68: 1; 0: 65; 1: 64 (+ its edge to 0); 66: 4; 67: 5; the rest small."""
    pairs = [(0, j) for j in range(1, 66)]        # atom 0: 65
    pairs += [(1, j) for j in range(2, 65)]       # atom 1: 1 + 63 = 64
    pairs += [(66, j) for j in (2, 3, 4, 5)]      # atom 66: 4
    pairs += [(67, j) for j in (2, 3, 4, 5, 6)]   # atom 67: 5
    pairs += [(68, 65)]                           # atom 68: 1; atom 69: 0
    return _sym(pairs), 70


def _loop_graph():
    return _sym([(0, 1), (1, 2), (2, 3), (0, 3), (4, 5)]) + [(2, 2)], 7


def _build(edges, n, pad=0):
    ei = torch.tensor(edges, dtype=torch.long, device=DEV).t().contiguous()
    g, _ = EdgeGraph.from_edge_index(ei, n)
    assert g.symmetric
    if pad:  # static-capacity padding: slots beyond row_ptr[N] that no row references
        neg = torch.full((pad,), -1, dtype=torch.int32, device=DEV)
        g.src, g.dst, g.transpose = torch.cat([g.src, neg]), torch.cat([g.dst, neg]), torch.cat([g.transpose, neg])
        g.static = True
    return g


GRAPHS = {"rows": lambda: _build(*_rows_graph()), "loop": lambda: _build(*_loop_graph()),
          "padded": lambda: _build(*_loop_graph(), pad=5)}


def _check_rows():
    g = GRAPHS["rows"]()
    lens = set((g.row_ptr[1:] - g.row_ptr[:-1]).tolist())
    assert {0, 1, 4, 5, 64, 65} <= lens, lens


def _inputs(g, F, seed=0):
    gen = torch.Generator().manual_seed(seed)
    E, N = g.n_edges, g.n_nodes
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(DEV)  # noqa: E731
    return mk(N, F), mk(E, F), mk(E).abs() + 0.1, mk(N, F)


def _close(a, b, dtype, what):
    a, b = a.double(), b.double()
    d = float((a - b).abs().max()) if a.numel() else 0.0
    ref = float(b.abs().max()) if b.numel() else 0.0
    print(f"{what}: max|d| = {d:.3e}, max|ref| = {ref:.3e}")
    if dtype == torch.float64:
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-9), what
    else:
        assert d <= 1e-4 * max(ref, 1e-30), what


def _check_arg(g, arg, h64, w64, C64, dtype):
    """The kernel's winners against the float64 messages (see the module docstring)."""
    src, dst = g.src.long().clamp(min=0), g.dst.long()
    real = g.src >= 0
    m = h64[src] * (w64 * C64[:, None])
    m = torch.where(real[:, None], m, m.new_full((), -float("inf")))
    N, F = h64.shape
    top = m.new_full((N, F), -float("inf")).scatter_reduce(0, dst.clamp(min=0)[:, None].expand(-1, F), m, "amax")
    empty = top == -float("inf")
    assert bool(((arg < 0) == empty).all())
    a = arg.long().clamp(min=0)
    assert bool((dst[a] == torch.arange(N, device=DEV)[:, None])[~empty].all()), "arg outside its row"
    picked = m.gather(0, a)
    # float64: the kernel forms the same products, so its winner IS the float64 row maximum
    tol = 4 * 2.0 ** -24 * float(m[real].abs().max()) if dtype == torch.float32 else 0.0
    assert bool(((top - picked)[~empty] <= tol).all())


def _run(g, F, dtype, aggr, order):
    h64, w64, C64, go64 = _inputs(g, F)
    E = g.n_edges
    src, dst = g.src.long(), g.dst.long()
    leaves = [t.to(dtype).requires_grad_(True) for t in (h64, w64, C64)]
    out, arg = kernels.cfconv(*leaves, g, aggr, return_arg=True)
    use_arg = None
    if aggr == "max":
        _check_arg(g, arg, h64, w64, C64, dtype)
        use_arg = arg
    ref_leaves = [t.clone().requires_grad_(True) for t in (h64, w64, C64)]
    ref = kernels.cfconv_composite(*ref_leaves, src, dst, g.n_nodes, aggr, arg=use_arg)
    _close(out, ref, dtype, f"out {aggr} F={F}")
    if aggr == "max" and dtype == torch.float64:  # the composite's own winners agree with the kernel's values
        _close(out, kernels.cfconv_composite(h64, w64, C64, src, dst, g.n_nodes, aggr), dtype, "own amax")
    go = go64.to(dtype).requires_grad_(True)
    gor = go64.clone().requires_grad_(True)
    grads = torch.autograd.grad(out, leaves, go, create_graph=True)
    rgrads = torch.autograd.grad(ref, ref_leaves, gor, create_graph=True)
    real = int(g.row_ptr[-1])
    for name, a, b in zip(("gh", "gw", "gC"), grads, rgrads):
        _close(a[:real] if name != "gh" else a, b[:real] if name != "gh" else b, dtype, f"{name} {aggr} F={F}")
        if name != "gh" and E > real:
            assert bool((a[real:] == 0).all()), f"{name}: padding slots not zero"
    if order < 2:
        return out, grads
    loss = sum((a ** 2).sum() for a in grads)
    rloss = sum((b ** 2).sum() for b in rgrads)  # (the composite's padding slots are zero)
    second = torch.autograd.grad(loss, [go] + leaves)
    rsecond = torch.autograd.grad(rloss, [gor] + ref_leaves)
    for name, a, b in zip(("d_g", "d_h", "d_w", "d_C"), second, rsecond):
        edge = name in ("d_w", "d_C")
        _close(a[:real] if edge else a, b[:real] if edge else b, dtype, f"{name} {aggr} F={F}")
        if edge and E > real:
            assert bool((a[real:] == 0).all()), f"{name}: padding slots not zero"
    return out, grads


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("F", WIDTHS)
def test_cfconv_rows_graph(F, dtype, aggr):
    _check_rows()
    _run(GRAPHS["rows"](), F, dtype, aggr, order=2 if F <= 128 else 1)


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["loop", "padded"])
def test_cfconv_self_loop_and_padding(name, dtype, aggr):
    for F in (7, 128):
        _run(GRAPHS[name](), F, dtype, aggr, order=2)


@pytest.mark.parametrize("aggr", AGGRS)
def test_cfconv_bitwise_reproducible(aggr):
    g = GRAPHS["rows"]()
    a_out, a_grads = _run(g, 66, torch.float32, aggr, order=1)
    b_out, b_grads = _run(g, 66, torch.float32, aggr, order=1)
    assert torch.equal(a_out, b_out)
    for a, b in zip(a_grads, b_grads):
        assert torch.equal(a, b)


def test_cfconv_asymmetric_list_refused():
    ei = torch.tensor([[0, 1, 2], [1, 0, 0]], dtype=torch.long, device=DEV)  # 2 -> 0 has no reverse
    g, _ = EdgeGraph.from_edge_index(ei, 3)
    assert not g.symmetric
    h = torch.randn(3, 8, device=DEV, requires_grad=True)
    w = torch.randn(3, 8, device=DEV, requires_grad=True)
    C = torch.rand(3, device=DEV)
    out = kernels.cfconv(h, w, C, g, "add")
    with pytest.raises(RuntimeError, match="needs a symmetric edge list"):
        out.sum().backward()
    gw, = torch.autograd.grad(kernels.cfconv(h.detach(), w, C, g, "add").sum(), w)  # no source pass: fine
    assert np.isfinite(gw.cpu().numpy()).all()
