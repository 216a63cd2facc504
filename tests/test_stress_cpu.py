"""CPU tests of the differentiable virial: the plain-torch second order with the virial's cotangent
(kernels.nl_backward2_virial_composite, the restatement of tmdnet_nl_backward2 given g_virial) against autograd
through the two first-order composites, in float64 on the hand list of tests/test_virial_cpu.py, and what the
stress-training interface refuses without a device."""
import itertools

import pytest
import torch

from conftest import yaml_args
from test_virial_cpu import _hand_list
from torchmdnet import kernels

TOL = dict(rtol=1e-12, atol=1e-12)


def _operands(has, E, g):
    """(gd, gr, G, B) on the hand list, each present or None; B non-symmetric and different per molecule."""
    gd = torch.randn(E, 3, generator=g, dtype=torch.float64) if has[0] else None
    gr = torch.randn(E, generator=g, dtype=torch.float64) if has[1] else None
    G = torch.randn(5, 3, generator=g, dtype=torch.float64) if has[2] else None
    B = torch.randn(2, 3, 3, generator=g, dtype=torch.float64) if has[3] else None
    if B is not None:
        assert all(not torch.allclose(b, b.T) for b in B) and not torch.allclose(B[0], B[1])
    return gd, gr, G, B


def _autograd_reference(pos, src, dst, batch, gd, gr, G, B):
    """d S / d (pos, gd, gr) of S = <G, nl_backward_composite> + <B, nl_backward_virial_composite> by autograd.
    The first term is differentiated w.r.t. the positions directly (the composite forms its deltas from them);
    the second w.r.t. a deltas leaf (the distances recomputed from it), scattered to the two ends by hand:
    d_pos[n] = sum_{e: src = n} h_e - sum_{e: dst = n} h_e."""
    s, d = src.long(), dst.long()
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    p, gd_, gr_ = leaf(pos), leaf(gd), leaf(gr)
    dl0 = pos[s] - pos[d]
    r0 = dl0.norm(dim=1)
    dl = dl0.clone().requires_grad_(True)
    zero = r0 == 0
    r = torch.where(zero, torch.zeros_like(r0), torch.where(zero, torch.ones_like(r0), (dl * dl).sum(1)).sqrt())
    S = pos.new_zeros(())
    if G is not None:
        S = S + (G * kernels.nl_backward_composite(p, gd_, gr_, dl0, r0, src, dst)).sum()
    if B is not None:
        S = S + (B * kernels.nl_backward_virial_composite(gd_, gr_, None, dl, r, dst, batch, B.shape[0])).sum()
    ins = [t for t in (p, dl, gd_, gr_) if t is not None]
    if not S.requires_grad:
        grads = [None] * len(ins)
    else:
        grads = list(torch.autograd.grad(S, ins, allow_unused=True))
    it = iter(grads)
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    d_p, h = z(next(it), pos), z(next(it), dl0)
    d_gd = None if gd is None else z(next(it), gd)
    d_gr = None if gr is None else z(next(it), gr)
    d_pos = d_p + torch.zeros_like(pos).index_add(0, s, h).index_add(0, d, -h)
    return d_pos, d_gd, d_gr


@pytest.mark.parametrize("has", list(itertools.product([True, False], repeat=4)),
                         ids=lambda h: "".join(n for n, on in zip(("gd", "gr", "G", "B"), h) if on) or "none")
def test_composite_is_the_autograd_of_the_first_order(has):
    """(d_pos, d_gd, d_gr) of the composite against autograd of <G, gpos> + <B, out>, each of gd, gr, G, B present
    and None (the hand list has two self loops, an edge-free atom and two molecules)."""
    src, dst, batch, dl, r, g = _hand_list()
    pos = torch.randn(5, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    assert torch.equal(pos[src.long()] - pos[dst.long()], dl)  # _hand_list's own positions
    gd, gr, G, B = _operands(has, src.numel(), g)
    ref_pos, ref_gd, ref_gr = _autograd_reference(pos, src, dst, batch, gd, gr, G, B)
    d_pos, d_gd, d_gr = kernels.nl_backward2_virial_composite(pos, G, B, gd, gr, dl, r, src, dst, batch, 2)
    assert torch.allclose(d_pos, ref_pos, **TOL)
    if gd is not None:
        assert torch.allclose(d_gd, ref_gd, **TOL)
    if gr is not None:
        assert torch.allclose(d_gr, ref_gr, **TOL)
    if has[1] and has[3]:  # the B terms are there
        assert float(d_pos.abs().max()) > 1e-3
    self_loops = r == 0
    assert float(d_gd[self_loops].abs().max()) == 0 and float(d_gr[self_loops].abs().max()) == 0


def test_composite_without_a_virial_cotangent_is_the_plain_second_order():
    src, dst, batch, dl, r, g = _hand_list()
    pos = torch.randn(5, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    gd, gr, G, _ = _operands((True, True, True, False), src.numel(), g)
    got = kernels.nl_backward2_virial_composite(pos, G, None, gd, gr, dl, r, src, dst, batch, 2)
    ref = kernels.nl_backward2_composite(pos, G, gr, dl, r, src, dst)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, **TOL)


def test_composite_ignores_padding_slots():
    """Static-capacity padding: r == 0, destination -1 and NaN in every other per-edge buffer.  The live rows are
    what they are without the padding, the padding rows of d_gd and d_gr are exactly zero, and so are the gradients
    a third-order pass sends back through them."""
    src, dst, batch, dl, r, g = _hand_list()
    pos = torch.randn(5, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    E = src.numel()
    gd, gr, G, B = _operands((True, True, True, True), E, g)
    ref = kernels.nl_backward2_virial_composite(pos, G, B, gd, gr, dl, r, src, dst, batch, 2)
    nan = float("nan")
    pad = lambda t, v: torch.cat([t, torch.full((3,) + t.shape[1:], v, dtype=t.dtype)])
    gd_p, gr_p = pad(gd, nan).requires_grad_(True), pad(gr, nan).requires_grad_(True)
    got = kernels.nl_backward2_virial_composite(pos, G, B, gd_p, gr_p, pad(dl, nan), pad(r, 0.0), pad(src, -1),
                                                pad(dst, -1), batch, 2)
    assert torch.equal(got[0], ref[0])
    for a, b in zip(got[1:], ref[1:]):
        assert torch.equal(a[:E], b) and float(a[E:].abs().max()) == 0
    back = torch.autograd.grad(got[0].sum() + got[1].sum() + got[2].sum(), (gd_p, gr_p))
    for t in back:
        assert bool(torch.isfinite(t).all()) and float(t[E:].abs().max()) == 0


def test_composite_skips_molecules_outside_the_range():
    """batch values outside [0, n_mol) for one molecule: its rows behave as B = 0."""
    src, dst, batch, dl, r, g = _hand_list()
    pos = torch.randn(5, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    gd, gr, G, B = _operands((True, True, True, True), src.numel(), g)
    out_of_range = torch.where(batch == 1, torch.full_like(batch, 7), batch)
    got = kernels.nl_backward2_virial_composite(pos, G, B, gd, gr, dl, r, src, dst, out_of_range, 2)
    B0 = B.clone()
    B0[1] = 0
    ref = kernels.nl_backward2_virial_composite(pos, G, B0, gd, gr, dl, r, src, dst, batch, 2)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_pairwise_edge_sums_are_the_same_sums():
    """tests/stress_ref.pairwise_edge_sums: index_add / index_select over dim 0 give the same values and gradients
    (to rounding), the methods are put back, and a sum of many identical addends -- the static padding case -- is
    closer to the exact product than the one-after-the-other sum."""
    import stress_ref as SR
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 7, (500,), generator=g)
    src = torch.randn(500, 4, 3, generator=g, dtype=torch.float64, requires_grad=True)
    base = torch.randn(7, 4, 3, generator=g, dtype=torch.float64)
    ref = base.index_add(0, idx, src).index_select(0, idx)
    g_ref, = torch.autograd.grad((ref ** 2).sum(), src)
    orig = (torch.Tensor.index_add, torch.Tensor.index_select)
    with SR.pairwise_edge_sums():
        got = base.index_add(0, idx, src).index_select(0, idx)
        g_got, = torch.autograd.grad((got ** 2).sum(), src)
        ints = torch.arange(7).index_select(0, idx)  # non-floating tensors go the usual way
    assert (torch.Tensor.index_add, torch.Tensor.index_select) == orig
    assert torch.equal(ints, idx)
    assert torch.allclose(got, ref, rtol=1e-13, atol=1e-13) and torch.allclose(g_got, g_ref, rtol=1e-12, atol=1e-12)
    c = torch.rand(1, 64, generator=g, dtype=torch.float64) + 0.5
    n = 4700
    exact = (c * n)  # one rounding
    zeros = torch.zeros(n, dtype=torch.long)
    seq = torch.zeros(1, 64, dtype=torch.float64).index_add(0, zeros, c.expand(n, 64))
    with SR.pairwise_edge_sums():
        blk = torch.zeros(1, 64, dtype=torch.float64).index_add(0, zeros, c.expand(n, 64))
    err = lambda t: float(((t - exact) / exact).abs().max())
    print(f"{n} identical addends: sequential {err(seq):.2e}, pairwise {err(blk):.2e}")
    assert err(blk) <= 1e-14 and err(blk) <= err(seq)


# ----------------------------------------------------------------------------- refusals that need no device
def _inputs():
    z = torch.tensor([8, 1, 1], dtype=torch.long)
    return z, torch.randn(3, 3), torch.zeros(3, dtype=torch.long)


def test_create_graph_refuses_a_half_storage_model():
    from torchmdnet.models.model import create_model
    m = create_model(yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=1, derivative=True,
                               precision=16))
    assert m._half_storage
    z, pos, batch = _inputs()
    with pytest.raises(ValueError, match="precision-16"):
        m.energy_forces_virial(z, pos.half(), batch, create_graph=True)


def test_create_graph_refuses_a_wrapped_representation_model():
    from torchmdnet.models.model import create_model
    m = create_model(yaml_args("graph-network", embedding_dimension=32, num_layers=1, derivative=False,
                               atom_filter=1, aggr="add", neighbor_embedding=True, output_model="Scalar",
                               reduce_op="add"))
    m.derivative = True  # as tests/test_virial_cpu.py reaches the wrapper check
    with pytest.raises(ValueError, match="AtomFilter"):
        m.energy_forces_virial(*_inputs(), create_graph=True)


def _tiny():
    from torchmdnet.models.model import create_model
    return create_model(yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=1, derivative=True))


def test_captured_trainers_refuse_a_virial_weight():
    """Raised on the host before anything touches a device (CPU tensors, no library call)."""
    from torchmdnet.training import GraphedTrainStep, PaddedGraphedTrainer
    z, pos, batch = _inputs()
    with pytest.raises(ValueError, match="virial_weight"):
        GraphedTrainStep(_tiny(), z, pos, batch, torch.zeros(1, 1), torch.zeros(3, 3), virial_weight=1.0)
    with pytest.raises(ValueError, match="virial_weight"):
        PaddedGraphedTrainer(_tiny(), None, virial_weight=0.5)


def test_lnnp_step_with_a_virial_weight_needs_the_label():
    from torchmdnet.training import LNNPStep
    tr = LNNPStep(_tiny(), virial_weight=1.0)
    assert tr.virial_weight == 1.0 and LNNPStep(_tiny()).virial_weight == 0.0
    z, pos, batch = _inputs()
    with pytest.raises(ValueError, match="virial label"):
        tr.loss(z, pos, batch, torch.zeros(1, 1), torch.zeros(3, 3))
