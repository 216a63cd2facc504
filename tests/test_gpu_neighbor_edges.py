"""The neighbour-list builders (csrc/neighbors.hip) at box faces, cell boundaries and row limits.

Every list is compared with the dense fp64 reference of tests/neighbor_cases.py: pair sets exactly (the
cases keep every distance 1e-4 * cutoff away from the cutoffs), deltas and distances at the tolerances of
test_neighbor_op_matches_reference_fixtures (1e-5 fp32, 1e-12 fp64, absolute + relative).

Before `cell_axis` folded a negative cell index, the `cell` rows of the face cases (A), the pair numbering
on the face graph (F) and the gradient through it (G) failed: an atom one ulp below a +L/2 face was binned
at cx = -1 -- argued from the CPU restatement (test_neighbor_cases_cpu.py); the parent's kernel was not run
over these inputs, its key -1 writes outside cstart/cend."""
import numpy as np
import pytest
import torch

import neighbor_cases as NC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"f32": 1e-5, "f64": 1e-12}
GRAD_TOL = {"f32": 1e-4, "f64": 1e-10}  # test_neighbor_grads_match_oracle
TDT = {"f32": torch.float32, "f64": torch.float64}
BOTH = list(NC.DTYPES)


def _inputs(c):
    pos = torch.tensor(c.pos, device=DEV)
    assert pos.dtype == TDT[c.dtype]
    box = None if c.box is None else torch.tensor(c.box, dtype=pos.dtype)
    return pos, torch.tensor(c.batch, device=DEV), box


def _raw(c, strategy, cap, pad=True, want_csr=True, pairs_out=None):
    """One tmdnet_nl_build through kernels.neighbor_pairs_raw; a `cell` build without a box gets the
    3 * cutoff box that build_graph and the reference project substitute (deltas stay unwrapped)."""
    from torchmdnet import kernels
    pos, batch, box = _inputs(c)
    periodic = box is not None
    if strategy == "cell" and not periodic:
        box = torch.eye(3, dtype=torch.float64) * 3 * c.cutoff
    return kernels.neighbor_pairs_raw(strategy, pos, batch, box, periodic, c.lower, c.cutoff, cap, c.loop,
                                      c.transpose, pad_output=pad, want_csr=want_csr, pairs_out=pairs_out)


def _graph(c, strategy, **kw):
    from torchmdnet import kernels
    pos, batch, box = _inputs(c)
    P = NC.ref(c.name, c.dtype)[0].shape[1]
    kw.setdefault("max_num_pairs", P + 64)
    return kernels.build_graph(pos, batch, c.lower, c.cutoff, loop=c.loop, strategy=strategy, box=box, **kw)


def _check_list(c, nb, dl, dist, num, row_ptr=None):
    """Pair set == reference exactly; deltas / distances within tolerance; padding; CSR row pointer."""
    rp, rd, rr = NC.ref(c.name, c.dtype)
    P, n, tol = rp.shape[1], len(c.pos), TOL[c.dtype]
    assert int(num.item()) == P
    assert (nb[:, P:] == -1).all() and (dl[P:] == 0).all() and (dist[P:] == 0).all()
    got = nb[:, :P].cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < n
    got, gd, gr = NC.sort_edges(got, dl[:P].cpu().numpy(), dist[:P].cpu().numpy())
    ref, rd, rr = NC.sort_edges(rp, rd, rr)
    assert np.array_equal(got, ref)
    assert np.allclose(gd, rd, rtol=tol, atol=tol), np.abs(gd - rd).max()
    assert np.allclose(gr, rr, rtol=tol, atol=tol), np.abs(gr - rr).max()
    if row_ptr is not None:
        assert np.array_equal(row_ptr.cpu().numpy(), NC.row_ptr_of(rp, n))
        assert (nb[1, :P].cpu().numpy() == np.repeat(np.arange(n), np.diff(NC.row_ptr_of(rp, n)))).all()


def _check_graph(c, g, exact_transpose):
    """build_graph's contract: the reference's pairs row by row, a transpose map without holes."""
    rp, rd, rr = NC.ref(c.name, c.dtype)
    n, tol = len(c.pos), TOL[c.dtype]
    src, dst, T = g.src.cpu().numpy(), g.dst.cpu().numpy(), g.transpose.cpu().numpy().astype(np.int64)
    assert g.symmetric and g.num_pairs == rp.shape[1] == len(src)
    assert np.array_equal(g.row_ptr.cpu().numpy(), NC.row_ptr_of(rp, n))
    assert (T >= 0).all()
    assert np.array_equal(src[T], dst) and np.array_equal(dst[T], src)
    dl = g.deltas.detach().cpu().numpy()
    if exact_transpose:  # brute / shared: round() is odd-symmetric
        assert np.array_equal(dl[T], -dl)
    assert np.allclose(dl[T], -dl, rtol=tol, atol=tol)
    got, gd, gr = NC.sort_edges(np.stack([src, dst]).astype(np.int64), dl, g.distances.detach().cpu().numpy())
    ref, rd, rr = NC.sort_edges(rp, rd, rr)
    assert np.array_equal(got, ref)
    assert np.allclose(gd, rd, rtol=tol, atol=tol) and np.allclose(gr, rr, rtol=tol, atol=tol)


def _params(prefix):
    return [pytest.param(name, s, id=f"{name}-{s}") for name in NC.names(prefix)
            for s in NC.strategies(name)]


# ----------------------------------------------------------------------------- A. faces and cell boundaries
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name,strategy", _params("face_"))
def test_faces_and_cell_boundaries(name, strategy, dt):
    """Atoms on the box faces, the cell boundaries, the folded partial cell, one ulp either side of each
    and on their images: the raw list and the graph equal the reference for cell, brute and shared."""
    c = NC.get(name, dt)
    P = NC.ref(name, dt)[0].shape[1]
    nb, dl, dist, num, row_ptr, T = _raw(c, strategy, P + 64)
    _check_list(c, nb, dl, dist, num, row_ptr)
    assert (T[P:] == -1).all()
    _check_graph(c, _graph(c, strategy), exact_transpose=strategy != "cell")


# ----------------------------------------------------------------------------- B. grid shapes, C. row limits
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name,strategy", _params("grid_") + _params("rows_"))
def test_grid_shapes_and_row_limits(name, strategy, dt):
    """B (cell): one occupied cell, mostly empty grids, n = 1, 2, 257, sorted and shuffled molecules,
    loop x include_transpose, a lower cutoff.  C (brute, shared): molecule segments of 63, 64, 65, 129 and
    1 atoms (the 64-lane ballot loop at, below and above one and two iterations, segments off the
    64-boundary), a batch whose only descent is the last pair of a k_segments block or of the array, the
    half list, a lower cutoff with self pairs."""
    c = NC.get(name, dt)
    P = NC.ref(name, dt)[0].shape[1]
    nb, dl, dist, num, row_ptr, T = _raw(c, strategy, P + 64)
    _check_list(c, nb, dl, dist, num, row_ptr)
    if c.transpose:
        assert (T[:P] >= 0).all() and (T[P:] == -1).all()
        if c.loop:  # build_graph builds looped symmetric lists
            _check_graph(c, _graph(c, strategy), exact_transpose=strategy != "cell")
    else:
        assert T is None
        assert (nb[0, :P] >= nb[1, :P]).all()


# ----------------------------------------------------------------------------- D. k_scan chunking
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name,strategy", _params("scan_"))
def test_scan_chunks(name, strategy, dt):
    """n = 1, 1023, 1024, 1025, 2049: one, then two, then three counts per k_scan thread, with threads
    past the end.  row_ptr and num_pairs equal the reference's cumulative counts (the reference forms its
    rows in blocks)."""
    c = NC.get(name, dt)
    rp = NC.ref(name, dt)[0]
    nb, dl, dist, num, row_ptr, T = _raw(c, strategy, rp.shape[1] + 64)
    assert int(num.item()) == rp.shape[1]
    assert np.array_equal(row_ptr.cpu().numpy(), NC.row_ptr_of(rp, len(c.pos)))
    _check_list(c, nb, dl, dist, num, row_ptr)


# ----------------------------------------------------------------------------- E. capacity
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ["cell", "brute", "shared"])
def test_capacity_dynamic(strategy, dt):
    """cap = num_pairs - 7: the count is the true total, the kept slots are the first cap edges of the
    uncapped list (the CSR order is deterministic), T is -1 exactly where the reverse lies past cap, and
    the paired build's numbers stay inside their arrays."""
    c = NC.get("grid_n257", dt)
    P, n = NC.ref(c.name, dt)[0].shape[1], len(c.pos)
    full = _raw(c, strategy, P + 64, pad=False)
    _check_list(c, full[0][:, :P], full[1][:P], full[2][:P], full[3], full[4])
    cap = P - 7
    pairs_out = None
    if strategy != "cell":
        slots = (cap + n) // 2
        pairs_out = (torch.full((cap,), -7, dtype=torch.int32, device=DEV),
                     torch.full((slots,), -7, dtype=torch.int32, device=DEV))
    nb, dl, dist, num, row_ptr, T = _raw(c, strategy, cap, pad=False, pairs_out=pairs_out)
    assert int(num.item()) == P
    assert torch.equal(row_ptr, full[4])
    assert torch.equal(nb, full[0][:, :cap]) and torch.equal(dl, full[1][:cap]) and torch.equal(dist, full[2][:cap])
    Tf = full[5][:cap]
    assert (Tf[:cap] >= cap).any()  # some reverse edges do lie past cap
    assert torch.equal(T, torch.where(Tf < cap, Tf, torch.full_like(Tf, -1)))
    if pairs_out is not None:
        pr, pe = pairs_out
        assert pe.min() >= 0 and pe.max() < cap
        assert pr.min() >= 0 and pr.max() < slots


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ["cell", "brute", "shared"])
def test_capacity_static(strategy, dt):
    """static_capacity = num_pairs + 37: reference padding (-1 / 0), T = -1 in it, overflow clear; the
    flag is set at num_pairs - 1."""
    c = NC.get("grid_n257", dt)
    rp = NC.ref(c.name, dt)[0]
    P, n = rp.shape[1], len(c.pos)
    g = _graph(c, strategy, static_capacity=P + 37)
    assert g.n_edges == P + 37 and int(g.num_pairs_dev.item()) == P
    assert not g.overflow.item()
    assert (g.src[P:] == -1).all() and (g.dst[P:] == -1).all() and (g.transpose[P:] == -1).all()
    assert (g.deltas[P:] == 0).all() and (g.distances[P:] == 0).all()
    assert (g.transpose[:P] >= 0).all()
    _check_list(c, torch.stack([g.src, g.dst]), g.deltas.detach(), g.distances.detach(), g.num_pairs_dev, g.row_ptr)
    over = _graph(c, strategy, static_capacity=P - 1)
    assert over.overflow.item() and int(over.num_pairs_dev.item()) == P


# ----------------------------------------------------------------------------- F. pair numbering
@pytest.mark.parametrize("dt", BOTH)
def test_pair_index_on_face_graph(dt):
    """tmdnet_pair_index over the cell-built (31, 23, 17.5) face graph == the numbering restated in
    test_et_stack_cpu.pair_index_composite; every pair row holds an edge and its transpose."""
    from torchmdnet import kernels
    from test_et_stack_cpu import pair_index_composite
    c = NC.get("face_b31_n0", dt)
    g = _graph(c, "cell")
    assert not g.sorted_rows
    pr, pe = kernels.pair_index(g)
    cpu = kernels.EdgeGraph(g.n_nodes, g.row_ptr.cpu(), g.src.cpu(), g.dst.cpu(), g.transpose.cpu(), None, None,
                            g.num_pairs, True)
    rr, re = pair_index_composite(cpu)
    assert torch.equal(pr.cpu(), rr) and torch.equal(pe.cpu(), re)
    E, n = g.n_edges, g.n_nodes
    T = g.transpose.long()
    assert (T >= 0).all() and torch.equal(pr[T], pr)
    npairs = (E + n) // 2  # n self pairs, (E - n) / 2 two-edge pairs: every slot is used
    assert int(pr.max()) == npairs - 1 and pe.shape[0] == npairs
    canon = pe.long()[pr.long()]  # the canonical edge of each edge's pair: the edge itself or its reverse
    e = torch.arange(E, device=DEV)
    assert ((canon == e) | (canon == T)).all()
    assert torch.equal(torch.bincount(pr.long(), minlength=npairs),
                       torch.where(g.src[pe.long()] == g.dst[pe.long()], 1, 2))


# ----------------------------------------------------------------------------- G. gradient
@pytest.mark.parametrize("dt", BOTH)
def test_gradient_through_face_graph(dt):
    """d/dpos of (w * r).sum() + (wv * deltas).sum() through build_graph(strategy="cell") on a face case
    against fp64 autograd over the reference's pairs."""
    c = NC.get("face_b15_n0", dt)
    from torchmdnet import kernels
    pos, batch, box = _inputs(c)
    pos.requires_grad_(True)
    rp, rd, _ = NC.ref(c.name, dt)
    g = kernels.build_graph(pos, batch, 0.0, c.cutoff, rp.shape[1] + 64, loop=True, strategy="cell", box=box)
    E, n = g.n_edges, len(c.pos)
    assert E == rp.shape[1]
    # weights attached to the pair (s, t), not to an edge slot: the two lists order their edges differently
    gen = torch.Generator().manual_seed(5)
    W = torch.randn(n, n, generator=gen, dtype=torch.float64)
    WV = torch.randn(n, n, 3, generator=gen, dtype=torch.float64)
    s, t = g.src.long().cpu(), g.dst.long().cpu()
    (gp,) = torch.autograd.grad((g.distances * W[s, t].to(DEV, pos.dtype)).sum()
                                + (g.deltas * WV[s, t].to(DEV, pos.dtype)).sum(), pos)
    p64 = torch.tensor(np.asarray(c.pos, dtype=np.float64), requires_grad=True)
    rs, rt = torch.tensor(rp[0]), torch.tensor(rp[1])
    raw = p64[rs] - p64[rt]
    dl = raw + (torch.tensor(rd) - raw).detach()  # the minimum-image shift is piecewise constant
    selfe = rs == rt
    r = torch.where(selfe, torch.zeros(len(rs), dtype=torch.float64),
                    torch.where(selfe, torch.ones(len(rs), dtype=torch.float64), (dl * dl).sum(1)).sqrt())
    (gref,) = torch.autograd.grad((r * W[rs, rt]).sum() + (dl * WV[rs, rt]).sum(), p64)
    err = (gp.cpu().double() - gref).abs().max() / gref.abs().max()
    assert err < GRAD_TOL[dt], float(err)
