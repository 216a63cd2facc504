"""The cell-list build of csrc/neighbors.hip in triclinic periodic boxes (k_cell_assign / k_cell_pairs with
TRIC): fractional-coordinate cells along the lattice directions, pairs accepted with the triclinic minimum
image of the brute strategy.

Every list is compared with the dense fp64 reference of tests/neighbor_cases.py over the inputs of
tests/neighbor_cases_tric.py: pair sets exactly (every distance is kept 1e-4 * cutoff away from the
cutoffs), deltas and distances at 1e-5 (fp32) / 1e-12 (fp64); the cell list against brute bitwise.  Without
the triclinic path every `cell` build here raises 'Expected "box_size" to be diagonal'."""
import ctypes

import numpy as np
import pytest
import torch

import neighbor_cases as NC
import neighbor_cases_tric as TC
from conftest import yaml_args

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"f32": 1e-5, "f64": 1e-12}
GRAD_TOL = {"f32": 1e-4, "f64": 1e-10}  # test_gpu_neighbor_edges.GRAD_TOL
TDT = {"f32": torch.float32, "f64": torch.float64}
BOTH = list(TC.DTYPES)


def _inputs(c):
    pos = torch.tensor(c.pos, device=DEV)
    assert pos.dtype == TDT[c.dtype]
    return pos, torch.tensor(c.batch, device=DEV), torch.tensor(c.box, dtype=pos.dtype)


def _raw(c, strategy, cap, pad=True):
    from torchmdnet import kernels
    pos, batch, box = _inputs(c)
    return kernels.neighbor_pairs_raw(strategy, pos, batch, box, True, c.lower, c.cutoff, cap, c.loop, c.transpose,
                                      pad_output=pad, want_csr=True)


def _graph(c, strategy, pos=None, **kw):
    from torchmdnet import kernels
    p, batch, box = _inputs(c)
    P = TC.ref(c.name, c.dtype)[0].shape[1]
    kw.setdefault("max_num_pairs", P + 64)
    return kernels.build_graph(p if pos is None else pos, batch, c.lower, c.cutoff, loop=c.loop, strategy=strategy,
                               box=box, **kw)


def _sorted_list(nb, dl, dist, P):
    got = nb[:, :P].cpu().numpy().astype(np.int64)
    return NC.sort_edges(got, dl[:P].detach().cpu().numpy(), dist[:P].detach().cpu().numpy())


def _check_list(c, nb, dl, dist, num, row_ptr):
    """Pair set == reference exactly; deltas / distances within tolerance; padding; CSR row pointer."""
    rp, rd, rr = TC.ref(c.name, c.dtype)
    P, n, tol = rp.shape[1], len(c.pos), TOL[c.dtype]
    assert int(num.item()) == P
    assert (nb[:, P:] == -1).all() and (dl[P:] == 0).all() and (dist[P:] == 0).all()
    got = nb[:, :P].cpu().numpy()
    assert got.min() >= 0 and got.max() < n
    got, gd, gr = _sorted_list(nb, dl, dist, P)
    ref, rd, rr = NC.sort_edges(rp, rd, rr)
    assert np.array_equal(got, ref)
    print(f"{c.name} {c.dtype}: {P} pairs, max|d delta| = {np.abs(gd - rd).max():.3e}, "
          f"max|d r| = {np.abs(gr - rr).max():.3e}")
    assert np.allclose(gd, rd, rtol=tol, atol=tol), np.abs(gd - rd).max()
    assert np.allclose(gr, rr, rtol=tol, atol=tol), np.abs(gr - rr).max()
    assert np.array_equal(row_ptr.cpu().numpy(), NC.row_ptr_of(rp, n))
    assert (nb[1, :P].cpu().numpy() == np.repeat(np.arange(n), np.diff(NC.row_ptr_of(rp, n)))).all()


def _params(prefix=""):
    return [pytest.param(name, s, id=f"{name}-{s}") for name in TC.names(prefix) for s in TC.strategies(name)]


# ----------------------------------------------------------------------------- raw build
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name,strategy", _params())
def test_raw_build_matches_reference(name, strategy, dt):
    """Faces of the fractional cells of four boxes (every cell scanned; pruning on every axis; the extreme
    skews validate_box admits, both signs) for cell, brute and shared; on (31, 23, 17.5)-skewed: n = 1, 2
    (a pair across the skewed c face), 257, sorted and shuffled molecules, loop x include_transpose, a
    lower cutoff."""
    c = TC.get(name, dt)
    P = TC.ref(name, dt)[0].shape[1]
    nb, dl, dist, num, row_ptr, T = _raw(c, strategy, P + 64)
    _check_list(c, nb, dl, dist, num, row_ptr)
    if c.transpose:
        assert (T[:P] >= 0).all() and (T[P:] == -1).all()
    else:
        assert T is None
        assert (nb[0, :P] >= nb[1, :P]).all()


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name", TC.FACE_CASES)
def test_cell_equals_brute_bitwise(name, dt):
    """The same Tric::apply on the same pos[s] - pos[t]: after sorting the edges, the cell list's deltas
    and distances are brute's bit for bit."""
    c = TC.get(name, dt)
    P = TC.ref(name, dt)[0].shape[1]
    cell = _raw(c, "cell", P + 64)
    brute = _raw(c, "brute", P + 64)
    assert int(cell[3].item()) == int(brute[3].item()) == P
    cp, cd, cr = _sorted_list(cell[0], cell[1], cell[2], P)
    bp, bd, br = _sorted_list(brute[0], brute[1], brute[2], P)
    assert np.array_equal(cp, bp)
    assert np.array_equal(cd, bd) and np.array_equal(cr, br)


# ----------------------------------------------------------------------------- build_graph
def _functional(g, n, dtype):
    """A random linear functional of (deltas, distances) with weights attached to the pair (s, t), not to
    an edge slot: the cell and the brute graph order their edges differently."""
    gen = torch.Generator().manual_seed(5)
    W = torch.randn(n, n, generator=gen, dtype=torch.float64)
    WV = torch.randn(n, n, 3, generator=gen, dtype=torch.float64)
    s, t = g.src.long().cpu().clamp_min(0), g.dst.long().cpu().clamp_min(0)  # padding: zero deltas / distances
    return (g.distances * W[s, t].to(DEV, dtype)).sum() + (g.deltas * WV[s, t].to(DEV, dtype)).sum()


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("form", ["dynamic", "static"])
@pytest.mark.parametrize("name", ["face_t31", "face_tmax"])
def test_graph_on_face_cases(name, form, dt):
    from torchmdnet import kernels
    c = TC.get(name, dt)
    rp = TC.ref(name, dt)[0]
    P, n = rp.shape[1], len(c.pos)
    kw = {"static_capacity": P + 37} if form == "static" else {}
    pos, _, _ = _inputs(c)
    pos.requires_grad_(True)
    g = _graph(c, "cell", pos=pos, **kw)
    assert not g.sorted_rows and g.symmetric
    if form == "static":
        assert g.n_edges == P + 37 and not g.overflow.item() and int(g.num_pairs_dev.item()) == P
        assert (g.src[P:] == -1).all() and (g.transpose[P:] == -1).all()
    else:
        assert g.n_edges == P == g.num_pairs
    _check_list(c, torch.stack([g.src, g.dst]), g.deltas.detach(), g.distances.detach(),
                g.num_pairs_dev if form == "static" else torch.tensor([g.num_pairs]), g.row_ptr)
    src, dst, T = g.src[:P].long(), g.dst[:P].long(), g.transpose[:P].long()
    assert (T >= 0).all() and (T < P).all()
    assert torch.equal(src[T], dst) and torch.equal(dst[T], src)
    dl = g.deltas.detach()[:P]
    assert torch.equal(dl[T], -dl)  # round() is odd-symmetric: the reversed edge's delta is the exact negation
    # pair numbering (tmdnet_pair_index over the unsorted rows): each pair once, both directions on one row
    pr, pe = kernels.pair_index(g)
    npairs = (P + n) // 2
    prl, pel = pr[:P].long(), pe[:npairs].long()
    assert int(prl.min()) == 0 and int(prl.max()) == npairs - 1 and torch.equal(prl[T], prl)
    assert torch.equal(torch.bincount(prl, minlength=npairs), torch.where(g.src[pel] == g.dst[pel], 1, 2))
    canon = pel[prl]
    e = torch.arange(P, device=DEV)
    assert ((canon == e) | (canon == T)).all()
    # gradient against the brute graph's
    (gp,) = torch.autograd.grad(_functional(g, n, pos.dtype), pos)
    pos_b = pos.detach().clone().requires_grad_(True)
    gb = _graph(c, "brute", pos=pos_b, **kw)
    (gref,) = torch.autograd.grad(_functional(gb, n, pos.dtype), pos_b)
    err = float((gp - gref).abs().max() / gref.abs().max())
    print(f"{name} {form} {dt}: gradient rel err {err:.3e}")
    assert err < GRAD_TOL[dt], err


@pytest.mark.parametrize("dt", BOTH)
def test_build_is_deterministic(dt):
    c = TC.get("face_t31", dt)
    P = TC.ref(c.name, dt)[0].shape[1]
    a = _raw(c, "cell", P + 64)
    b = _raw(c, "cell", P + 64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])


# ----------------------------------------------------------------------------- scripted OptimizedDistance
@pytest.mark.parametrize("include_transpose", [True, False])
@pytest.mark.parametrize("loop", [True, False])
def test_jit_script_cell_in_a_triclinic_box(loop, include_transpose):
    """test_torchscript.test_jit_script_compatible with a box that is triclinic (t31): the scripted
    OptimizedDistance(strategy="cell") returns the reference pairs."""
    from torchmdnet import _native
    from torchmdnet.models.utils import OptimizedDistance
    _native.load_torch_ops()
    c = TC.get("grid_mols_sorted", "f32")
    pos, batch, box = _inputs(c)
    pos.requires_grad_(True)
    rp, rd, rr = NC.reference(c.pos, c.batch, c.box, 0.0, c.cutoff, loop, include_transpose)
    nl = torch.jit.script(OptimizedDistance(cutoff_lower=0.0, loop=loop, cutoff_upper=c.cutoff,
                                            max_num_pairs=rp.shape[1], strategy="cell", box=box.to(DEV),
                                            return_vecs=True, include_transpose=include_transpose))
    neighbors, distances, vecs = nl(pos, batch)
    assert neighbors.shape == rp.shape
    got, gd, gr = _sorted_list(neighbors, vecs, distances, rp.shape[1])
    ref, rd, rr = NC.sort_edges(rp, rd, rr)
    assert np.array_equal(got, ref)
    assert np.allclose(gr, rr, atol=1e-5) and np.allclose(gd, rd, atol=1e-5)


# ----------------------------------------------------------------------------- models, end to end
N_WATER = 201


@pytest.fixture(scope="module")
def water():
    """201 atoms at water density (0.1003 / A^3) in the t31 box.  The whole box would hold 1251, so the atoms
    fill a block of it: fractional coordinates in [-0.25, 0.25) x [-0.25, 0.25) x [-0.25, 0.39), 0.16 of
    the volume (1996 A^3), straddling the a, b and c faces, each atom then moved by a random lattice vector
    (the box wraps it back).  About 27 neighbours per atom inside the block, fewer at its surface."""
    box = TC.box_of("t31")
    g = torch.Generator().manual_seed(21)
    frac = torch.rand(N_WATER, 3, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.5, 0.64]) - 0.25
    frac = frac + torch.randint(-1, 2, (N_WATER, 3), generator=g).double()
    pos = frac @ torch.tensor(box)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(N_WATER // 3)
    return z, pos, torch.zeros(N_WATER, dtype=torch.long), torch.tensor(box)


def _model(kind, precision, strategy, box):
    from torchmdnet.models.model import create_model
    kw = dict(embedding_dimension=32, num_layers=2, num_rbf=16, derivative=True, output_model="Scalar",
              precision=precision, cutoff_upper=4.0, max_num_neighbors=96)
    if kind == "equivariant-transformer":
        kw.update(num_heads=4)
    if kind == "graph-network":
        kw.update(aggr="add", max_z=10)
    torch.manual_seed(4)
    m = create_model(yaml_args(kind, **kw)).to(DEV)
    d = m.representation_model.distance  # as bench.py's water-box arm configures OptimizedDistance
    d.box = box.to(torch.float64 if precision == 64 else torch.float32)
    d.use_periodic = True
    d.strategy = strategy
    return m


def _close(a, ref, precision, what):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape and bool(torch.isfinite(a).all()), what
    err = float((a - ref).abs().max())
    print(f"{what}: max|d| = {err:.3e}, max|ref| = {float(ref.abs().max()):.3e}")
    if precision == 64:
        assert torch.allclose(a, ref, rtol=1e-9, atol=1e-9), (what, err)
    else:
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("kind", ["equivariant-transformer", "tensornet", "graph-network"])
def test_models_cell_equals_brute(kind, precision, water):
    """Energy, forces and the virial of small ET, TensorNet and graph-network models (32 channels, 2 layers,
    cutoff 4) in the t31 box: the cell-list graph against the brute one (the rows list their sources in
    another order, so sums differ in the last bits)."""
    z, pos, batch, box = water
    dt = torch.float64 if precision == 64 else torch.float32
    z, pos, batch = z.to(DEV), pos.to(dt).to(DEV), batch.to(DEV)
    out = {}
    for strategy in ("brute", "cell"):
        m = _model(kind, precision, strategy, box)
        y, f = m(z, pos.clone(), batch)
        yv, fv, w = m.energy_forces_virial(z, pos.clone(), batch)
        assert w.shape == (1, 3, 3)
        out[strategy] = (y, f, yv, fv, w)
        d = m.representation_model.distance
        npairs = int(d.last_num_pairs.item()) if torch.is_tensor(d.last_num_pairs) else d.last_num_pairs
        assert npairs is None or npairs > 5 * N_WATER  # a connected block, not isolated atoms
    for got, ref, what in zip(out["cell"], out["brute"], ("energy", "forces", "energy (virial call)",
                                                          "forces (virial call)", "virial")):
        _close(got, ref, precision, f"{kind} {precision} {what}")


def test_et_graphed_replays_eager_in_a_triclinic_box(water):
    """GraphedEnergyForces over the ET model with the cell list in t31: the captured step (static-capacity
    triclinic build inside the capture) replays the eager result, also at moved positions."""
    from torchmdnet.graphs import GraphedEnergyForces
    z, pos, batch, box = water
    z, pos, batch = z.to(DEV), pos.float().to(DEV), batch.to(DEV)
    m = _model("equivariant-transformer", 32, "cell", box)
    gm = GraphedEnergyForces(m, z, pos, batch)
    for p in (pos, pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(2)).to(DEV)):
        y0, f0 = m(z, p.clone(), batch)
        y, f = gm(p)
        gm.check_capacity()
        _close(y, y0, 32, "graphed energy")
        _close(f, f0, 32, "graphed forces")


# ----------------------------------------------------------------------------- refusals
def _native_build(pos, batch, box9, periodic, cutoff, cap):
    """tmdnet_nl_build (cell) called directly over sentinel-filled outputs: (status, outputs)."""
    from torchmdnet import _native as nat
    lib = nat.load()
    n = pos.shape[0]
    b9 = (ctypes.c_double * 9)(*box9)
    ws = torch.empty(max(int(lib.tmdnet_nl_workspace_bytes(n, nat.NL_CELL, b9, float(cutoff))), 16),
                     dtype=torch.uint8, device=DEV)
    outs = [torch.full((2, cap), -7, dtype=torch.int32, device=DEV), torch.full((cap, 3), -7.0, device=DEV),
            torch.full((cap,), -7.0, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV),
            torch.full((n + 1,), -7, dtype=torch.int32, device=DEV),
            torch.full((cap,), -7, dtype=torch.int32, device=DEV)]
    rc = lib.tmdnet_nl_build(nat.dtype_code(pos.dtype), nat.NL_CELL, nat.ptr(pos), nat.ptr(batch), n, b9,
                             int(periodic), 0.0, float(cutoff), cap, 1, 1, *[nat.ptr(o) for o in outs], 1,
                             nat.ptr(ws), int(ws.numel()), None, None, 0, None, nat.stream(pos.device))
    torch.cuda.synchronize()
    return rc, outs


def test_refusals_write_nothing():
    from torchmdnet import kernels
    c = TC.get("grid_n257", "f32")
    pos, batch, box = _inputs(c)
    # cell, not periodic, a non-diagonal box
    with pytest.raises(RuntimeError, match="to be diagonal"):
        kernels.neighbor_pairs_raw("cell", pos, batch, box, False, 0.0, c.cutoff, 4096, True, True)
    rc, outs = _native_build(pos, batch, c.box.reshape(-1).tolist(), False, c.cutoff, 4096)
    assert rc == 1  # TMDNET_BAD_ARGUMENT
    assert all(bool((o == -7).all()) for o in outs)
    # a grid past 1024 cells on an axis (t31 stretched along a: width 0.896 * 4700 / 4 = 1053 cells)
    big = c.box.copy()
    big[0, 0] = 4700.0
    assert TC.grid(big, c.cutoff)[0] > 1024
    with pytest.raises(RuntimeError, match="unsupported"):
        kernels.neighbor_pairs_raw("cell", pos, batch, torch.tensor(big), True, 0.0, c.cutoff, 4096, True, True)
    rc, outs = _native_build(pos, batch, big.reshape(-1).tolist(), True, c.cutoff, 4096)
    assert rc == 2  # TMDNET_UNSUPPORTED
    assert all(bool((o == -7).all()) for o in outs)
    # the same box through the scripted op's front end
    from torchmdnet import _native
    from torchmdnet.models.utils import OptimizedDistance
    _native.load_torch_ops()
    nl = torch.jit.script(OptimizedDistance(cutoff_lower=0.0, cutoff_upper=c.cutoff, max_num_pairs=4096,
                                            strategy="cell", box=torch.tensor(big, dtype=torch.float32),
                                            return_vecs=True))
    with pytest.raises(RuntimeError, match="unsupported"):
        nl(pos, batch)
