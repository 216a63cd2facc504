"""The device-box cell build (csrc/neighbors.hip ``k_cell_geom`` and the DEVGEOM forms of ``k_cell_assign`` /
``k_cell_pairs``): ``tmdnet_nl_build`` with the cell strategy and ``use_periodic == 2``, the box nine doubles on
the device, the grid derived there; through ``kernels.neighbor_pairs_raw`` / ``build_graph`` (``cell_bound``),
``OptimizedDistance``, ``get_neighbor_pairs`` and ``GraphedEnergyForces(..., box=, cell_margin=)``.

Yardsticks: the host-box cell build of the same box (bit for bit: the same kernels' statements over the same
values), the brute build where the grid is coarsened (tests/test_gpu_neighbor_tric.test_cell_equals_brute_bitwise's
comparison), and for the models the eager brute model with the same weights at the project's ``_close``.
Without the feature every (1, 3, 3) box with ``"cell"`` raises 'brute and shared strategies only'."""
import ctypes

import numpy as np
import pytest
import torch

import neighbor_cases as NC
import neighbor_cases_tric as TC
from test_gpu_batch_boxes import build_spy  # noqa: F401  (fixture)
from test_gpu_neighbor_tric import N_WATER, _close, _model, _sorted_list, water  # noqa: F401  (water: fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
TDT = {"f32": torch.float32, "f64": torch.float64}
BOTH = list(TC.DTYPES)
WORKSPACE_TOO_SMALL = 4  # TMDNET_WORKSPACE_TOO_SMALL

TRIC_CASES = [("tric", n) for n in TC.names() if "cell" in TC.strategies(n)]
DIAG_CASES = [("diag", n) for n in NC.names() if "cell" in NC.strategies(n) and NC.get(n, "f32").box is not None]


def _case(family, name, dt):
    mod = TC if family == "tric" else NC
    return mod.get(name, dt), mod.ref(name, dt)[0].shape[1]


def _inputs(c):
    pos = torch.tensor(c.pos, device=DEV)
    assert pos.dtype == TDT[c.dtype]
    return pos, torch.tensor(c.batch, device=DEV), torch.tensor(c.box, dtype=pos.dtype)


def _build(c, pos, batch, box, cap, strategy="cell", cell_bound=None):
    """kernels.neighbor_pairs_raw; a 3-d ``box`` goes to the device (the device-box build)."""
    from torchmdnet import kernels
    if box.dim() == 3:
        box = box.to(DEV)
    return kernels.neighbor_pairs_raw(strategy, pos, batch, box, True, c.lower, c.cutoff, cap, c.loop, c.transpose,
                                      pad_output=True, want_csr=True, cell_bound=cell_bound)


def _grid(box, cut):
    """Cells per axis as the host sizes them (cell_dims): the edge lengths of a diagonal box, else the widths."""
    b = np.asarray(box, dtype=np.float64)
    if b[1, 0] == 0 and b[2, 0] == 0 and b[2, 1] == 0:
        return tuple(NC.grid(float(b[i, i]), cut) for i in range(3))
    return TC.grid(b, cut)


def _same_outputs(a, b):
    """neighbors, deltas, distances, num_pairs, row_ptr and the transpose map."""
    assert len(a) == len(b) == 6
    differ = []
    for what, x, y in zip(("neighbors", "deltas", "distances", "num_pairs", "row_ptr", "transpose"), a, b):
        assert (x is None) == (y is None)
        if x is not None and not torch.equal(x, y):  # the figures first, then the assertion
            bad = x != y
            if x.is_floating_point():
                ulp = torch.finfo(x.dtype).eps * x.abs().clamp_min(torch.finfo(x.dtype).tiny)
                print(f"{what}: {int(bad.sum())} of {x.numel()} entries differ, "
                      f"max |d| = {float((x - y).abs().max()):.3e}, max |d| / (eps |x|) = "
                      f"{float(((x - y).abs() / ulp)[bad].max()):.2f}")
            else:
                print(f"{what}: {int(bad.sum())} of {x.numel()} entries differ")
            differ.append(what)
    assert not differ, differ


# ----------------------------------------------------------------------------- 1. device box == host box
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("family,name", TRIC_CASES + DIAG_CASES, ids=lambda v: v)
def test_device_box_is_bitwise_the_host_box_build(family, name, dt):
    """Every cell case of neighbor_cases_tric (four skewed boxes, face atoms, n = 1, 2, 257, sorted and shuffled
    molecules, loop x transpose, a lower cutoff) and every periodic cell case of neighbor_cases (diagonal boxes):
    the (1, 3, 3) device box gives the (3, 3) host box's six outputs, the workspace sized for that box both
    times.  (At the parent commit the device-box call raises.)"""
    c, P = _case(family, name, dt)
    pos, batch, box = _inputs(c)
    host = _build(c, pos, batch, box, P + 64)
    assert int(host[3].item()) == P
    dev = _build(c, pos, batch, box.reshape(1, 3, 3), P + 64, cell_bound=box)
    _same_outputs(host, dev)


# ----------------------------------------------------------------------------- 2. one workspace, a moving cell
MOVING = [("tric", "face_t31", (1.0, 0.9, 0.8)), ("tric", "grid_mols_shuffled", (1.0, 0.9, 0.8)),
          ("diag", "grid_sparse", (1.0, 0.9))]


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("family,name,factors", MOVING, ids=lambda v: str(v))
def test_one_workspace_follows_a_shrinking_cell(family, name, factors, dt):
    """The workspace sized for the case's box; builds at that box and the positions scaled by ``factors``.  On the
    CPU first: one of the grids is the bound's own and, on every axis that can lose a cell (more than 3), one
    grid has exactly one cell less.  Each build equals the host build at its box bit for bit.  (An axis whose bound
    is 3 cells cannot lose one: in the diagonal ``grid_sparse`` case and on the c axis of t31 at 0.8 the count only
    changes on the axes above 3; an axis already at 3 is never seen with a changing count.)

    The face case in float32 at 0.9 and 0.8 is the sharp one: the scaled box entries fill the mantissa and the probe
    atoms sit 3 and more box lengths apart, so the image's products ``round(k) * c`` are inexact, and a kernel that
    fuses another one of ``Tric::apply``'s multiply-subtract pairs than the host-box kernel does differs in the last
    bit of a coordinate near 100 A (csrc/neighbors.hip ``cell_pairs_outlined`` is there for this case)."""
    c, P = _case(family, name, dt)
    pos, batch, box = _inputs(c)
    boxes = [box * f for f in factors]  # in the dtype, as the builds get them
    bound = _grid(box.numpy(), c.cutoff)
    grids = [_grid(b.numpy(), c.cutoff) for b in boxes]
    assert bound in grids
    for ax in range(3):
        if bound[ax] > 3:
            assert any(g[ax] == bound[ax] - 1 for g in grids), (ax, grids)
    assert any(g != bound for g in grids)
    cap = 4 * P + 256  # the shrunk cell is denser: the largest factor^-3 is below 2
    failed = []
    for f, b in zip(factors, boxes):
        p = (pos * f).contiguous()
        assert float(torch.diagonal(b).min()) >= 2 * c.cutoff
        host = _build(c, p, batch, b, cap)
        assert int(host[3].item()) <= cap
        dev = _build(c, p, batch, b.reshape(1, 3, 3), cap, cell_bound=box)
        try:  # every factor's figures before the verdict
            _same_outputs(host, dev)
        except AssertionError as e:
            print(f"{name} {dt} factor {f}: {e}")
            failed.append((f, str(e)))
    assert not failed, failed


# ----------------------------------------------------------------------------- 3. coarsened grid
def _coarse_bounds(c):
    """(bound, its grid) pairs with fewer cells than the box's own grid: the box shrunk to 0.8, and 3 cutoffs
    cubed -- room for exactly 27 cells."""
    out = []
    for b in (c.box * 0.8, np.eye(3) * 3 * c.cutoff):
        out.append((torch.tensor(b), _grid(b, c.cutoff)))
    return out


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name", ["face_t31", "face_tmax"])
def test_coarsened_grid_equals_brute_bitwise(name, dt):
    """A workspace with room for fewer cells than the box's grid: the build takes cells off its largest axes until
    it fits.  The cells stay at least a cutoff thick, so the list is brute's: equal pair sets and, after sorting
    the edges, bitwise brute's deltas and distances."""
    c = TC.get(name, dt)
    P = TC.ref(name, dt)[0].shape[1]
    pos, batch, box = _inputs(c)
    own = _grid(c.box, c.cutoff)
    brute = _build(c, pos, batch, box, P + 64, strategy="brute")
    assert int(brute[3].item()) == P
    bp, bd, br = _sorted_list(brute[0], brute[1], brute[2], P)
    bounds = _coarse_bounds(c)
    assert bounds[1][1] == (3, 3, 3)
    for bound, g in bounds:
        assert g[0] * g[1] * g[2] < own[0] * own[1] * own[2], (g, own)
        cell = _build(c, pos, batch, box.reshape(1, 3, 3), P + 64, cell_bound=bound)
        assert int(cell[3].item()) == P
        assert (cell[0][:, P:] == -1).all()
        cp, cd, cr = _sorted_list(cell[0], cell[1], cell[2], P)
        assert np.array_equal(cp, bp)
        assert np.array_equal(cd, bd) and np.array_equal(cr, br)
        t = cell[5][:P].long()
        assert (t >= 0).all() and torch.equal(cell[0][0, :P][t], cell[0][1, :P])


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("name", ["face_b31_n0", "grid_sparse"])
def test_coarsened_rectangular_grid_keeps_the_list(name, dt):
    """A diagonal box with room for fewer cells than its grid.  The rectangular binning keeps cells one cutoff wide
    (``cell_axis`` divides by the cutoff, not by L / n): on a coarsened axis every atom past cell n - 1 folds into
    cell 0, which cells 0 and n - 1 both scan, so the list stays exact while cell 0 grows.  Yardsticks: the
    reference pair set exactly, and the host-box cell build (same ``rect_apply``) after sorting the edges, deltas
    and distances bit for bit."""
    c, P = _case("diag", name, dt)
    pos, batch, box = _inputs(c)
    own = _grid(c.box, c.cutoff)
    host = _build(c, pos, batch, box, P + 64)
    assert int(host[3].item()) == P
    hp, hd, hr = _sorted_list(host[0], host[1], host[2], P)
    ref = NC.sort_edges(NC.ref(name, dt)[0])[0]
    assert np.array_equal(hp, ref)
    for bound, g in _coarse_bounds(c):
        assert g[0] * g[1] * g[2] < own[0] * own[1] * own[2], (g, own)
        cell = _build(c, pos, batch, box.reshape(1, 3, 3), P + 64, cell_bound=bound)
        assert int(cell[3].item()) == P and (cell[0][:, P:] == -1).all()
        cp, cd, cr = _sorted_list(cell[0], cell[1], cell[2], P)
        assert np.array_equal(cp, ref)
        assert np.array_equal(cd, hd) and np.array_equal(cr, hr)
        t = cell[5][:P].long()
        assert (t >= 0).all() and torch.equal(cell[0][0, :P][t], cell[0][1, :P])


# ----------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("dt", BOTH)
def test_device_box_build_is_deterministic(dt):
    c, P = _case("tric", "face_t31", dt)
    pos, batch, box = _inputs(c)
    a = _build(c, pos, batch, box.reshape(1, 3, 3), P + 64, cell_bound=box)
    b = _build(c, pos, batch, box.reshape(1, 3, 3), P + 64, cell_bound=box)
    _same_outputs(a, b)


# ----------------------------------------------------------------------------- 5. refusals
def test_a_workspace_below_27_cells_is_refused_with_nothing_written():
    """tmdnet_nl_build itself over sentinel-filled outputs: the workspace of a 3 x 3 x 3 bound is taken; the same
    workspace less one cell (one cstart and one cend entry) is TMDNET_WORKSPACE_TOO_SMALL and writes nothing."""
    from torchmdnet import _native as nat
    lib = nat.load()
    c, P = _case("tric", "grid_n257", "f32")
    pos, batch, box = _inputs(c)
    n, cap = pos.shape[0], P + 64
    dbox = box.double().reshape(1, 3, 3).to(DEV).contiguous()
    b27 = (ctypes.c_double * 9)(*(np.eye(3) * 3 * c.cutoff).reshape(-1).tolist())
    full = int(lib.tmdnet_nl_workspace_bytes(n, nat.NL_CELL, b27, c.cutoff))

    def call(ws_bytes):
        ws = torch.empty(full, dtype=torch.uint8, device=DEV)
        outs = [torch.full((2, cap), -7, dtype=torch.int32, device=DEV), torch.full((cap, 3), -7.0, device=DEV),
                torch.full((cap,), -7.0, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV),
                torch.full((n + 1,), -7, dtype=torch.int32, device=DEV),
                torch.full((cap,), -7, dtype=torch.int32, device=DEV)]
        rc = lib.tmdnet_nl_build(nat.F32, nat.NL_CELL, nat.ptr(pos), nat.ptr(batch), n, nat.ptr(dbox), 2, 0.0,
                                 c.cutoff, cap, 1, 1, *[nat.ptr(o) for o in outs], 1, nat.ptr(ws), ws_bytes, None,
                                 None, 0, None, nat.stream(pos.device))
        torch.cuda.synchronize()
        return rc, outs

    rc, outs = call(full - 2 * 4)
    assert rc == WORKSPACE_TOO_SMALL
    assert all(bool((o == -7).all()) for o in outs)
    rc, outs = call(full)
    assert rc == 0 and int(outs[3].item()) == P


def test_static_capacity_without_a_bound_launches_nothing(build_spy):  # noqa: F811
    from torchmdnet import kernels
    c, P = _case("tric", "grid_n257", "f32")
    pos, batch, box = _inputs(c)
    dbox = box.reshape(1, 3, 3).to(DEV)
    with pytest.raises(RuntimeError, match="cell_bound"):
        kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=dbox, static_capacity=P + 64)
    with pytest.raises(RuntimeError, match="brute and shared"):
        kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=dbox.expand(2, 3, 3).contiguous(),
                            static_capacity=P + 64, cell_bound=box)
    assert build_spy == []
    g = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=dbox, static_capacity=P + 64,
                            cell_bound=box)
    assert len(build_spy) == 1 and build_spy[0][6] == 2  # use_periodic = one device box
    assert not g.sorted_rows and not g.overflow.item() and int(g.num_pairs_dev.item()) == P
    # eager, no bound: sized for the box read back with its checks; the host-box graph's edges
    e = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=dbox)
    h = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=box)
    assert e.num_pairs == h.num_pairs == P and not e.sorted_rows
    assert torch.equal(e.src, h.src) and torch.equal(e.deltas.detach(), h.deltas.detach())
    assert torch.equal(e.transpose, h.transpose)
    short = dbox.clone()
    short[0, 2, 2] = 2 * c.cutoff - 0.5
    with pytest.raises(RuntimeError, match=r"molecule 0: Invalid box vectors: box_vectors\[2\]\[2\] < 2\*cutoff"):
        kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, strategy="cell", box=short)


# ----------------------------------------------------------------------------- 6. models, end to end
DIAG_BOX = torch.diag(torch.tensor([31.0, 23.0, 17.5], dtype=torch.float64))


@pytest.fixture(scope="module")
def water_diag():
    """The ``water`` block of test_gpu_neighbor_tric.py laid out in the diagonal (31, 23, 17.5) box."""
    g = torch.Generator().manual_seed(21)
    frac = torch.rand(N_WATER, 3, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.5, 0.64]) - 0.25
    frac = frac + torch.randint(-1, 2, (N_WATER, 3), generator=g).double()
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(N_WATER // 3)
    return z, frac @ DIAG_BOX, torch.zeros(N_WATER, dtype=torch.long), DIAG_BOX


def _captured_follows_eager(kind, precision, data):
    from torchmdnet.graphs import GraphedEnergyForces
    z, pos, batch, box = data
    dt = torch.float64 if precision == 64 else torch.float32
    z, pos, batch, box = z.to(DEV), pos.to(dt).to(DEV), batch.to(DEV), box.to(DEV)
    m_cell = _model(kind, precision, "cell", box.cpu())
    m_brute = _model(kind, precision, "brute", box.cpu())
    gm = GraphedEnergyForces(m_cell, z, pos, batch, box=box, virial=True)
    try:
        d = m_cell.representation_model.distance
        assert gm.box.shape == (1, 3, 3) and gm.box.dtype == torch.float64
        assert torch.equal(d.cell_bound, box.cpu().double() * 1.25)
        # the last of them lies beyond cell_margin: the captured build coarsens its grid
        for s in (1.0, 1.04, 0.96, 1.0, 1.3):
            p, b = pos * s, box * s
            y_e, f_e, w_e = m_brute.energy_forces_virial(z, p.clone(), batch, box=b)
            y, f = gm(p, box=b)
            gm.check_capacity()
            _close(y, y_e, precision, f"{kind} x{s} captured y")
            _close(f, f_e, precision, f"{kind} x{s} captured forces")
            _close(gm.virial, w_e, precision, f"{kind} x{s} captured virial")
    finally:
        gm.release()
    assert d.cell_bound is None and d.static_capacity is None


@pytest.mark.parametrize("kind,precision", [("equivariant-transformer", 32), ("tensornet", 32),
                                            ("equivariant-transformer", 64)])
def test_captured_cell_list_follows_a_changing_cell(kind, precision, water):  # noqa: F811
    """GraphedEnergyForces over a ``strategy="cell"`` model with ``box=`` (201 atoms, t31, cutoff 4, 32 channels, 2
    layers): replays at the cell, 1.04 and 0.96 of it, the first again and 1.3 of it against the eager brute model
    with the same weights."""
    _captured_follows_eager(kind, precision, water)


def test_captured_cell_list_in_a_diagonal_box(water_diag):
    _captured_follows_eager("equivariant-transformer", 32, water_diag)


def test_a_failed_construction_leaves_no_bound_behind(water):  # noqa: F811
    """GraphedEnergyForces raises in its warm-up (a box shorter than two cutoffs): no object, so no release(); the
    distance module must not keep the cell_bound set before the warm-up."""
    from torchmdnet.graphs import GraphedEnergyForces
    z, pos, batch, box = water
    m = _model("equivariant-transformer", 32, "cell", box)
    short = box.clone()
    short[2, 2] = 7.0
    with pytest.raises(RuntimeError, match=r"box_vectors\[2\]\[2\] < 2\*cutoff"):
        GraphedEnergyForces(m, z.to(DEV), pos.float().to(DEV), batch.to(DEV), box=short.to(DEV))
    d = m.representation_model.distance
    assert d.cell_bound is None and d.static_capacity is None


# ----------------------------------------------------------------------------- 7. the operator
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("family,name", [("tric", "grid_mols_sorted"), ("diag", "grid_n257")])
def test_get_neighbor_pairs_takes_one_device_box(family, name, dt):
    from torchmdnet.models.utils import OptimizedDistance
    from torchmdnet.neighbors import get_neighbor_pairs_kernel
    c, P = _case(family, name, dt)
    pos, batch, box = _inputs(c)
    dbox = box.reshape(1, 3, 3).to(DEV)
    host = get_neighbor_pairs_kernel("cell", pos, batch, box, True, 0.0, c.cutoff, P + 64, True, True)
    dev = get_neighbor_pairs_kernel("cell", pos, batch, dbox, True, 0.0, c.cutoff, P + 64, True, True)
    assert int(host[3].item()) == P
    for a, b in zip(host, dev):
        assert torch.equal(a, b)
    od = OptimizedDistance(0.0, c.cutoff, max_num_pairs=P + 64, return_vecs=True, loop=True, strategy="cell")
    ei, ew, ev = od(pos, batch, dbox)
    assert ei.shape == (2, P) and torch.equal(ei, host[0][:, :P].long()) and torch.equal(ew, host[2][:P])
    g = od.graph(pos, batch, dbox)
    assert g.num_pairs == P and torch.equal(g.src, host[0][0, :P])
