"""Per-molecule periodic boxes on the GPU: the brute / shared build with ``use_periodic = n_boxes + 1``
(csrc/neighbors.hip ``k_pairs<.., MOLBOX>``), ``box=`` through ``OptimizedDistance``, the three models,
``energy_forces_virial``, ``LNNPStep``, ``GraphedEnergyForces`` and ``get_neighbor_pairs``.

Yardstick: tests/batch_box_ref.py (``neighbor_cases.reference`` once per molecule with its own box), checked on the
CPU by tests/test_batch_boxes_cpu.py; the models against the same weights evaluated one molecule at a time through the
single-box route (``distance.box = box_m``), which this feature leaves as it was.

Tolerances are the project's: builds at tests/test_gpu_neighbor_edges.TOL (pair sets exactly); model quantities at
tests/test_gpu_gn._close (float64 rtol = atol = 1e-9; float32 max|d| <= 1e-4 max|ref|); the strain difference with
tests/test_virial_cpu.py's step and gate (h = 1e-5, 1e-8 of the largest virial entry).

TensorNet runs with ``static_shapes = False`` here: with the padding semantics the energy of atom 0 depends on the
unused capacity of the whole batch's list, so a batch and its molecules evaluated alone differ by construction.
"""
import contextlib
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import batch_box_ref as BB
import neighbor_cases as NC
from conftest import yaml_args
from test_gpu_neighbor_edges import TDT, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOTH = list(NC.DTYPES)
ROWS = ["brute", "shared"]
BAD_ARGUMENT = 1  # TMDNET_BAD_ARGUMENT


# ----------------------------------------------------------------------------- build helpers
def _inputs(c):
    pos = torch.tensor(c.pos, device=DEV)
    assert pos.dtype == TDT[c.dtype]
    return pos, torch.tensor(c.batch, device=DEV), torch.tensor(c.boxes, device=DEV)


def _raw(strategy, pos, batch, box, cutoff, cap, loop=True, transpose=True):
    from torchmdnet import kernels
    return kernels.neighbor_pairs_raw(strategy, pos, batch, box, True, 0.0, cutoff, cap, loop, transpose,
                                      pad_output=True, want_csr=True)


def _check_against_yardstick(c, out, loop, transpose):
    """Pair set == yardstick exactly (and in its order: destination-major, sources ascending); row pointer; deltas and
    distances within TOL; padding; with the transpose map, deltas[T] == -deltas bit for bit."""
    nb, dl, dist, num, row_ptr, T = out
    rp, rd, rr = BB.ref(c.name, c.dtype, loop, transpose)
    P, n, tol = rp.shape[1], len(c.pos), TOL[c.dtype]
    assert int(num.item()) == P
    assert (nb[:, P:] == -1).all() and (dl[P:] == 0).all() and (dist[P:] == 0).all()
    got = nb[:, :P].cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < n
    got, gd, gr = NC.sort_edges(got, dl[:P].cpu().numpy(), dist[:P].cpu().numpy())
    assert np.array_equal(got, rp)
    assert np.allclose(gd, rd, rtol=tol, atol=tol), np.abs(gd - rd).max()
    assert np.allclose(gr, rr, rtol=tol, atol=tol), np.abs(gr - rr).max()
    assert np.array_equal(row_ptr.cpu().numpy(), NC.row_ptr_of(rp, n))
    assert (nb[1, :P].cpu().numpy() == np.repeat(np.arange(n), np.diff(NC.row_ptr_of(rp, n)))).all()
    if transpose:
        t = T[:P].long()
        assert (t >= 0).all() and (T[P:] == -1).all()
        assert torch.equal(nb[0, :P][t], nb[1, :P]) and torch.equal(nb[1, :P][t], nb[0, :P])
        assert torch.equal(dl[:P][t], -dl[:P])
    else:
        assert T is None
        assert (nb[0, :P] >= nb[1, :P]).all()
    return P


# ----------------------------------------------------------------------------- 1. build against the yardstick
@pytest.mark.parametrize("transpose", [True, False], ids=["full", "half"])
@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_build_against_yardstick(strategy, dt, loop, transpose):
    c = BB.get("main", dt)
    pos, batch, boxes = _inputs(c)
    P = BB.ref("main", dt, loop, transpose)[0].shape[1]
    out = _raw(strategy, pos, batch, boxes, c.cutoff, P + 64, loop, transpose)
    _check_against_yardstick(c, out, loop, transpose)


# ----------------------------------------------------------------------------- 2. bitwise agreement
def _same_outputs(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_equal_boxes_are_bitwise_the_single_box_build(strategy, dt):
    """A (4, 3, 3) stack of one box: neighbors, deltas, distances, num_pairs, row_ptr and the transpose map are
    ``torch.equal`` to the (3, 3) call's (which takes the host-box route)."""
    c = BB.get("main", dt)
    pos, batch, boxes = _inputs(c)
    for k in (2, 0):
        one = torch.tensor(BB.BOXES[k], dtype=pos.dtype)  # host, as OptimizedDistance holds it
        single = _raw(strategy, pos, batch, one, c.cutoff, 8192)
        stacked = _raw(strategy, pos, batch, boxes[k].expand(4, 3, 3).contiguous(), c.cutoff, 8192)
        assert 300 < int(single[3].item()) < 8192
        _same_outputs(single, stacked)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_each_molecule_is_bitwise_its_own_single_box_build(strategy, dt):
    """The four different boxes: molecule m's rows are those of a single-box build of molecule m alone, bit for
    bit, once the atom and edge offsets are taken off."""
    c = BB.get("main", dt)
    pos, batch, boxes = _inputs(c)
    nb, dl, dist, num, row_ptr, T = _raw(strategy, pos, batch, boxes, c.cutoff, 8192)
    a0 = 0
    for m, n in enumerate(c.sizes):
        alone = torch.zeros(n, dtype=torch.long, device=DEV)
        s_nb, s_dl, s_dist, s_num, s_rp, s_T = _raw(strategy, pos[a0:a0 + n].contiguous(), alone,
                                                     torch.tensor(BB.BOXES[m], dtype=pos.dtype), c.cutoff, 8192)
        E = int(s_num.item())
        e0 = int(row_ptr[a0].item())
        assert int(row_ptr[a0 + n].item()) - e0 == E
        assert torch.equal(row_ptr[a0:a0 + n + 1] - e0, s_rp)
        assert torch.equal(nb[:, e0:e0 + E] - a0, s_nb[:, :E])
        assert torch.equal(dl[e0:e0 + E], s_dl[:E]) and torch.equal(dist[e0:e0 + E], s_dist[:E])
        assert torch.equal(T[e0:e0 + E] - e0, s_T[:E])
        a0 += n
    assert int(num.item()) == int(row_ptr[-1].item())


# ----------------------------------------------------------------------------- 3. unsorted batch
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_interleaved_batch_over_two_boxes(strategy, dt):
    """Atoms of two molecules alternating (every k_segments block sees a descent: all atoms are candidates): each
    destination still takes its own molecule's box."""
    c = BB.get("interleaved", dt)
    pos, batch, boxes = _inputs(c)
    P = BB.ref("interleaved", dt)[0].shape[1]
    out = _raw(strategy, pos, batch, boxes, c.cutoff, P + 64)
    _check_against_yardstick(c, out, True, True)
    from torchmdnet import kernels
    g = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, loop=True, strategy=strategy, box=boxes)
    assert g.symmetric and g.num_pairs == P
    assert torch.equal(g.src, out[0][0, :P]) and torch.equal(g.deltas.detach(), out[1][:P])


# ----------------------------------------------------------------------------- 4. refusals and bounds
@pytest.fixture
def build_spy(monkeypatch):
    """Counts the calls that reach tmdnet_nl_build through the Python hub."""
    from torchmdnet import _native as nat
    lib = nat.load()
    real = lib.tmdnet_nl_build
    calls = []

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "tmdnet_nl_build", spy)
    return calls


def test_refusals_launch_nothing(build_spy):
    from torchmdnet import kernels
    from torchmdnet.neighbors import get_neighbor_pairs_kernel
    c = BB.get("main", "f32")
    pos, batch, boxes = _inputs(c)
    graph = lambda **kw: kernels.build_graph(pos, batch, 0.0, c.cutoff, 8192, **kw)
    op = lambda strategy, bx: get_neighbor_pairs_kernel(strategy, pos, batch, bx, True, 0.0, c.cutoff, 8192, True, True)
    # the cell strategy
    with pytest.raises(RuntimeError, match="brute and shared"):
        graph(strategy="cell", box=boxes)
    with pytest.raises(RuntimeError, match="brute and shared"):
        _raw("cell", pos, batch, boxes, c.cutoff, 8192)
    with pytest.raises(RuntimeError, match="brute and shared"):
        op("cell", boxes)
    # fewer boxes than molecules
    with pytest.raises(RuntimeError, match="3 boxes.*molecule 3"):
        graph(box=boxes[:3].contiguous())
    with pytest.raises(RuntimeError, match="3 boxes.*molecule 3"):
        op("brute", boxes[:3].contiguous())
    # a box shorter than 2 * cutoff, named by its molecule
    short = boxes.clone()
    short[1, 1, 1] = 5.9
    with pytest.raises(RuntimeError, match=r"molecule 1: Invalid box vectors: box_vectors\[1\]\[1\] < 2\*cutoff"):
        graph(box=short)
    with pytest.raises(RuntimeError, match=r"molecule 1: Invalid box vectors: box_vectors\[1\]\[1\] < 2\*cutoff"):
        op("shared", short)
    # boxes on the host
    with pytest.raises(RuntimeError, match="on the device"):
        graph(box=boxes.cpu())
    assert build_spy == []
    graph(box=boxes)
    assert len(build_spy) == 1 and build_spy[0][6] == 5  # use_periodic = n_boxes + 1


def test_native_refusals_leave_the_outputs_alone():
    """tmdnet_nl_build itself: use_periodic >= 2 with a NULL box is bad-argument, with the cell strategy unsupported;
    neither writes an output.  A batch value outside the boxes is clamped to the last (first) box."""
    from torchmdnet import _native as nat
    lib = nat.load()
    c = BB.get("main", "f64")
    pos, batch, boxes = _inputs(c)
    n, cap = pos.shape[0], 4096
    ws = torch.empty(max(int(lib.tmdnet_nl_workspace_bytes(n, nat.NL_CELL, None, c.cutoff)), 1 << 20),
                     dtype=torch.uint8, device=DEV)

    def call(strategy, box_ptr, code, bt=batch):
        nb = torch.full((2, cap), 77, dtype=torch.int32, device=DEV)
        dl = torch.full((cap, 3), 7.0, dtype=pos.dtype, device=DEV)
        dist = torch.full((cap,), 7.0, dtype=pos.dtype, device=DEV)
        num = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        rp = torch.full((n + 1,), 77, dtype=torch.int32, device=DEV)
        tr = torch.full((cap,), 77, dtype=torch.int32, device=DEV)
        rc = lib.tmdnet_nl_build(nat.F64, strategy, nat.ptr(pos), nat.ptr(bt), n, box_ptr, code, 0.0, c.cutoff, cap,
                                 1, 1, nat.ptr(nb), nat.ptr(dl), nat.ptr(dist), nat.ptr(num), nat.ptr(rp), nat.ptr(tr),
                                 1, nat.ptr(ws), ws.numel(), None, None, 0, None, nat.stream(pos.device))
        torch.cuda.synchronize()
        return rc, (nb, dl, dist, num, rp, tr)

    def untouched(out):
        nb, dl, dist, num, rp, tr = out
        return all(bool((t == 77).all()) for t in (nb, num, rp, tr)) and all(bool((t == 7.0).all()) for t in (dl, dist))

    for strategy in (nat.NL_BRUTE, nat.NL_SHARED, nat.NL_CELL):
        rc, out = call(strategy, None, 5)
        assert rc == BAD_ARGUMENT and untouched(out)
    rc, out = call(nat.NL_CELL, nat.ptr(boxes), 5)
    assert rc == nat.UNSUPPORTED and untouched(out)
    # the molecule index is clamped to [0, n_boxes - 1]: batch values 3 -> 900 and 0 -> -5 build the same list
    rc, ref = call(nat.NL_BRUTE, nat.ptr(boxes), 5)
    assert rc == 0
    far = batch.clone()
    far[far == 3] = 900
    far[far == 0] = -5  # still ascending (-5 < 1 < 2 < 900): the same candidate segments
    rc, out = call(nat.NL_BRUTE, nat.ptr(boxes), 5, far)
    assert rc == 0
    _same_outputs(ref, out)


# ----------------------------------------------------------------------------- models
SIZES3 = (20, 9, 14)


def _model_args(kind, precision):
    common = dict(embedding_dimension=32, num_layers=2, num_rbf=16, max_num_neighbors=64, cutoff_upper=BB.CUTOFF,
                  derivative=True, output_model="Scalar", precision=precision, max_z=10)
    if kind == "et":
        return yaml_args("equivariant-transformer", num_heads=4, **common)
    if kind == "tn":
        return yaml_args("tensornet", **common)
    return yaml_args("graph-network", aggr="add", **common)


def _model(kind, precision, seed=11):
    from torchmdnet.models.model import create_model
    torch.manual_seed(seed)
    m = create_model(_model_args(kind, precision))
    if kind == "tn":
        m.representation_model.static_shapes = False
        m.representation_model.distance.resize_to_fit = True
    return m.to(DEV)


_BATCH3 = {}
MIN_DISTANCE = 1.0


def _spaced_molecule(n, box, rng):
    """``batch_box_ref._molecule`` redrawn until no two atoms (minimum image) are closer than MIN_DISTANCE, as in
    a physical structure.  The strain test differentiates the energy numerically: the truncation error of its
    central difference, h^2 E''' / 6, grows with the third derivative, which overlapping atoms (the steep end of
    the exponential basis) make orders of magnitude larger than any structure the models are used on.  (Measured
    on MI355X: with unconstrained uniform positions the ET difference quotient of the 14-atom molecule stood
    1.26e-8 of the largest entry from the virial, its other two molecules below 1e-8 (TensorNet and the graph
    network were not run on that input); with spaced atoms all nine cases lie between 1.5e-10 and 1.1e-9, the
    level tests/test_virial_cpu.py reports for the oracle's fixtures.)"""
    for _ in range(1000):
        pos = BB._molecule(n, box, rng)
        close = NC.reference(pos, np.zeros(n, dtype=np.int64), box, 0.0, MIN_DISTANCE, loop=False)[0]
        if close.shape[1] == 0:
            return pos
    raise AssertionError("no spaced molecule drawn")


def _batch3(dtype):
    """Three molecules of 20, 9 and 14 atoms in the cubic, the orthorhombic and the triclinic box (a third of the
    atoms in other images, no two atoms within MIN_DISTANCE), float64 master copy rounded to ``dtype``.  Shared:
    treat as read-only."""
    if dtype not in _BATCH3:
        rng = np.random.default_rng(5)
        pos = np.concatenate([_spaced_molecule(n, BB.BOXES[m], rng) for m, n in enumerate(SIZES3)])
        z = torch.tensor(rng.choice([1, 6, 7, 8], sum(SIZES3)), dtype=torch.long)
        batch = torch.repeat_interleave(torch.arange(3), torch.tensor(SIZES3))
        _BATCH3[dtype] = (z.to(DEV), torch.tensor(pos).to(dtype).to(DEV), batch.to(DEV),
                          torch.tensor(BB.BOXES[:3]).to(DEV))
    return _BATCH3[dtype]


@contextlib.contextmanager
def _own_box(model, box):
    """The route that exists without this feature: the distance module's one host box."""
    d = model.representation_model.distance
    old = (d.box, d.use_periodic)
    d.box, d.use_periodic = box.detach().cpu(), True
    try:
        yield
    finally:
        d.box, d.use_periodic = old


def _alone(model, z, pos, batch, boxes, m, **kw):
    """Molecule m evaluated alone through the single-box route: (y [1, 1], neg_dy [n_m, 3], virial [1, 3, 3])."""
    idx = (batch == m).nonzero().flatten()
    with _own_box(model, boxes[m]):
        return model.energy_forces_virial(z[idx], pos[idx].clone(), torch.zeros_like(idx), **kw)


def _close(a, ref, dtype, what):  # tests/test_gpu_virial._close
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert a.shape == ref.shape, what
    assert bool(torch.isfinite(a).all()), what
    err = float((a - ref).abs().max())
    print(f"{what}: max|d| = {err:.3e}, max|ref| = {float(ref.abs().max()):.3e}")
    if dtype == torch.float64:
        assert torch.allclose(a, ref, rtol=1e-9, atol=1e-9), (what, err)
    else:
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)


# ----------------------------------------------------------------------------- 5. models
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("kind", ["et", "tn", "gn"])
def test_models_match_their_molecules_alone(kind, precision):
    """y, forces and the virial of energy_forces_virial(..., box=boxes) equal, molecule by molecule, the same weights
    on that molecule alone with ``distance.box = box_m``.  (Without the feature ``box=`` is a TypeError.)"""
    dtype = torch.float64 if precision == 64 else torch.float32
    model = _model(kind, precision)
    z, pos, batch, boxes = _batch3(dtype)
    y, f, w = model.energy_forces_virial(z, pos.clone(), batch, box=boxes)
    assert y.shape == (3, 1) and w.shape == (3, 3, 3) and w.dtype == dtype
    ref = [_alone(model, z, pos, batch, boxes, m) for m in range(3)]
    _close(y, torch.cat([r[0] for r in ref]), dtype, f"{kind} y")
    _close(f, torch.cat([r[1] for r in ref]), dtype, f"{kind} forces")
    _close(w, torch.cat([r[2] for r in ref]), dtype, f"{kind} virial")
    # forward alone takes the box too, and a (3, 3) box passed per call is the constructor's route
    y1, f1 = model(z, pos.clone(), batch, box=boxes)
    _close(y1, y, dtype, f"{kind} forward y")
    _close(f1, f, dtype, f"{kind} forward forces")
    idx = (batch == 2).nonzero().flatten()
    y2, f2 = model(z[idx], pos[idx].clone(), torch.zeros_like(idx), box=boxes[2].cpu())
    _close(y2, ref[2][0], dtype, f"{kind} (3, 3) per call y")
    _close(f2, ref[2][1], dtype, f"{kind} (3, 3) per call forces")
    # the periodic images matter: without a box the energies are others
    y0, _ = model(z, pos.clone(), batch)
    assert float((y0 - y).detach().abs().max()) > 1e-3 * float(y.detach().abs().max())


# ----------------------------------------------------------------------------- 6. virial against a strain difference
def _reduced(box, pos):
    """Rotate a strained cell back to the reduced form (a along x, b in the xy plane): box -> box Q, pos -> pos Q
    with Q orthogonal.  The energy does not change under a rotation."""
    q, r = torch.linalg.qr(box.T.cpu())
    sgn = torch.sign(torch.diagonal(r))
    q = (q * sgn).to(box.device)
    red = box @ q
    red = torch.tril(red)  # the entries above the diagonal are rounding noise of the factorisation
    return red, pos @ q


@pytest.mark.parametrize("kind", ["et", "tn", "gn"])
def test_virial_is_the_strain_derivative_of_its_own_molecule(kind):
    """float64: molecule m's positions and ITS box strained together, pos -> pos (I + eps)^T, box -> box (I + eps)^T
    (rotated back to the reduced form the build takes), central differences of E_m with h = 1e-5 over all nine
    entries: -dE_m/d eps = virial[m] within 1e-8 of the largest entry (tests/test_virial_cpu.py's step and gate).
    The other molecules' energies do not move (up to the order of the energy reduction's atomic adds, N eps |y|:
    tests/test_gpu_virial._same_call)."""
    model = _model(kind, 64)
    z, pos, batch, boxes = _batch3(torch.float64)
    y0, _, w = model.energy_forces_virial(z, pos.clone(), batch, box=boxes)
    y0 = y0.detach()
    h = 1e-5
    noise = pos.shape[0] * torch.finfo(torch.float64).eps * float(y0.abs().max())
    errs = []
    for m in range(3):
        idx = (batch == m).nonzero().flatten()
        others = [k for k in range(3) if k != m]
        fd = torch.zeros(3, 3, dtype=torch.float64)
        for a, b in itertools.product(range(3), range(3)):
            e = []
            for sgn in (1.0, -1.0):
                s = torch.eye(3, dtype=torch.float64, device=DEV)
                s[a, b] += sgn * h
                bx, p = boxes.clone(), pos.clone()
                bx[m], p[idx] = _reduced(boxes[m] @ s.T, pos[idx] @ s.T)
                y, _ = model(z, p, batch, box=bx)
                y = y.detach()
                assert float((y[others] - y0[others]).abs().max()) <= noise
                e.append(y[m, 0])
            fd[a, b] = float(e[0] - e[1]) / (2 * h)
        err = float((w[m].cpu() + fd).abs().max() / w[m].abs().max())
        print(f"{kind} molecule {m}: max |W + dE/d eps (FD)| / max|W| = {err:.3e}")
        errs.append(err)
    assert max(errs) < 1e-8, errs


# ----------------------------------------------------------------------------- 7. stress training
@pytest.mark.parametrize("kind", ["et", "tn", "gn"])
def test_stress_training_loss_and_gradients(kind):
    """LNNPStep(virial_weight=1, neg_dy_weight=1).loss(..., box=boxes) and its parameter gradients (float64) against
    the same F.mse_loss terms put together from single-molecule create_graph=True evaluations on the single-box
    route, concatenated."""
    from torchmdnet.training import LNNPStep
    model = _model(kind, 64)
    z, pos, batch, boxes = _batch3(torch.float64)
    g = torch.Generator().manual_seed(17)
    y_l = torch.randn(3, 1, generator=g, dtype=torch.float64).to(DEV)
    f_l = torch.randn(pos.shape[0], 3, generator=g, dtype=torch.float64).to(DEV)
    w_l = torch.randn(3, 3, 3, generator=g, dtype=torch.float64).to(DEV)
    tr = LNNPStep(model, lr=0.0, y_weight=1.0, neg_dy_weight=1.0, virial_weight=1.0)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in model.named_parameters() if p.requires_grad]
    parts = [_alone(model, z, pos, batch, boxes, m, create_graph=True) for m in range(3)]
    loss_ref = (F.mse_loss(torch.cat([r[2] for r in parts]), w_l) + F.mse_loss(torch.cat([r[0] for r in parts]), y_l)
                + F.mse_loss(torch.cat([r[1] for r in parts]), f_l))
    grads = torch.autograd.grad(loss_ref, params, allow_unused=True)
    ref = {n: (torch.zeros_like(p) if gi is None else gi.detach().clone()) for n, p, gi in zip(names, params, grads)}
    tr.opt.zero_grad(set_to_none=False)
    loss = tr.loss(z, pos.clone(), batch, y_l, f_l, virial=w_l, box=boxes)
    tr.backward(loss)
    print(f"{kind}: loss {float(loss):.12e}, reference {float(loss_ref):.12e}")
    assert abs(float(loss) - float(loss_ref)) <= 1e-9 * abs(float(loss_ref))
    seen = 0
    for n, p in zip(names, params):
        got = torch.zeros_like(p) if p.grad is None else p.grad
        _close(got, ref[n], torch.float64, f"{kind} {n}")
        seen += float(ref[n].abs().max()) > 0
    assert seen > 0
    # step() takes the box as well
    tr.step(z, pos.clone(), batch, y_l, f_l, virial=w_l, box=boxes)


# ----------------------------------------------------------------------------- 8. capture
@pytest.mark.parametrize("precision", [64, 32])
def test_captured_evaluation_follows_a_changing_cell(precision):
    """GraphedEnergyForces(..., box=boxes, virial=True): a replay with every box and the positions scaled by 1.03
    equals the eager call with the new boxes; so does a replay back at the first cell."""
    from torchmdnet.graphs import GraphedEnergyForces
    dtype = torch.float64 if precision == 64 else torch.float32
    model = _model("et", precision)
    z, pos, batch, boxes = _batch3(dtype)
    cells = [(pos * 1.03, boxes * 1.03), (pos, boxes)]
    eager = [tuple(t.detach().clone() for t in model.energy_forces_virial(z, p.clone(), batch, box=b))
             for p, b in cells]
    assert float((eager[0][0] - eager[1][0]).abs().max()) > 0
    gm = GraphedEnergyForces(model, z, pos, batch, box=boxes, virial=True)
    try:
        assert gm.box.shape == (3, 3, 3) and gm.box.dtype == torch.float64 and gm.box.data_ptr() != boxes.data_ptr()
        for (p, b), (y_e, f_e, w_e) in zip(cells, eager):
            y, f = gm(p, box=b)
            gm.check_capacity()
            _close(y, y_e, dtype, "captured y")
            _close(f, f_e, dtype, "captured forces")
            _close(gm.virial, w_e, dtype, "captured virial")
    finally:
        gm.release()
    with pytest.raises(ValueError, match="without a box"):
        plain = GraphedEnergyForces(model, z, pos, batch)
        try:
            plain(pos, box=boxes)
        finally:
            plain.release()


# ----------------------------------------------------------------------------- 9. other entry points
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_get_neighbor_pairs_takes_the_boxes(strategy, dt):
    """torchmdnet_neighbors::get_neighbor_pairs with (n, 3, 3): the list of test 1 in the reference op's layout, and
    OptimizedDistance.forward(pos, batch, box) through it."""
    from torchmdnet.models.utils import OptimizedDistance
    from torchmdnet.neighbors import get_neighbor_pairs_kernel
    c = BB.get("main", dt)
    pos, batch, boxes = _inputs(c)
    rp, rd, rr = BB.ref("main", dt)
    P, tol = rp.shape[1], TOL[dt]
    nb, dl, dist, num = get_neighbor_pairs_kernel(strategy, pos, batch, boxes, True, 0.0, c.cutoff, P + 64, True, True)
    assert int(num.item()) == P and (nb[:, P:] == -1).all()
    raw = _raw(strategy, pos, batch, boxes, c.cutoff, P + 64)
    assert torch.equal(nb, raw[0]) and torch.equal(dl, raw[1]) and torch.equal(dist, raw[2])
    got, gd, gr = NC.sort_edges(nb[:, :P].cpu().numpy().astype(np.int64), dl[:P].cpu().numpy(), dist[:P].cpu().numpy())
    assert np.array_equal(got, rp)
    assert np.allclose(gd, rd, rtol=tol, atol=tol) and np.allclose(gr, rr, rtol=tol, atol=tol)
    od = OptimizedDistance(0.0, c.cutoff, max_num_pairs=P + 64, return_vecs=True, loop=True, strategy=strategy)
    ei, ew, ev = od(pos, batch, boxes)
    assert ei.shape == (2, P) and torch.equal(ei, nb[:, :P].long()) and torch.equal(ew, dist[:P])
    assert torch.equal(ev, dl[:P])
    g = od.graph(pos, batch, boxes)
    assert g.num_pairs == P and torch.equal(g.src, nb[0, :P])


@pytest.mark.parametrize("kind", ["et", "tn"])
def test_scripted_forward_refuses_a_box(kind):
    from torchmdnet import _native
    _native.load_torch_ops()
    model = _model(kind, 32)
    z, pos, batch, boxes = _batch3(torch.float32)
    scripted = torch.jit.script(model)
    y, f = scripted(z, pos.clone(), batch)  # without a box: as before
    assert y.shape == (3, 1) and f.shape == pos.shape
    # the scripted ``raise RuntimeError`` reaches Python as the interpreter's torch.jit.Error, naming the RuntimeError
    with pytest.raises((RuntimeError, torch.jit.Error), match="RuntimeError: .*per-call box runs eagerly"):
        scripted(z, pos.clone(), batch, box=boxes)
