"""Open molecules among per-molecule boxes on the GPU: an all-zero entry of the ``(n_molecules, 3, 3)`` boxes means
that molecule has no box (csrc/neighbors.hip ``k_pairs<.., MOLBOX>`` clears its wave's periodic flag), through
``neighbor_pairs_raw``, ``build_graph``, ``OptimizedDistance``, ``get_neighbor_pairs`` and the models'
``energy_forces_virial``.

Yardstick: tests/open_mol_ref.py (``neighbor_cases.reference`` once per molecule, ``box=None`` for the open one),
checked on the CPU by tests/test_open_molecules_cpu.py.  Pair sets are compared exactly; deltas and distances at
tests/test_gpu_neighbor_edges.TOL; model quantities at the project's gates (float64 rtol = atol = 1e-9, float32
max|d| <= 1e-4 max|ref|) against the float64 model evaluated one molecule at a time through the single-box route
(no box at all for the open molecule), which this feature leaves as it was.

TensorNet runs with ``static_shapes = False``, as in tests/test_gpu_batch_boxes.py.
"""
import numpy as np
import pytest
import torch

import neighbor_cases as NC
import open_mol_ref as OM
from conftest import yaml_args
from test_gpu_neighbor_edges import TDT, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOTH = list(NC.DTYPES)
ROWS = ["brute", "shared"]


def _inputs(c):
    pos = torch.tensor(c.pos, device=DEV)
    assert pos.dtype == TDT[c.dtype]
    return pos, torch.tensor(c.batch, device=DEV), torch.tensor(c.boxes, device=DEV)


def _raw(strategy, pos, batch, box, cutoff, cap, loop=True, transpose=True, periodic=True):
    from torchmdnet import kernels
    return kernels.neighbor_pairs_raw(strategy, pos, batch, box, periodic, 0.0, cutoff, cap, loop, transpose,
                                      pad_output=True, want_csr=True)


def _check_against_yardstick(c, out, loop, transpose):
    """Pair set == yardstick exactly, in its order (destination-major, sources ascending); row pointer; deltas and
    distances within TOL; padding; the open molecule's deltas are the plain differences bit for bit."""
    nb, dl, dist, num, row_ptr, T = out
    rp, rd, rr = OM.ref(c.dtype, c.shuffled, loop, transpose)
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
    rows = (c.batch[got[1]] == OM.OPEN) & (got[0] != got[1])
    assert rows.any()
    assert np.array_equal(gd[rows], c.pos[got[0][rows]] - c.pos[got[1][rows]])  # in the dtype: no image
    if transpose:
        t = T[:P].long()
        assert (t >= 0).all() and (T[P:] == -1).all()
        assert torch.equal(nb[0, :P][t], nb[1, :P]) and torch.equal(dl[:P][t], -dl[:P])
    else:
        assert T is None and (nb[0, :P] >= nb[1, :P]).all()
    return P


# ----------------------------------------------------------------------------- 1. the build
@pytest.mark.parametrize("transpose", [True, False], ids=["full", "half"])
@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_build_against_yardstick(strategy, dt, loop, transpose):
    """Sorted batch (each wave scans its own molecule) and static capacity with padding (P + 64 slots)."""
    c = OM.get(dt)
    pos, batch, boxes = _inputs(c)
    P = OM.ref(dt, False, loop, transpose)[0].shape[1]
    out = _raw(strategy, pos, batch, boxes, c.cutoff, P + 64, loop, transpose)
    _check_against_yardstick(c, out, loop, transpose)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_shuffled_batch(strategy, dt):
    """The atoms in random order: the batch descends, every atom is a candidate of every destination, and each
    destination still takes its own molecule's box -- or none."""
    c = OM.get(dt, True)
    pos, batch, boxes = _inputs(c)
    P = OM.ref(dt, True)[0].shape[1]
    _check_against_yardstick(c, _raw(strategy, pos, batch, boxes, c.cutoff, P + 64), True, True)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_entry_points_agree(strategy, dt):
    """build_graph (dynamic and static capacity), OptimizedDistance and get_neighbor_pairs hold the raw build's
    list; all of them pass the host checks with the all-zero box."""
    from torchmdnet import kernels
    from torchmdnet.models.utils import OptimizedDistance
    from torchmdnet.neighbors import get_neighbor_pairs_kernel
    c = OM.get(dt)
    pos, batch, boxes = _inputs(c)
    P = OM.ref(dt)[0].shape[1]
    raw = _raw(strategy, pos, batch, boxes, c.cutoff, P + 64)
    g = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, loop=True, strategy=strategy, box=boxes)
    assert g.symmetric and g.num_pairs == P
    assert torch.equal(g.src, raw[0][0, :P]) and torch.equal(g.deltas.detach(), raw[1][:P])
    gs = kernels.build_graph(pos, batch, 0.0, c.cutoff, P + 64, loop=True, strategy=strategy, box=boxes,
                             static_capacity=P + 192)
    assert not gs.overflow.item() and int(gs.num_pairs_dev.item()) == P
    assert torch.equal(gs.src[:P], raw[0][0, :P]) and torch.equal(gs.deltas.detach()[:P], raw[1][:P])
    assert (gs.src[P:] == -1).all() and (gs.deltas.detach()[P:] == 0).all()
    nb, dl, dist, num = get_neighbor_pairs_kernel(strategy, pos, batch, boxes, True, 0.0, c.cutoff, P + 64, True, True)
    assert int(num.item()) == P
    assert torch.equal(nb, raw[0]) and torch.equal(dl, raw[1]) and torch.equal(dist, raw[2])
    od = OptimizedDistance(0.0, c.cutoff, max_num_pairs=P + 64, return_vecs=True, loop=True, strategy=strategy)
    ei, ew, ev = od(pos, batch, boxes)
    assert ei.shape == (2, P) and torch.equal(ei, nb[:, :P].long()) and torch.equal(ew, dist[:P])
    assert torch.equal(ev, dl[:P])
    assert torch.equal(od.graph(pos, batch, boxes).src, raw[0][0, :P])


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("strategy", ROWS)
def test_all_zero_boxes_are_bitwise_the_call_without_a_box(strategy, dt):
    c = OM.get(dt)
    pos, batch, _ = _inputs(c)
    zeros = torch.zeros(len(c.sizes), 3, 3, dtype=torch.float64, device=DEV)
    a = _raw(strategy, pos, batch, zeros, c.cutoff, 4096)
    b = _raw(strategy, pos, batch, None, c.cutoff, 4096, periodic=False)
    assert 200 < int(a[3].item()) < 4096
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    from torchmdnet import kernels
    g = kernels.build_graph(pos, batch, 0.0, c.cutoff, 4096, box=zeros)  # and the host checks let it through
    assert g.num_pairs == int(b[3].item())


def test_partly_zero_and_lone_zero_boxes_are_refused():
    from torchmdnet import kernels
    from torchmdnet.neighbors import get_neighbor_pairs_kernel
    c = OM.get("f32")
    pos, batch, boxes = _inputs(c)
    bad = boxes.clone()
    bad[OM.OPEN, 0, 0] = 7.0
    msg = r"molecule 1: Invalid box vectors: box_vectors\[1\]\[1\] < 2\*cutoff"
    with pytest.raises(RuntimeError, match=msg):
        kernels.build_graph(pos, batch, 0.0, c.cutoff, 4096, box=bad)
    with pytest.raises(RuntimeError, match=msg):
        get_neighbor_pairs_kernel("brute", pos, batch, bad, True, 0.0, c.cutoff, 4096, True, True)
    one = torch.zeros(pos.shape[0], dtype=torch.long, device=DEV)
    lone = r"Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"
    for z in (torch.zeros(1, 3, 3, dtype=torch.float64, device=DEV), torch.zeros(3, 3, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match=lone):
            kernels.build_graph(pos, one, 0.0, c.cutoff, 8192, box=z)
        with pytest.raises(RuntimeError, match=lone):
            get_neighbor_pairs_kernel("brute", pos, one, z, True, 0.0, c.cutoff, 8192, True, True)


# ----------------------------------------------------------------------------- 2. models
def _model_args(kind, precision):
    common = dict(embedding_dimension=32, num_layers=2, num_rbf=16, max_num_neighbors=64, cutoff_upper=OM.CUTOFF,
                  derivative=True, output_model="Scalar", precision=precision, max_z=10)
    if kind == "et":
        return yaml_args("equivariant-transformer", num_heads=4, **common)
    return yaml_args("tensornet", **common)


_MODELS = {}


def _models(kind):
    """(float64 model, float32 model with the same weights rounded)."""
    from torchmdnet.models.model import create_model
    if kind not in _MODELS:
        torch.manual_seed(11)
        pair = [create_model(_model_args(kind, p)) for p in (64, 32)]
        pair[1].load_state_dict({k: (v.float() if v.is_floating_point() else v)
                                 for k, v in pair[0].state_dict().items()})
        for m in pair:
            if kind == "tn":
                m.representation_model.static_shapes = False
                m.representation_model.distance.resize_to_fit = True
            m.to(DEV)
        _MODELS[kind] = pair
    return _MODELS[kind]


_ALONE = {}


def _alone_f64(kind):
    """The float64 model on every molecule alone: its box as the distance module's own, none for the open one.
    Computed once per kind.  Shared: treat as read-only."""
    if kind not in _ALONE:
        model = _models(kind)[0]
        c = OM.get("f64")
        pos, batch, boxes = _inputs(c)
        z = torch.tensor(c.z, device=DEV)
        d = model.representation_model.distance
        parts = []
        for m in range(len(c.sizes)):
            idx = (batch == m).nonzero().flatten()
            old = (d.box, d.use_periodic)
            if not OM.is_open(c.boxes[m]):
                d.box, d.use_periodic = boxes[m].cpu(), True
            try:
                parts.append(model.energy_forces_virial(z[idx], pos[idx].clone(), torch.zeros_like(idx)))
            finally:
                d.box, d.use_periodic = old
        _ALONE[kind] = tuple(torch.cat([p[k] for p in parts]).detach() for k in range(3))
    return _ALONE[kind]


def _close(a, ref, dtype, what):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape and bool(torch.isfinite(a).all()), what
    err = float((a - ref).abs().max())
    print(f"{what}: max|d| = {err:.3e}, max|ref| = {float(ref.abs().max()):.3e}")
    if dtype == torch.float64:
        assert torch.allclose(a, ref, rtol=1e-9, atol=1e-9), (what, err)
    else:
        assert err <= 1e-4 * float(ref.abs().max()), (what, err)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("kind", ["et", "tn"])
def test_models_with_an_open_molecule_in_the_batch(kind, precision):
    """energy_forces_virial(..., box=boxes) with the all-zero box: y, forces and virial against the float64 model
    on each molecule alone; the open molecule's virial is sum_i F_i (x) pos_i of this call's own forces."""
    dtype = torch.float64 if precision == 64 else torch.float32
    model = _models(kind)[precision == 32]
    c = OM.get("f64" if precision == 64 else "f32")
    pos, batch, boxes = _inputs(c)
    z = torch.tensor(c.z, device=DEV)
    y, f, w = model.energy_forces_virial(z, pos.clone(), batch, box=boxes)
    assert y.shape == (4, 1) and w.shape == (4, 3, 3) and w.dtype == dtype
    y_ref, f_ref, w_ref = _alone_f64(kind)
    _close(y, y_ref, dtype, f"{kind} y")
    _close(f, f_ref, dtype, f"{kind} forces")
    _close(w, w_ref, dtype, f"{kind} virial")
    idx = (batch == OM.OPEN).nonzero().flatten()
    own = f.detach().double()[idx].T @ pos.double()[idx]
    _close(w[OM.OPEN], own, dtype, f"{kind} open molecule's virial against sum F (x) pos")
    # the boxes matter for the boxed molecules and not for the open one
    y0, _ = model(z, pos.clone(), batch)
    tol = 1e-9 if precision == 64 else 1e-4
    assert abs(float((y0[OM.OPEN] - y[OM.OPEN]).detach())) <= tol * float(y.detach().abs().max())
    assert float((y0 - y).detach().abs()[[0, 2]].min()) > 1e-3 * float(y.detach().abs().max())
