"""The per-molecule virial (tmdnet_nl_backward_virial, TorchMD_Net.energy_forces_virial) on the GPU.

Kernel level: against ``kernels.nl_backward_virial_composite`` evaluated in float64 on upcast inputs, with
``grad_pos`` bitwise equal to tmdnet_nl_backward's.  Model level: against the exact strain derivative of
the fp64 oracle (tests/virial_ref.py) on the reference-run periodic fixtures, and against
``sum_i neg_dy_i (x) pos_i`` for isolated molecules.

Tolerances are the project's (tests/test_gpu_gn.py): float64 rtol = atol = 1e-9; float32 max|d| <= 1e-4 max|ref|.
"""
import types

import numpy as np
import pytest
import torch

import virial_ref as VR
from conftest import yaml_args
from oracle import model_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUTOFF = 5.0


def _close(a, ref, dtype, what):
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


def _same_call(y, f, y0, f0):
    """(y, neg_dy) of energy_forces_virial against the plain call's.  It IS the plain call (the same forward, the
    same force pass up to the neighbour backward, whose grad_pos is bitwise the same), so the forces -- segmented
    sums in a fixed order -- are ``torch.equal``.  The energies are not compared bitwise: the per-molecule energy
    reduction (reduce.hip) adds its atoms with LDS atomics whose order differs from launch to launch, so two
    PLAIN calls already differ in the last bits (measured on the 120-atom fixtures in float64: 2 of 6 repeated
    plain calls differed from the first by 2.7e-15 = 2.5 eps |y|).  Two orderings of the same N addends differ
    by at most ~N eps times their magnitude: the gate is N eps max|y|."""
    assert torch.equal(f, f0), "forces differ from the plain call"
    assert y.shape == y0.shape and y.dtype == y0.dtype
    tol = f.shape[0] * torch.finfo(y.dtype).eps * float(y0.detach().abs().max())
    assert float((y - y0).detach().abs().max()) <= tol, tol


# ----------------------------------------------------------------------------- kernel level
def _atoms():
    """48 atoms in 4 molecules of 30, 12, 5 and 1: the 30 lie in a sphere of radius 0.45 cutoff (every pair within
    the cutoff: rows of 29 or 30 entries = one full 16-lane stride plus a remainder); the single atom's row is
    empty."""
    g = torch.Generator().manual_seed(21)
    v = torch.randn(30, 3, generator=g, dtype=torch.float64)
    ball = v / v.norm(dim=1, keepdim=True) * (0.45 * CUTOFF) * torch.rand(30, 1, generator=g, dtype=torch.float64) ** (1 / 3)
    rest = torch.randn(18, 3, generator=g, dtype=torch.float64) * 1.5 + torch.tensor([20.0, 0.0, 0.0])
    pos = torch.cat([ball, rest])
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor([30, 12, 5, 1]))
    return pos, batch


def _build(pos, batch, loop, static, box=None, strategy="brute", room=None):
    """The CSR list as ``build_graph`` holds it: (graph stand-in, deltas, distances, E live edges).  Static:
    capacity = the pair count rounded up to 256 (at least one padding slot)."""
    from torchmdnet import kernels
    n = pos.shape[0]
    raw = lambda cap, pad: kernels.neighbor_pairs_raw(strategy, pos, batch, box, box is not None, 0.0, CUTOFF, cap,
                                                      loop, True, pad_output=pad, want_csr=True)
    nb, dl, dist, num, row_ptr, tr = raw(n * n if room is None else room, False)
    E = int(num.item())
    if static:
        cap = (E // 256 + 1) * 256
        nb, dl, dist, num, row_ptr, tr = raw(cap, True)
        assert int(num.item()) == E < cap
    else:
        nb, dl, dist, tr = nb[:, :E], dl[:E], dist[:E], tr[:E]
    graph = types.SimpleNamespace(row_ptr=row_ptr, transpose=tr, n_edges=dl.shape[0], src=nb[0], dst=nb[1])
    return graph, dl, dist, E


def _multi(pos, gd, gr, gr2, dl, dist, graph):
    from torchmdnet import _native as nat
    lib = nat.load()
    gpos = torch.empty_like(pos)
    rc = lib.tmdnet_nl_backward(nat.dtype_code(pos.dtype), pos.shape[0], nat.ptr(graph.row_ptr),
                                nat.ptr(graph.transpose), graph.n_edges, nat.ptr(gd), nat.ptr(gr), nat.ptr(gr2),
                                nat.ptr(dl), nat.ptr(dist), nat.ptr(gpos), nat.stream(pos.device))
    nat.check(rc, "tmdnet_nl_backward")
    return gpos


def _cotangents(which, E, rows, dtype):
    """Random cotangents for the E live edges; rows beyond them (static padding) are NaN: never read."""
    g = torch.Generator().manual_seed(5)
    out = {}
    for name, shape in (("gd", (E, 3)), ("gr", (E,)), ("gr2", (E,))):
        v = torch.randn(shape, generator=g, dtype=torch.float64)
        if name in which:
            full = torch.full((rows,) + shape[1:], float("nan"), dtype=torch.float64)
            full[:E] = v
            out[name] = full.to(dtype).to(DEV)
        else:
            out[name] = None
    return out["gd"], out["gr"], out["gr2"]


def _kernel_case(pos64, batch, loop, static, which, dtype, box=None, need_shift=False):
    from torchmdnet import kernels
    pos = pos64.to(dtype).to(DEV)
    batch = batch.to(DEV)
    n_mol = int(batch.max()) + 1
    b = None if box is None else box.to(dtype)
    graph, dl, dist, E = _build(pos, batch, loop, static, box=b)
    rows = dl.shape[0]
    counts = (graph.row_ptr[1:] - graph.row_ptr[:-1]).cpu()
    if box is None:
        assert int(counts[0]) == (30 if loop else 29) and int(counts[-1]) == (1 if loop else 0)
    if need_shift:
        raw = pos[graph.src[:E].long()] - pos[graph.dst[:E].long()]
        assert float((dl[:E] - raw).abs().max()) > 1.0, "no edge crosses a periodic image"
    gd, gr, gr2 = _cotangents(which, E, rows, dtype)
    if static:  # the padding rows of the geometry buffers too (pad_output = 0 leaves garbage there)
        dl = dl.clone()
        dist = dist.clone()
        dl[E:] = float("nan")
        dist[E:] = float("nan")
    ref_gpos = _multi(pos, gd, gr, gr2, dl, dist, graph)
    gpos, w = kernels.nl_backward_virial(pos, gd, gr, gr2, dl, dist, graph, batch, n_mol)
    torch.cuda.synchronize()
    assert torch.equal(gpos, ref_gpos), "grad_pos differs from tmdnet_nl_backward"
    up = lambda t: None if t is None else t[:E].double()
    ref = kernels.nl_backward_virial_composite(up(gd), up(gr), up(gr2), dl[:E].double(), dist[:E].double(),
                                               graph.dst[:E], batch, n_mol)
    assert w.shape == (n_mol, 3, 3) and w.dtype == dtype
    _close(w, ref, dtype, f"loop={loop} static={static} {sorted(which)} {dtype}")
    assert float(ref[0].abs().max()) > 0 and float(ref[-1].abs().max()) == 0  # the single atom: no pair
    return gpos, w


SETS = [("gd",), ("gr",), ("gr", "gr2"), ("gd", "gr", "gr2")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", SETS, ids=["gd", "gr", "gr+gr2", "all"])
@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
def test_kernel_against_composite(loop, which, dtype):
    """Dynamic list and static capacity (NaN in every padding row) on the same input: each against the float64
    composite, grad_pos bitwise tmdnet_nl_backward's, and the two forms agree with each other."""
    pos, batch = _atoms()
    g_dyn, w_dyn = _kernel_case(pos, batch, loop, False, set(which), dtype)
    g_st, w_st = _kernel_case(pos, batch, loop, True, set(which), dtype)
    assert torch.equal(g_dyn, g_st)
    _close(w_st, w_dyn, dtype, "static vs dynamic")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_periodic_image_shifts(dtype):
    """The same atoms wrapped into a triclinic box (L = 2.2 cutoff, brute): edges across the cell faces carry a
    non-zero image shift, and the virial is the sum over the minimum-image deltas."""
    pos, batch = _atoms()
    L = 2.2 * CUTOFF
    box = torch.tensor([[L, 0, 0], [0.2 * L, L, 0], [0.1 * L, -0.15 * L, L]], dtype=torch.float64)
    pos = pos.clone()
    pos[30:] -= torch.tensor([20.0, 0.0, 0.0]) - 0.5 * box.sum(0)  # the small molecules inside the cell
    s = pos @ torch.linalg.inv(box)  # the ball sits on the cell's corner: wrapping splits it over 8 images
    pos = (s - torch.floor(s)) @ box
    _kernel_case(pos, batch, False, False, {"gd", "gr", "gr2"}, dtype, box=box, need_shift=True)


def test_molecule_envelope_falls_back():
    """One molecule more than the sum kernel's ceiling (tmdnet_atom_sum_fwd's, 8192): a 3-atom molecule followed
    by single atoms.  The entry point reports unsupported and launches nothing; the Python path runs the row
    pass alone and sums per molecule itself."""
    from torchmdnet import _native as nat, kernels
    n_mol = kernels.ATOM_SUM_MAX_MOLECULES + 1
    n = n_mol + 2
    g = torch.Generator().manual_seed(3)
    pos = torch.cat([torch.randn(3, 3, generator=g, dtype=torch.float64),
                     torch.rand(n - 3, 3, generator=g, dtype=torch.float64) * 50]).to(DEV)
    batch = torch.cat([torch.zeros(3, dtype=torch.long), torch.arange(1, n_mol)]).to(DEV)
    graph, dl, dist, E = _build(pos, batch, False, False, room=4096)
    assert E == 6
    gr = torch.randn(E, generator=g, dtype=torch.float64).to(DEV)
    gpos = torch.full_like(pos, 7.0)
    out = torch.full((n_mol, 9), 7.0, dtype=pos.dtype, device=DEV)
    scratch = torch.full((n, 9), 7.0, dtype=pos.dtype, device=DEV)
    rc = nat.load().tmdnet_nl_backward_virial(nat.F64, n, nat.ptr(graph.row_ptr), nat.ptr(graph.transpose), E, None,
                                              nat.ptr(gr), None, nat.ptr(dl), nat.ptr(dist), nat.ptr(gpos),
                                              nat.ptr(batch), n_mol, nat.ptr(out), nat.ptr(scratch),
                                              nat.stream(pos.device))
    torch.cuda.synchronize()
    assert rc == nat.UNSUPPORTED
    assert bool((gpos == 7.0).all()) and bool((out == 7.0).all()) and bool((scratch == 7.0).all())
    gpos, w = kernels.nl_backward_virial(pos, None, gr, None, dl, dist, graph, batch, n_mol)
    assert torch.equal(gpos, _multi(pos, None, gr, None, dl, dist, graph))
    ref = kernels.nl_backward_virial_composite(None, gr, None, dl, dist, graph.dst, batch, n_mol)
    _close(w, ref, torch.float64, "fallback")
    assert float(w[0].abs().max()) > 0 and float(w[1:].abs().max()) == 0


# ----------------------------------------------------------------------------- model level: periodic fixtures
def _fixture_model(name, precision, strategy):
    from conftest import golden, state_dict_from
    from torchmdnet.models.model import create_model
    d = golden(name + ".npz")
    dtype = torch.float64 if precision == 64 else torch.float32
    m = create_model(VR.fixture_args(name, precision))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict_from(d).items()})
    if name.startswith("tn"):
        static = "static" in name
        m.representation_model.static_shapes = static
        m.representation_model.distance.resize_to_fit = not static
    m = m.to(DEV)
    dist = m.representation_model.distance
    dist.box = torch.as_tensor(d["box"]).to(dtype)
    dist.use_periodic = True
    dist.strategy = strategy
    return m, torch.as_tensor(d["z"]).to(DEV), torch.as_tensor(d["pos"]).to(dtype).to(DEV), \
        torch.as_tensor(d["batch"]).to(DEV), dtype


FIXTURE_CASES = [(n, p) for n in VR.PERIODIC_FIXTURES for p in (64, 32) if not (p == 32 and "static" in n)]


@pytest.mark.parametrize("strategy", ["brute", "cell"])
@pytest.mark.parametrize("name,precision", FIXTURE_CASES)
def test_periodic_fixture_virial_vs_oracle(name, precision, strategy):
    """ET-tiny and TensorNet-tiny (dynamic and static shapes) on the reference-run 120-atom periodic water box
    (rectangular: the cell list applies): the virial against the oracle's exact strain derivative, and (y, neg_dy)
    equal to the plain call's."""
    m, z, pos, batch, dtype = _fixture_model(name, precision, strategy)
    y_ref, f_ref, w_ref = VR.fixture_virial(name)
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch)
    y0, f0 = m(z, pos.clone(), batch)
    _same_call(y, f, y0, f0)
    assert w.shape == (1, 3, 3) and w.dtype == dtype and not w.requires_grad
    _close(f, f_ref, dtype, f"{name} {strategy} forces")
    _close(w, w_ref, dtype, f"{name} {strategy} virial")


# the ET launch forms that only large systems turn on, forced as tests/test_gpu_periodic_oracle.py forces them (the
# fixture of that file, restated: existing test files stay as they are)
@pytest.fixture
def large_switches(monkeypatch):
    from torchmdnet import et_stack, kernels
    monkeypatch.setattr(kernels, "REORDER_MIN_ATOMS", 0)
    monkeypatch.setattr(et_stack, "PLANAR_MIN_EDGES", 0)
    monkeypatch.setattr(kernels, "CHECK_SYMMETRY", True)
    prev = kernels.set_tuning(kernels.TUNE_ET_MERGED_MIN_NODES, 0)
    yield
    kernels.set_tuning(kernels.TUNE_ET_MERGED_MIN_NODES, prev)


_BOX_REF = {}


def _box_case():
    """ET at the width the fused kernels take (128 channels, 8 heads, 64 RBF; 2 layers) on a 600-atom periodic
    water box, with the oracle's virial -- computed once for both paths."""
    from torchmdnet.models.model import create_model
    args = yaml_args("equivariant-transformer", embedding_dimension=128, num_layers=2, num_rbf=64, num_heads=8,
                     cutoff_upper=5.0, max_num_neighbors=128, derivative=True)
    torch.manual_seed(0)
    m = create_model(args)
    n = 600
    g = torch.Generator().manual_seed(11)
    L = (n / 0.1003) ** (1.0 / 3.0)
    pos = torch.rand(n, 3, generator=g, dtype=torch.float64) * L
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3)
    batch = torch.zeros(n, dtype=torch.long)
    if not _BOX_REF:
        cfg = dict(args)
        cfg["box"] = np.eye(3) * L
        _BOX_REF["ref"] = VR.oracle_virial(m.state_dict(), cfg, z, pos, batch)
    return m, z, pos, batch, L, _BOX_REF["ref"]


@pytest.mark.parametrize("path", ["rows", "fused"])
def test_et_large_system_paths_virial_vs_oracle(path, large_switches, monkeypatch):
    """The two ET force passes of large systems -- pair rows with the merged dr-mode backward, and the
    fused-projection kernels -- hand the neighbour backward different cotangent sets; both give the oracle's
    virial (float32, cell list, Morton renumbering)."""
    from torchmdnet import et_stack, kernels
    fused_b = []
    if path == "fused":
        monkeypatch.setattr(et_stack, "FEP_MIN_EDGES", 0)
        orig_b = kernels.et_fused_bwd_launch
        monkeypatch.setattr(kernels, "et_fused_bwd_launch", lambda *a, **k: (fused_b.append(1), orig_b(*a, **k))[1])
    else:
        monkeypatch.setattr(et_stack, "FEP", "0")
    m, z, pos, batch, L, (y_ref, f_ref, w_ref) = _box_case()
    m = m.to(DEV)
    d = m.representation_model.distance
    d.box = torch.eye(3) * L
    d.use_periodic = True
    d.strategy = "cell"
    z, pos, batch = z.to(DEV), pos.float().to(DEV), batch.to(DEV)
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch)
    assert (len(fused_b) == 2) == (path == "fused")
    y0, f0 = m(z, pos.clone(), batch)
    _same_call(y, f, y0, f0)
    _close(f, f_ref, torch.float32, f"{path} forces")
    _close(w, w_ref, torch.float32, f"{path} virial")


# ----------------------------------------------------------------------------- model level: isolated molecules
def _pos_virial(f, pos, batch, n_mol):
    """sum_{i in m} neg_dy_i (x) pos_i in float64: the virial of isolated molecules."""
    t = f.detach().double().unsqueeze(2) * pos.detach().double().unsqueeze(1)
    return torch.zeros(n_mol, 3, 3, dtype=torch.float64, device=f.device).index_add_(0, batch, t)


def _small(model, precision=64, **kw):
    base = dict(embedding_dimension=32, num_layers=2, num_rbf=16, derivative=True, output_model="Scalar",
                precision=precision)
    if model == "equivariant-transformer":
        base.update(num_heads=4)
    if model == "graph-network":
        base.update(aggr="add", max_z=10)
    base.update(kw)
    return yaml_args(model, **base)


def _zbl_args():
    a = _small("equivariant-transformer")
    a["prior_model"] = [{"ZBL": dict(cutoff_distance=5.0, max_num_neighbors=40, atomic_number=list(range(100)),
                                     distance_scale=1e-10, energy_scale=4.35974e-18)}]
    return a


@pytest.mark.parametrize("kind", ["et", "tensornet", "gn", "et+zbl"])
def test_isolated_molecules_virial_is_force_times_position(kind):
    """Without a box virial[m] = sum_{i in m} neg_dy_i (x) pos_i, from the call's own forces (pinned by the
    existing tests); with a ZBL prior a second graph adds into the sink."""
    from torchmdnet.models.model import create_model
    args = {"et": lambda: _small("equivariant-transformer"), "tensornet": lambda: _small("tensornet"),
            "gn": lambda: _small("graph-network"), "et+zbl": _zbl_args}[kind]()
    torch.manual_seed(4)
    m = create_model(args).to(DEV)
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(3))
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch)
    y0, f0 = m(z, pos.clone(), batch)
    _same_call(y, f, y0, f0)
    assert w.shape == (3, 3, 3) and w.dtype == torch.float64 and not w.requires_grad
    _close(w, _pos_virial(f, pos, batch, 3), torch.float64, kind)
    if kind == "et+zbl":  # the prior's share is there: the model alone gives another virial
        m.prior_model = None
        _, _, w1 = m.energy_forces_virial(z, pos.clone(), batch)
        assert float((w - w1).abs().max()) > 1e-6 * float(w.abs().max())


def test_precision16_virial_is_float16():
    """A precision-16 model (float16 storage, float32 arithmetic) returns the virial in float16, like y.  Against
    sum_i neg_dy_i (x) pos_i from its own float16 forces: the virial and every force component were rounded to
    float16 once (relative 2^-11 each), so |d| <= 2^-11 (|ref| + sum_i |neg_dy_i| (x) |pos_i|) elementwise, plus the
    float32 bar of the arithmetic underneath."""
    from torchmdnet.models.model import create_model
    torch.manual_seed(4)
    m = create_model(_small("equivariant-transformer", precision=16)).to(DEV)
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(3))
    pos = pos.float()
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch)
    assert y.dtype == f.dtype == w.dtype == torch.float16 and w.shape == (3, 3, 3) and not w.requires_grad
    ref = _pos_virial(f, pos, batch, 3)
    bound = 2.0 ** -11 * (ref.abs() + _pos_virial(f.abs(), pos.abs(), batch, 3)) + 1e-4 * ref.abs().max()
    d = (w.double() - ref).abs()
    print(f"precision 16: max|d| = {float(d.max()):.3e}, max|ref| = {float(ref.abs().max()):.3e}")
    assert bool((d <= bound).all()), float((d - bound).max())


def test_optimized_graph_network_virial():
    """optimize() keeps the graph: the fused float32 model's virial against its float64 unoptimised twin."""
    from torchmdnet.models.model import create_model
    from torchmdnet.optimize import optimize
    torch.manual_seed(4)
    twin = create_model(_small("graph-network"))
    fused = create_model(_small("graph-network", precision=32))
    fused.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in twin.state_dict().items()})
    fused = optimize(fused).to(DEV)
    twin = twin.to(DEV)
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(3))
    _, _, w_ref = twin.energy_forces_virial(z, pos.clone(), batch)
    y, f, w = fused.energy_forces_virial(z, pos.float(), batch)
    y0, f0 = fused(z, pos.float(), batch)
    _same_call(y, f, y0, f0)
    assert w.dtype == torch.float32
    _close(w, w_ref, torch.float32, "optimized gn")


def test_sink_is_one_shot():
    """train(): after energy_forces_virial a force-matching backward (the second order of the neighbour op) and
    a plain call leave the returned virial alone; the next call returns a new tensor."""
    from torchmdnet.models.model import create_model
    torch.manual_seed(4)
    m = create_model(_small("equivariant-transformer")).to(DEV).train()
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(3))
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch)
    assert f.requires_grad and not w.requires_grad
    kept = w.clone()
    ((y ** 2).sum() + (f ** 2).sum()).backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m.parameters())
    m(z, pos.clone(), batch)
    torch.cuda.synchronize()
    assert torch.equal(w, kept)
    moved = pos * 1.01
    _, f2, w2 = m.energy_forces_virial(z, moved.clone(), batch)
    assert w2 is not w and w2.data_ptr() != w.data_ptr()
    assert torch.equal(w, kept)
    _close(w2, _pos_virial(f2, moved, batch, 3), torch.float64, "second call")
    assert float((w2 - w).abs().max()) > 0


def test_captured_virial_replays():
    """GraphedEnergyForces(virial=True): gm.virial is refreshed by every replay and matches the eager call;
    (y, neg_dy) equal those of a capture without the virial."""
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_model
    torch.manual_seed(4)
    m = create_model(_small("equivariant-transformer", precision=32)).to(DEV)
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(3))
    pos = pos.float()
    gm = GraphedEnergyForces(m, z, pos, batch, virial=True)
    assert gm.virial.shape == (3, 3, 3) and gm.virial.dtype == torch.float32
    gen = torch.Generator().manual_seed(3)
    sets = [pos + 0.05 * torch.randn(pos.shape, generator=gen).to(DEV) for _ in range(2)]
    got = []
    for p in sets:
        y, f = gm(p)
        gm.check_capacity()
        got.append((y.clone(), f.clone(), gm.virial.clone()))
    gm.release()
    plain = GraphedEnergyForces(m, z, pos, batch)
    assert plain.virial is None
    for p, (y, f, w) in zip(sets, got):
        y1, f1 = plain(p)
        _same_call(y, f, y1, f1)
    plain.release()
    for p, (y, f, w) in zip(sets, got):
        _, _, w_e = m.energy_forces_virial(z, p.clone(), batch)
        _close(w, w_e, torch.float32, "replayed virial")
    assert float((got[0][2] - got[1][2]).abs().max()) > 0
