"""Periodic pair priors on the GPU: ``ZBL(periodic=True)`` and ``D2(periodic=True)`` build their own list under the
call's box -- one ``(3, 3)`` box, per-molecule boxes with a triclinic and an open one, or the distance module's own --
with their own cutoff (3.0 here), by ``"brute"`` or ``"cell"``; their pairs reach the virial and its second order;
``GraphedEnergyForces`` replays follow a new box.

Yardstick: tests/periodic_prior_ref.py, the dense float64 minimum-image restatement (pinned on the CPU by
tests/test_open_molecules_cpu.py), evaluated on the CPU.  Inputs: the batch of tests/open_mol_ref.py, where every boxed
molecule has pairs that exist only through a face.

Gates, from tests/test_gpu_pair_priors.py: float64 rtol = atol = 1e-9; float32 max|d| <= 1e-4 max|ref|."""
import functools

import pytest
import torch

import open_mol_ref as OM
import periodic_prior_ref as PR
from conftest import yaml_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALES = dict(distance_scale=1e-10, energy_scale=4.35974e-18)
NUMBERS = list(range(100))
CUT = 3.0
KINDS = ["zbl", "d2"]
DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
N_MOL = len(OM.SIZES)


def _prior(kind, cutoff=CUT, **kw):
    from torchmdnet.priors import D2, ZBL
    kw.setdefault("periodic", True)
    if kind == "zbl":
        return ZBL(cutoff, 64, atomic_number=NUMBERS, **SCALES, **kw).to(DEV)
    return D2(cutoff, 64, atomic_number=NUMBERS, dtype=torch.float64, **SCALES, **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def _d2_tables():
    t = _prior("d2")
    return t.C_6.cpu(), t.R_r.cpu()


def _ref_energy(kind, z, batch, n_mol, boxes):
    """The restatement as ``(pos, eps=None) -> (n_mol,)`` on the CPU in float64."""
    z, batch = z.cpu(), batch.cpu()
    boxes = None if boxes is None else boxes.detach().cpu().double()
    if kind == "zbl":
        return lambda p, eps=None: PR.zbl_energy(p, z, batch, n_mol, CUT, NUMBERS, boxes=boxes, eps=eps, **SCALES)
    c6, r_r = _d2_tables()
    return lambda p, eps=None: PR.d2_energy(p, z, batch, n_mol, CUT, NUMBERS, c6=c6, r_r=r_r, boxes=boxes, eps=eps,
                                            **SCALES)


def _prior_energy(prior, z, batch, n_mol, box):
    def energy(p):
        y0 = torch.zeros(n_mol, 1, dtype=p.dtype, device=p.device)
        return prior.post_reduce_box(y0, z, p, batch, None, box)
    return energy


def _orders(energy, pos):
    """(y, F = -dy/dpos, d(sum F^2)/dpos) of ``energy(pos) -> (n_mol,) or (n_mol, 1)``, as float64 on the CPU."""
    p = pos.detach().clone().requires_grad_(True)
    y = energy(p).reshape(-1)
    f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
    h, = torch.autograd.grad((f ** 2).sum(), p)
    return [t.detach().double().cpu() for t in (y, f, h)]


def _check(got, ref, dtype, what, names=("y", "forces", "dF2")):
    for name, a, b in zip(names, got, ref):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print(f"{what} {name}: max|d| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    for name, a, b in zip(names, got, ref):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), (what, name)
        if dtype == torch.float64:
            assert torch.allclose(a, b, rtol=1e-9, atol=1e-9), (what, name)
        else:
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), (what, name)


def _same_evaluation(a, b, pos):
    """Two energy functions that must run the same kernels on the same list: the forces (CSR sums in a fixed order)
    are bit for bit the same; the energies go through the per-molecule sum's atomic adds, whose order is
    unspecified, so they agree to N eps max|y| (tests/test_gpu_virial._same_call)."""
    outs = []
    for energy in (a, b):
        p = pos.detach().clone().requires_grad_(True)
        y = energy(p)
        f, = torch.autograd.grad(-y.sum(), p)
        outs.append((y.detach(), f))
    (ya, fa), (yb, fb) = outs
    assert torch.equal(fa, fb)
    assert float((ya - yb).abs().max()) <= pos.shape[0] * torch.finfo(pos.dtype).eps * float(yb.abs().max())
    return yb


def _batch(dtype):
    c = OM.get("f64" if dtype == torch.float64 else "f32")
    return (torch.tensor(c.z, device=DEV), torch.tensor(c.pos, device=DEV), torch.tensor(c.batch, device=DEV),
            torch.tensor(c.boxes, device=DEV))


def _molecule(dtype, m):
    """Molecule m of the batch alone: (z, pos, batch of zeros, its (3, 3) box on the host)."""
    z, pos, batch, boxes = _batch(dtype)
    idx = (batch == m).nonzero().flatten()
    return z[idx], pos[idx].contiguous(), torch.zeros_like(idx), boxes[m].cpu()


@functools.lru_cache(maxsize=None)
def _ref_orders(kind, dtype, case):
    """The restatement's (y, F, dF2) on the positions the GPU sees, once per case.  Shared: treat as read-only."""
    if case == "batch":
        z, pos, batch, boxes = _batch(dtype)
        return tuple(_orders(_ref_energy(kind, z, batch, N_MOL, boxes), pos.double().cpu()))
    if case == "batch_open":  # no box anywhere
        z, pos, batch, _ = _batch(dtype)
        return tuple(_orders(_ref_energy(kind, z, batch, N_MOL, None), pos.double().cpu()))
    z, pos, batch, box = _molecule(dtype, int(case))
    return tuple(_orders(_ref_energy(kind, z, batch, 1, box), pos.double().cpu()))


# ----------------------------------------------------------------------------- energy, forces, second order
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_box(kind, dtype):
    """The triclinic molecule alone under its (3, 3) box, given on the host and on the device."""
    z, pos, batch, box = _molecule(dtype, 2)
    prior = _prior(kind)
    ref = _ref_orders(kind, dtype, "2")
    _check(_orders(_prior_energy(prior, z, batch, 1, box), pos), ref, dtype, f"{kind} (3, 3) host")
    assert int(prior.last_num_pairs) > 0
    _check(_orders(_prior_energy(prior, z, batch, 1, box.to(DEV)), pos), ref, dtype, f"{kind} (3, 3) device")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_per_molecule_boxes_with_a_triclinic_and_an_open_one(kind, dtype):
    z, pos, batch, boxes = _batch(dtype)
    got = _orders(_prior_energy(_prior(kind), z, batch, N_MOL, boxes), pos)
    _check(got, _ref_orders(kind, dtype, "batch"), dtype, f"{kind} per-molecule boxes")
    assert float(got[0][3]) == 0.0 and float(got[0][OM.OPEN]) != 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_opt_in(kind, dtype):
    """periodic=False with a box is exactly the call without one (the same list: ``_same_evaluation``); periodic=True
    changes the boxed molecules' energies and leaves the open molecule's; periodic=True without a box is the
    non-periodic evaluation."""
    z, pos, batch, boxes = _batch(dtype)
    plain, per = _prior(kind, periodic=False), _prior(kind)
    no_box = _prior_energy(plain, z, batch, N_MOL, None)
    without = _same_evaluation(_prior_energy(plain, z, batch, N_MOL, boxes), no_box, pos)
    five = lambda p: plain.post_reduce(torch.zeros(N_MOL, 1, dtype=dtype, device=DEV), z, p, batch, None)  # no keyword
    _same_evaluation(five, no_box, pos)
    _same_evaluation(_prior_energy(per, z, batch, N_MOL, None), no_box, pos)
    _check(_orders(_prior_energy(plain, z, batch, N_MOL, boxes), pos), _ref_orders(kind, dtype, "batch_open"), dtype,
           f"{kind} periodic=False")
    y = _prior_energy(per, z, batch, N_MOL, boxes)(pos)
    scale = float(without.abs().max())
    assert abs(float(y[0] - without[0])) > 1e-3 * scale and abs(float(y[2] - without[2])) > 1e-3 * scale
    # the open molecule: the same pairs and deltas (the bound of _same_evaluation)
    assert abs(float(y[OM.OPEN] - without[OM.OPEN])) <= pos.shape[0] * torch.finfo(dtype).eps * scale


# ----------------------------------------------------------------------------- through the model
def _model_args(precision, prior=None):
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                     max_num_neighbors=64, cutoff_upper=CUT, derivative=True, output_model="Scalar",
                     precision=precision, max_z=10)
    if prior is not None:
        args["prior_model"] = [{"ZBL": dict(cutoff_distance=CUT, max_num_neighbors=64, atomic_number=NUMBERS,
                                            **SCALES, **prior)}]
    return args


def _model(precision, prior=None):
    from torchmdnet.models.model import create_model
    torch.manual_seed(11)
    return create_model(_model_args(precision, prior)).to(DEV)


def test_model_hands_the_box_to_its_periodic_prior():
    """float64 ET + ZBL(periodic=True) equals the same weights without a prior plus the restatement: with ``box=``
    per molecule, and with the distance module's own (3, 3) box and no call box.  A non-periodic ZBL in the same
    model stays the non-periodic restatement."""
    from torchmdnet.priors import ZBL
    z, pos, batch, boxes = _batch(torch.float64)
    with_p, with_np, bare = _model(64, dict(periodic=True)), _model(64, dict()), _model(64)
    assert isinstance(with_p.prior_model[0], ZBL) and with_p.prior_model[0].periodic
    assert not with_np.prior_model[0].periodic
    y0, f0 = bare(z, pos.clone(), batch, box=boxes)
    for model, case in ((with_p, "batch"), (with_np, "batch_open")):
        y, f = model(z, pos.clone(), batch, box=boxes)
        ry, rf, _ = _ref_orders("zbl", torch.float64, case)
        _check([(y - y0).detach().reshape(-1).cpu(), (f - f0).detach().cpu()], [ry, rf], torch.float64,
               f"model box= ({case})", names=("y", "forces"))
    # the module's own box
    zm, pm, bm, box = _molecule(torch.float64, 2)
    ry, rf, _ = _ref_orders("zbl", torch.float64, "2")
    outs = []
    for model in (with_p, bare):
        d = model.representation_model.distance
        old = (d.box, d.use_periodic)
        d.box, d.use_periodic = box, True
        try:
            outs.append(model(zm, pm.clone(), bm))
        finally:
            d.box, d.use_periodic = old
    _check([(outs[0][0] - outs[1][0]).detach().reshape(-1).cpu(), (outs[0][1] - outs[1][1]).detach().cpu()], [ry, rf],
           torch.float64, "model, the module's own box", names=("y", "forces"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_modules_own_box_with_no_call_box(kind, dtype):
    """No ``box=``: ``TorchMD_Net._post_reduce_priors`` hands the prior the distance module's own host box, cast to
    the dtype of the positions.  The box is the triclinic one scaled by 1 + 1e-6, which float32 cannot hold (the
    pair set does not change: the fixture's margin is 3e-4), so in float32 the prior builds under the rounded box,
    and that is the box the restatement is given.  Energy, forces and d(sum F^2)/dpos of the priors' share."""
    z, pos, batch, box = _molecule(dtype, 2)
    own = box * (1.0 + 1e-6)
    seen = own.to(dtype).double()
    assert torch.equal(seen, own) == (dtype == torch.float64)
    model = _model(64 if dtype == torch.float64 else 32, dict(periodic=True))
    model.prior_model = torch.nn.ModuleList([_prior(kind)])
    d = model.representation_model.distance
    d.box, d.use_periodic = own, True

    def energy(p):
        return model._post_reduce_priors(torch.zeros(1, 1, dtype=dtype, device=DEV), z, p, batch, None, None)

    got = _orders(energy, pos)
    assert int(model.prior_model[0].last_num_pairs) > 0
    ref = _orders(_ref_energy(kind, z, batch, 1, seen), pos.double().cpu())
    _check(got, ref, dtype, f"{kind} the module's own box")
    # and it is the box that matters: a non-periodic module gives the prior none
    d.use_periodic = False
    open_ref = _orders(_ref_energy(kind, z, batch, 1, None), pos.double().cpu())
    _check(_orders(energy, pos), open_ref, dtype, f"{kind} a non-periodic module")
    assert float((ref[0] - open_ref[0]).abs().max()) > 1e-3 * float(ref[0].abs().max())


def _two_in_one_box(dtype):
    """The 70-atom molecule as two molecules of 35 atoms that share its box."""
    z, pos, _, box = _molecule(dtype, 0)
    batch = torch.repeat_interleave(torch.arange(2, device=DEV), 35)
    return z, pos, batch, box


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_all_pairs_prior_takes_the_one_device_box_of_a_cell_list_model(kind, dtype):
    """A model on the cell list hands its one ``(1, 3, 3)`` device box to every prior; an all-pairs prior over two
    molecules expands it per molecule (``PairPrior._graph``)."""
    z, pos, batch, box = _two_in_one_box(dtype)
    prior = _prior(kind)
    got = _orders(_prior_energy(prior, z, batch, 2, box.to(DEV).reshape(1, 3, 3)), pos)
    _check(got, tuple(_orders(_ref_energy(kind, z, batch, 2, box), pos.double().cpu())), dtype,
           f"{kind} (1, 3, 3) over two molecules")
    _same_evaluation(_prior_energy(prior, z, batch, 2, box.to(DEV).reshape(1, 3, 3)),
                     _prior_energy(prior, z, batch, 2, box.to(DEV).expand(2, 3, 3).contiguous()), pos)


def test_cell_list_model_with_an_all_pairs_prior_eager_and_captured():
    """ET on the cell list + ZBL(periodic=True) on the default strategy, two molecules in one box: the eager call
    with the ``(1, 3, 3)`` device box equals the bare model plus the restatement, and a captured replay with the
    box and the positions scaled by 1.05 equals the eager call at the new box."""
    from torchmdnet.graphs import GraphedEnergyForces
    z, pos, batch, box = _two_in_one_box(torch.float32)
    model, bare = _model(32, dict(periodic=True)), _model(32)
    for m in (model, bare):
        m.representation_model.distance.strategy = "cell"
    dbox = box.to(DEV).reshape(1, 3, 3)
    y, f = model(z, pos.clone(), batch, box=dbox)
    y0, f0 = bare(z, pos.clone(), batch, box=dbox)
    ry, rf, _ = _orders(_ref_energy("zbl", z, batch, 2, box), pos.double().cpu())
    # the prior's share as a difference of two float32 evaluations: the gate is taken on the whole model's scale
    for name, a, b, whole in (("y", (y - y0).reshape(-1), ry, y), ("forces", f - f0, rf, f)):
        err = float((a.detach().double().cpu() - b).abs().max())
        scale = max(float(b.abs().max()), float(whole.detach().abs().max()))
        print(f"cell model + brute prior {name}: max|d| = {err:.3e}, scale = {scale:.3e}")
        assert err <= 1e-4 * scale
    cells = [(pos * 1.05, dbox * 1.05), (pos, dbox)]
    eager = [tuple(t.detach().clone() for t in model(z, p.clone(), batch, box=b)) for p, b in cells]
    gm = GraphedEnergyForces(model, z, pos, batch, box=box)
    try:
        assert gm.box.shape == (1, 3, 3) and model.prior_model[0].cell_bound is None
        for (p, b), (y_e, f_e) in zip(cells, eager):
            y_g, f_g = gm(p, box=b)
            gm.check_capacity()
            assert _rel(y_g, y_e) < 1e-5 and _rel(f_g, f_e) < 1e-5
    finally:
        gm.release()


def test_a_five_argument_prior_keeps_working():
    from torchmdnet.priors.base import BasePrior

    class Shift(BasePrior):
        def post_reduce(self, y, z, pos, batch, extra_args):
            return y + 1.5

    z, pos, batch, boxes = _batch(torch.float32)
    model = _model(32, dict(periodic=True))
    y0, _ = model(z, pos.clone(), batch, box=boxes)
    model.prior_model.append(Shift())
    y1, _ = model(z, pos.clone(), batch, box=boxes)
    assert torch.allclose(y1, y0 + 1.5, rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- virial and stress
def _prior_virial(prior, z, pos, batch, n_mol, box, create_graph=False):
    """(y, neg_dy, W) of the prior alone, as TorchMD_Net.energy_forces_virial forms them: the force pass is seeded
    with -1 inside a virial sink."""
    from torchmdnet import kernels
    p = pos if pos.requires_grad else pos.detach().clone().requires_grad_(True)
    with kernels.virial_sink(n_mol, batch, pos.dtype, differentiable=create_graph) as sink:
        w = sink.out
        y = _prior_energy(prior, z, batch, n_mol, box)(p)
        f, = torch.autograd.grad([y], [p], grad_outputs=[torch.full_like(y, -1.0)], create_graph=True)
        assert sink.attached == 1
        if create_graph:
            w = sink.total()
    return y, f, w


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_virial_is_the_strain_derivative_of_the_restatement(kind, dtype):
    """W[m] = -dE_m/d eps of the restatement under pos -> pos (I + eps)^T, box -> box (I + eps)^T, exact in float64
    by autograd; the open molecule's is sum F (x) pos; detached and create_graph=True give the same values."""
    z, pos, batch, boxes = _batch(dtype)
    prior = _prior(kind)
    _, f, w = _prior_virial(prior, z, pos, batch, N_MOL, boxes)
    _, _, w_cg = _prior_virial(prior, z, pos, batch, N_MOL, boxes, create_graph=True)
    assert not w.requires_grad and w_cg.requires_grad
    ref = PR.virial(_ref_energy(kind, z, batch, N_MOL, boxes), pos.double().cpu()).detach()
    _check([w.double().cpu(), w_cg.detach().double().cpu()], [ref, ref], dtype, f"{kind} virial",
           names=("virial", "virial (create_graph)"))
    idx = (batch == OM.OPEN).nonzero().flatten()
    own = (f.detach().double()[idx].T @ pos.double()[idx]).cpu()
    _check([w[OM.OPEN].double().cpu()], [own], dtype, f"{kind} open molecule", names=("sum F (x) pos",))
    assert float(w[3].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_stress_loss_gradient_reaches_the_positions(kind, dtype):
    """d/dpos of sum((W - W_label)^2) + sum(neg_dy^2) through create_graph=True (the neighbour op's second order
    with the virial's cotangent) against the same loss on the restatement, differentiated by autograd in float64
    as tests/stress_ref.py differentiates the oracle's."""
    z, pos, batch, boxes = _batch(dtype)
    g = torch.Generator().manual_seed(23)
    label = torch.randn(N_MOL, 3, 3, generator=g, dtype=torch.float64)
    p = pos.detach().clone().requires_grad_(True)
    _, f, w = _prior_virial(_prior(kind), z, p, batch, N_MOL, boxes, create_graph=True)
    scale = float(w.detach().abs().max())
    loss = ((w / scale - label.to(DEV, dtype)) ** 2).sum() + (f ** 2).sum() / scale ** 2
    got, = torch.autograd.grad(loss, p)
    q = pos.double().cpu().requires_grad_(True)
    e = _ref_energy(kind, z, batch, N_MOL, boxes)
    w_ref = PR.virial(e, q)
    f_ref, = torch.autograd.grad(-e(q).sum(), q, create_graph=True)
    loss_ref = ((w_ref / scale - label) ** 2).sum() + (f_ref ** 2).sum() / scale ** 2
    ref, = torch.autograd.grad(loss_ref, q)
    _check([loss.detach().double().cpu().reshape(1), got.double().cpu()], [loss_ref.detach().reshape(1), ref], dtype,
           f"{kind} stress loss", names=("loss", "d loss / d pos"))


# ----------------------------------------------------------------------------- strategy
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("m", [0, 2], ids=["diagonal", "skewed"])
@pytest.mark.parametrize("kind", KINDS)
def test_cell_strategy_equals_brute(kind, m, dtype):
    z, pos, batch, box = _molecule(dtype, m)
    brute, cell = _prior(kind), _prior(kind, neighbor_strategy="cell")
    ref = _ref_orders(kind, dtype, str(m))
    a = _orders(_prior_energy(brute, z, batch, 1, box), pos)
    b = _orders(_prior_energy(cell, z, batch, 1, box), pos)
    assert int(brute.last_num_pairs) == int(cell.last_num_pairs) > 0
    _check(a, ref, dtype, f"{kind} brute")
    _check(b, ref, dtype, f"{kind} cell")
    # the device box (1, 3, 3) of the cell list, read back with its checks
    c = _orders(_prior_energy(cell, z, batch, 1, box.to(DEV).reshape(1, 3, 3)), pos)
    _check(c, ref, dtype, f"{kind} cell, device box")
    # without a box the strategy is not used: the non-periodic list is the all-pairs one
    _same_evaluation(_prior_energy(cell, z, batch, 1, None),
                     _prior_energy(_prior(kind, periodic=False), z, batch, 1, None), pos)


# ----------------------------------------------------------------------------- capture
def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("strategy", ["brute", "cell"])
def test_captured_replay_follows_a_new_box(strategy):
    """GraphedEnergyForces(..., box=): a replay with the box and the positions scaled by 1.05 equals the eager call
    at the new box.  Default prior: the whole batch, per-molecule boxes (the open one stays zero); ``"cell"``: the
    rectangular molecule alone in its one box, with the prior's cell bound set and cleared with the capture."""
    from torchmdnet.graphs import GraphedEnergyForces
    model = _model(32, dict(periodic=True, neighbor_strategy=strategy))
    prior = model.prior_model[0]
    if strategy == "cell":
        z, pos, batch, box = _molecule(torch.float32, 0)
    else:
        z, pos, batch, box = _batch(torch.float32)
    cells = [(pos * 1.05, box * 1.05), (pos, box)]
    eager = [tuple(t.detach().clone() for t in model(z, p.clone(), batch, box=b)) for p, b in cells]
    bare = _model(32)
    y_bare, _ = bare(z, pos.clone(), batch, box=box)
    assert _rel(eager[1][0], y_bare) > 1e-3  # the prior is not a rounding error here
    gm = GraphedEnergyForces(model, z, pos, batch, box=box)
    try:
        assert len(gm.priors) == 1 and prior.static_capacity % 256 == 0
        assert (prior.cell_bound is not None) == (strategy == "cell")
        if strategy == "cell":
            assert torch.equal(prior.cell_bound, box.double() * 1.25)
        for (p, b), (y_e, f_e) in zip(cells, eager):
            y, f = gm(p, box=b)
            gm.check_capacity()
            assert _rel(y, y_e) < 1e-5 and _rel(f, f_e) < 1e-5
    finally:
        gm.release()
    assert prior.static_capacity is None and prior.cell_bound is None
    # release() clears the bounds the constructor set, not one the user put on a prior for eager device-box calls
    if strategy == "brute":
        mine = box.reshape(-1, 3, 3)[0].double().cpu() * 2.0
        prior.cell_bound = mine
        GraphedEnergyForces(model, z, pos, batch, box=box).release()
        assert prior.cell_bound is mine
        prior.cell_bound = None
    # each prior keeps its own capacity and flag: one below its pair count is named by check_capacity
    gs = GraphedEnergyForces(model, z, pos, batch, box=box, prior_capacity=256)
    try:
        gs(pos)
        with pytest.raises(RuntimeError, match="ZBL prior"):
            gs.check_capacity()
    finally:
        gs.release()


def test_captured_training_with_a_periodic_prior_stays_refused():
    from torchmdnet.training import GraphedTrainStep
    z, pos, batch, _ = _batch(torch.float32)
    model = _model(32, dict(periodic=True))
    with pytest.raises(ValueError, match="LNNPStep"):
        GraphedTrainStep(model, z, pos, batch, torch.zeros(N_MOL, 1, device=DEV), torch.zeros(len(z), 3, device=DEV))


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.priors import Coulomb
    with pytest.raises(ValueError, match="infinite cutoff"):
        Coulomb(0.3, 40, periodic=True, **SCALES)
    z, pos, batch, boxes = _batch(torch.float64)
    y0 = torch.zeros(N_MOL, 1, dtype=torch.float64, device=DEV)
    # the box checks run with the prior's own cutoff: 3.6 needs 7.2, the boxes are 7.0 and up
    with pytest.raises(RuntimeError, match=r"molecule 0: Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"):
        _prior("zbl", cutoff=3.6).post_reduce_box(y0, z, pos, batch, None, boxes)
    zm, pm, bm, box = _molecule(torch.float64, 0)
    with pytest.raises(RuntimeError, match=r"Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"):
        _prior("d2", cutoff=3.6).post_reduce_box(y0[:1], zm, pm, bm, None, box)
    # the cell list takes one box
    with pytest.raises(RuntimeError, match="brute and shared"):
        _prior("zbl", neighbor_strategy="cell").post_reduce_box(y0, z, pos, batch, None, boxes)
    model = _model(32, dict(periodic=True, neighbor_strategy="cell"))
    with pytest.raises(RuntimeError, match="brute and shared"):
        GraphedEnergyForces(model, z, pos.float(), batch, box=boxes)
    assert model.prior_model[0].cell_bound is None and model.prior_model[0].static_capacity is None
    # one (3, 3) box over several molecules beside a model on brute: the limit is named, not the per-molecule error
    with pytest.raises(RuntimeError, match='neighbor_strategy="cell" is captured with one box.*4 molecules'):
        GraphedEnergyForces(model, z, pos.float(), batch, box=boxes[0].cpu())
    assert model.prior_model[0].cell_bound is None
