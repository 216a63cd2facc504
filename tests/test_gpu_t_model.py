"""GPU tests of the invariant Transformer (models/torchmd_t.py on the scalar message kernels): the reference's
recorded outputs (expected_outputs.json, t_ref.npz), the dense restatement tests/t_ref.py, periodic boxes, the
virial, HIP-graph capture and the TorchScript refusal.

Tolerances (test_gpu_gn.py's): float64 rtol = atol = 1e-9; float32 max|d| <= 1e-4 max|ref|; expected_outputs.json
at test_expected_outputs_graph_network's rtol / atol."""
import json
import os

import numpy as np
import pytest
import torch

import t_ref
from conftest import GOLDEN, golden, yaml_args
from test_gpu_gn import _close, _np, _quantities, _seed
from test_t_cpu import _case
from torchmdnet._native import ET_SCALAR  # noqa: F401  (the feature: this module fails at import without it)
from torchmdnet.models.model import create_transformer_model

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("head", ["Scalar", "DipoleMoment", "ElectronicSpatialExtent"])
def test_expected_outputs_transformer(head):
    exp = json.load(open(os.path.join(GOLDEN, "expected_outputs.json")))["transformer"][head]
    _seed()
    m = create_transformer_model(yaml_args("transformer", output_model=head, derivative=head == "Scalar"))
    zs = torch.tensor([1, 6, 7, 8, 9], dtype=torch.long)
    z = zs[torch.randint(0, len(zs), (5,))]
    pos = torch.randn(len(z), 3)
    batch = torch.zeros(len(z), dtype=torch.long)
    batch[len(batch) // 2:] = 1
    m = m.to(DEV)
    y, neg_dy = m(z.to(DEV), pos.to(DEV), batch.to(DEV))
    assert np.allclose(_np(y).ravel(), exp["pred"]["values"], rtol=1e-4, atol=1e-5), head
    if exp["deriv"] is not None:
        assert np.allclose(_np(neg_dy).ravel(), exp["deriv"]["values"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_reference_fixture(name, dtype):
    """Every stored quantity of every case: y, forces, d(sum F^2)/dpos and every parameter gradient of
    sum y + sum F^2 (through the message kernels' second order)."""
    d = golden("t_ref.npz")
    args, sd, gp_ref = _case(d, name)
    args["precision"] = 64 if dtype == torch.float64 else 32
    model = create_transformer_model(args)
    model.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    model = model.to(DEV)
    z, batch = torch.tensor(d["z"], device=DEV), torch.tensor(d["batch"], device=DEV)
    pos = torch.tensor(d["pos"], device=DEV).to(dtype)
    y, f, h, gp = _quantities(model, z, pos, batch)
    _close(_np(y), d[name + "/y"], dtype, f"{name} y")
    _close(_np(f), d[name + "/forces"], dtype, f"{name} forces")
    _close(_np(h), d[name + "/dF2"], dtype, f"{name} dF2")
    for k, ref in gp_ref.items():
        if np.abs(ref).max() == 0:
            assert float(gp[k].abs().max()) == 0, k
        else:
            _close(_np(gp[k]), ref, dtype, f"{name} gp/{k}")


def _outside_input():
    """40 atoms in two molecules."""
    gen = torch.Generator().manual_seed(7)
    z = torch.tensor([1, 6, 7, 8])[torch.randint(0, 4, (40,), generator=gen)]
    pos = torch.randn(40, 3, generator=gen, dtype=torch.float64) * 1.5
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor([23, 17]))
    return z, pos, batch


def _args(**kw):
    base = dict(embedding_dimension=64, num_heads=8, num_layers=2, num_rbf=16, derivative=True,
                output_model="Scalar", precision=64, max_z=10, max_num_neighbors=64)
    base.update(kw)
    return yaml_args("transformer", **base)


def _model(seed=11, **kw):
    torch.manual_seed(seed)
    args = _args(**kw)
    return args, create_transformer_model(args)


def test_outside_fixture_against_restatement():
    args, model = _model()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    z, pos, batch = _outside_input()
    p = pos.clone().requires_grad_(True)
    y_ref = t_ref.energy(sd, args, z, p, batch)
    f_ref, = torch.autograd.grad(-y_ref.sum(), p)
    model = model.to(DEV)
    y, f = model(z.to(DEV), pos.to(DEV), batch.to(DEV))
    _close(_np(y), _np(y_ref), torch.float64, "y")
    _close(_np(f), _np(f_ref), torch.float64, "forces")


@pytest.mark.parametrize("per_molecule", [False, True], ids=["one-box", "box-per-molecule"])
def test_wrap_invariance_under_a_box(per_molecule):
    """A cubic box of edge 3 x cutoff: shifting some atoms by box vectors changes nothing; the energy differs from
    the open evaluation."""
    args, model = _model()
    model = model.to(DEV)
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    L = 3.0 * float(args["cutoff_upper"])
    box = L * torch.eye(3, dtype=torch.float64, device=DEV)
    if per_molecule:
        box = torch.stack([box, box])
    y0, f0 = model(z, pos.clone(), batch, box=box)
    gen = torch.Generator().manual_seed(5)
    shift = L * torch.randint(-2, 3, (40, 3), generator=gen).to(torch.float64).to(DEV)
    shift[::3] = 0
    y1, f1 = model(z, (pos + shift).clone(), batch, box=box)
    _close(_np(y1), _np(y0), torch.float64, "wrapped y")
    _close(_np(f1), _np(f0), torch.float64, "wrapped forces")
    # the spread-out copy differs from its open evaluation (the box joins what the shifts pulled apart)
    y_open, _ = model(z, (pos + shift).clone(), batch)
    assert float((y_open - y1).abs().max()) > 1e-3


def test_virial_without_a_box():
    args, model = _model()
    model = model.to(DEV)
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    y, f, w = model.energy_forces_virial(z, pos.clone(), batch)
    ref = torch.zeros(2, 3, 3, dtype=torch.float64, device=DEV).index_add(
        0, batch, f.detach().unsqueeze(2) * pos.unsqueeze(1))
    _close(_np(w), _np(ref), torch.float64, "virial")


def test_graphed_replay_equals_eager():
    from torchmdnet.graphs import GraphedEnergyForces
    args, model = _model(precision=32)
    model = model.to(DEV)
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    pos = pos.float()
    gm = GraphedEnergyForces(model, z, pos, batch)
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y, f = gm(moved)
    gm.check_capacity()
    y, f = y.clone(), f.clone()
    gm.release()
    y_e, f_e = model(z, moved.clone(), batch)
    _close(_np(y), _np(y_e), torch.float32, "graphed y")
    _close(_np(f), _np(f_e), torch.float32, "graphed forces")


def test_training_step_with_a_force_loss():
    """LNNPStep, eager, force loss: the parameter gradients against autograd through the restatement (float64)."""
    from torchmdnet.training import LNNPStep
    args, model = _model()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    z, pos, batch = _outside_input()
    gen = torch.Generator().manual_seed(9)
    y_l = torch.randn(2, 1, generator=gen, dtype=torch.float64)
    f_l = torch.randn(40, 3, generator=gen, dtype=torch.float64)
    p = pos.clone().requires_grad_(True)
    y_ref = t_ref.energy(sd, args, z, p, batch)
    f_ref, = torch.autograd.grad(-y_ref.sum(), p, create_graph=True)
    loss_ref = torch.nn.functional.mse_loss(y_ref, y_l) + torch.nn.functional.mse_loss(f_ref, f_l)
    names = [k for k, _ in model.named_parameters()]
    g_ref = torch.autograd.grad(loss_ref, [sd[k] for k in names], allow_unused=True)
    model = model.to(DEV)
    tr = LNNPStep(model, lr=0.0, y_weight=1.0, neg_dy_weight=1.0)
    loss = tr.loss(z.to(DEV), pos.to(DEV), batch.to(DEV), y_l.to(DEV), f_l.to(DEV))
    loss.backward()
    _close(_np(loss), _np(loss_ref), torch.float64, "loss")
    for k, g in zip(names, g_ref):
        got = dict(model.named_parameters())[k].grad
        if g is None or float(g.abs().max()) == 0:
            assert got is None or float(got.abs().max()) == 0, k
        else:
            _close(_np(got), _np(g), torch.float64, f"grad {k}")


def test_atomref_prior():
    """Atomref on top of the Transformer: the model without priors plus the per-atom offsets, same forces."""
    from torchmdnet.priors import Atomref
    args, model = _model()
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    with_prior = create_transformer_model(_args(), prior_model=Atomref(max_z=10))
    with_prior.load_state_dict(model.state_dict(), strict=False)
    with torch.no_grad():
        with_prior.prior_model[0].atomref.weight.copy_(0.1 * torch.arange(10, dtype=torch.float64).view(10, 1))
    model, with_prior = model.to(DEV), with_prior.to(DEV)
    y0, f0 = model(z, pos.clone(), batch)
    y1, f1 = with_prior(z, pos.clone(), batch)
    shift = torch.zeros(2, 1, dtype=torch.float64, device=DEV).index_add(0, batch, (0.1 * z.double()).unsqueeze(1))
    _close(_np(y1), _np(y0 + shift), torch.float64, "atomref y")
    _close(_np(f1), _np(f0), torch.float64, "atomref forces")


def test_zbl_pair_prior():
    """ZBL on top of the Transformer: the model without priors plus the restatement's ZBL energy and forces
    (tests/pair_prior_ref.py, which has no self loops: the prior builds its own list, whatever the model's)."""
    import pair_prior_ref as R
    from torchmdnet.priors import ZBL
    scales = dict(distance_scale=1e-10, energy_scale=4.35974e-18)
    numbers = list(range(100))
    args, model = _model()
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    with_prior = create_transformer_model(_args(), prior_model=ZBL(5.0, 40, atomic_number=numbers, **scales))
    with_prior.load_state_dict(model.state_dict(), strict=False)
    model, with_prior = model.to(DEV), with_prior.to(DEV)
    y0, f0 = model(z, pos.clone(), batch)
    y1, f1 = with_prior(z, pos.clone(), batch)
    p = pos.clone().requires_grad_(True)
    e = R.zbl_energy(p, z, batch, 2, 5.0, numbers, **scales).reshape(2, 1)
    fe, = torch.autograd.grad(-e.sum(), p)
    assert float(e.abs().min()) > 1e-3  # ZBL is not a rounding error on this input
    _close(_np(y1), _np(y0 + e), torch.float64, "zbl y")
    _close(_np(f1), _np(f0 + fe), torch.float64, "zbl forces")


def test_torchscript_is_refused():
    _, model = _model(precision=32)
    with pytest.raises(RuntimeError, match="runs eagerly"):
        torch.jit.script(model.to(DEV))
