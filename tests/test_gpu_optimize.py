"""GPU tests of ``optimize(model)`` (the graph network on ``kernels.cfconv_fused``) and of ``calculators.External``.

References: the dense float64 restatement tests/gn_ref.py on the same weights, the unoptimized float32 model, and
the reference's recorded outputs (gn_ref.npz).  Tolerance (the project's): float32 max|d| <= 1e-4 max|ref|."""
import copy

import numpy as np
import pytest
import torch

import gn_ref
from conftest import golden, yaml_args
from test_gn_cpu import _case

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _close(a, ref, what):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d, top = np.abs(a - ref).max(), np.abs(ref).max()
    print(f"{what}: max|d| = {d:.3e}, max|ref| = {top:.3e}")
    assert d <= 1e-4 * top, what


def _np(t):
    return t.detach().cpu().numpy()


def _small_args(**kw):
    base = dict(embedding_dimension=32, num_layers=2, num_rbf=16, aggr="add", derivative=True,
                output_model="Scalar", precision=32, max_z=10)
    base.update(kw)
    return yaml_args("graph-network", **base)


def _pair(args, seed=11):
    """(unoptimized, optimized) float32 models on the GPU carrying the same weights, and their state_dict."""
    from torchmdnet.models.model import create_model
    from torchmdnet.optimize import optimize
    torch.manual_seed(seed)
    plain = create_model(args)
    sd = {k: v.detach().clone() for k, v in plain.state_dict().items()}
    fused = optimize(copy.deepcopy(plain))
    return plain.to(DEV), fused.to(DEV), sd


def _reference(sd, args, z, pos, batch):
    p = pos.double().clone().requires_grad_(True)
    y = gn_ref.energy(sd, args, z, p, batch)
    f, = torch.autograd.grad(-y.sum(), p)
    return _np(y), _np(f)


def _molecules():
    """40 atoms, 4 molecules, the last one a single atom (row length 0)."""
    gen = torch.Generator().manual_seed(7)
    z = torch.tensor([1, 6, 7, 8])[torch.randint(0, 4, (40,), generator=gen)]
    pos = (torch.randn(40, 3, generator=gen, dtype=torch.float64) * 1.5).float()
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor([17, 13, 9, 1]))
    return z, pos, batch


@pytest.mark.parametrize("num_atoms", [10, 100])
def test_reference_optimize_configuration(num_atoms):
    """The reference's tests/test_optimize.py model and inputs."""
    args = yaml_args("graph-network", embedding_dimension=128, num_layers=6, num_rbf=50, rbf_type="gauss",
                     trainable_rbf=False, activation="ssp", neighbor_embedding=False, cutoff_lower=0.0,
                     cutoff_upper=5.0, max_z=100, max_num_neighbors=num_atoms, aggr="add", derivative=True,
                     atom_filter=-1, output_model="Scalar", reduce_op="add", precision=32)
    gen = torch.Generator().manual_seed(num_atoms)
    z = torch.randint(1, 100, (num_atoms,), generator=gen)
    pos = 10 * torch.rand((num_atoms, 3), generator=gen) - 5
    batch = torch.zeros(num_atoms, dtype=torch.long)
    plain, fused, sd = _pair(args, seed=5)
    y_ref, f_ref = _reference(sd, args, z, pos, batch)
    y_p, f_p = plain(z.to(DEV), pos.to(DEV))
    y, f = fused(z.to(DEV), pos.to(DEV))
    _close(_np(y), y_ref, f"N={num_atoms} y vs float64")
    _close(_np(f), f_ref, f"N={num_atoms} forces vs float64")
    _close(_np(y), _np(y_p), f"N={num_atoms} y vs unoptimized")
    _close(_np(f), _np(f_p), f"N={num_atoms} forces vs unoptimized")


@pytest.mark.parametrize("name", ["a", "b"])
def test_reference_fixture_optimized(name):
    """gn_ref.npz: a = add, neighbour embedding, expnorm; b = mean, gauss, cutoff_lower 1.0."""
    from torchmdnet.models.model import create_model
    from torchmdnet.optimize import optimize
    d = golden("gn_ref.npz")
    args, sd, _ = _case(d, name)
    args["precision"] = 32
    model = create_model(args)
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    model = optimize(model).to(DEV)
    z, batch = torch.tensor(d["z"], device=DEV), torch.tensor(d["batch"], device=DEV)
    pos = torch.tensor(d["pos"], device=DEV).float().requires_grad_(True)
    y, _ = model(z, pos, batch)   # (the fixture's models are built without the derivative)
    f, = torch.autograd.grad(-y.sum(), pos)
    _close(_np(y), d[name + "/y"], f"{name} y")
    _close(_np(f), d[name + "/forces"], f"{name} forces")


@pytest.mark.parametrize("kw", [dict(aggr="add"), dict(aggr="mean", activation="ssp", rbf_type="gauss"),
                                dict(aggr="add", neighbor_embedding=False, trainable_rbf=True, cutoff_lower=0.5)],
                         ids=["add", "mean-ssp-gauss", "no-nbr-trainable-cl"])
def test_multi_molecule_batch(kw):
    args = _small_args(**kw)
    plain, fused, sd = _pair(args)
    z, pos, batch = _molecules()
    y_ref, f_ref = _reference(sd, args, z, pos, batch)
    y, f = fused(z.to(DEV), pos.to(DEV), batch.to(DEV))
    assert y.shape == (4, 1) and f.shape == (40, 3)
    _close(_np(y), y_ref, "y vs float64")
    _close(_np(f), f_ref, "forces vs float64")
    y_p, f_p = plain(z.to(DEV), pos.to(DEV), batch.to(DEV))
    _close(_np(y), _np(y_p), "y vs unoptimized")
    _close(_np(f), _np(f_p), "forces vs unoptimized")
    # the frozen filter networks get no gradient, everything else does
    y.sum().backward()
    for n, p in fused.named_parameters():
        if ".mlp." in n or ".distance_expansion." in n:
            assert p.grad is None, n
    assert fused.representation_model.model.interactions[0].conv.lin1.weight.grad is not None


def _new_weights(models, seed=2):
    gen = torch.Generator().manual_seed(seed)
    w = models[0].representation_model.interactions[1].mlp[2].weight
    new = (0.3 * torch.randn(w.shape, generator=gen)).to(DEV)
    for m in models:
        rep = m.representation_model
        rep = getattr(rep, "model", rep)
        rep.interactions[1].mlp[2].weight.data.copy_(new)


def test_weights_are_read_live():
    plain, fused, _ = _pair(_small_args())
    z, pos, batch = (t.to(DEV) for t in _molecules())
    y0, f0 = fused(z, pos.clone(), batch)
    _new_weights([plain, fused])
    y1, f1 = fused(z, pos.clone(), batch)
    y_p, f_p = plain(z, pos.clone(), batch)
    assert float((f1 - f0).detach().abs().max()) > 1e-3 * float(f0.detach().abs().max()), "the new weights changed nothing"
    _close(_np(y1), _np(y_p), "y after the update")
    _close(_np(f1), _np(f_p), "forces after the update")


def test_graphed_replay_equals_eager_and_reads_live_weights():
    from torchmdnet.graphs import GraphedEnergyForces
    plain, fused, _ = _pair(_small_args())
    z, pos, batch = (t.to(DEV) for t in _molecules())
    gm = GraphedEnergyForces(fused, z, pos, batch)
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y, f = gm(moved)
    gm.check_capacity()
    y, f = y.clone(), f.clone()
    _new_weights([plain, fused])
    y2, f2 = gm(moved)
    gm.check_capacity()
    y2, f2 = y2.clone(), f2.clone()
    gm.release()
    y_p, f_p = plain(z, moved.clone(), batch)      # the new weights
    _close(_np(y2), _np(y_p), "replay after the update: y")
    _close(_np(f2), _np(f_p), "replay after the update: forces")
    assert float((f2 - f).detach().abs().max()) > 1e-3 * float(f.detach().abs().max()), "the replay kept the old weights"
    y_e, f_e = fused(z, moved.clone(), batch)
    _close(_np(y2), _np(y_e), "graphed y vs eager optimized")
    _close(_np(f2), _np(f_e), "graphed forces vs eager optimized")


def test_optimized_models_are_inference_only():
    from torchmdnet.training import LNNPStep
    _, fused, _ = _pair(_small_args())
    z, pos, batch = (t.to(DEV) for t in _molecules())
    p = pos.clone().requires_grad_(True)
    y, f = fused(z, p, batch)
    with pytest.raises(RuntimeError, match="inference-only"):
        torch.autograd.grad((f ** 2).sum(), p)
    step = LNNPStep(fused, lr=1e-4)
    with pytest.raises(RuntimeError, match="inference-only"):
        step.step(z, pos.clone(), batch, torch.zeros(4, 1, device=DEV), torch.zeros(40, 3, device=DEV))
    with pytest.raises(RuntimeError, match="runs eagerly"):
        torch.jit.script(fused)


# ----------------------------------------------------------------------------- External
def _checkpoint(path):
    from torchmdnet.models.model import create_model
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                     max_z=10, derivative=False)
    torch.manual_seed(3)
    model = create_model(args)
    torch.save({"state_dict": {"model." + k: v for k, v in model.state_dict().items()}, "hyper_parameters": args},
               path)
    return str(path)


def _molecule(seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.tensor([1, 6, 7, 8])[torch.randint(0, 4, (6,), generator=gen)]
    return z, torch.randn(6, 3, generator=gen)


def test_external_compare_forward(tmp_path):
    from torchmdnet.calculators import External
    from torchmdnet.models.model import load_model
    ckpt = _checkpoint(tmp_path / "et.ckpt")
    z, pos = _molecule(0)
    calc = External(ckpt, z.unsqueeze(0), device=DEV)
    model = load_model(ckpt, derivative=True, device=DEV)
    e_calc, f_calc = calc.calculate(pos, None)
    e_pred, f_pred = model(z.to(DEV), pos.to(DEV))
    assert e_calc.shape == (1, 1) and f_calc.shape == (1, 6, 3)
    assert not e_calc.requires_grad and not f_calc.requires_grad
    _close(_np(e_calc), _np(e_pred), "energy")
    _close(_np(f_calc), _np(f_pred.unsqueeze(0)), "forces")
    scaled = External(ckpt, z.unsqueeze(0), device=DEV, output_transform="Hartree/Bohr -> kcal/mol/A")
    e_s, f_s = scaled.calculate(pos, None)
    _close(_np(e_s), _np(e_calc) * 627.509, "preset energy")
    _close(_np(f_s), _np(f_calc) * 627.509 / 0.529177, "preset forces")


def test_external_compare_forward_multiple(tmp_path):
    from torchmdnet.calculators import External
    from torchmdnet.models.model import load_model
    ckpt = _checkpoint(tmp_path / "et.ckpt")
    (z1, pos1), (z2, pos2) = _molecule(1), _molecule(2)
    calc = External(ckpt, torch.stack([z1, z2], dim=0), device=DEV)
    model = load_model(ckpt, derivative=True, device=DEV)
    e_calc, f_calc = calc.calculate(torch.cat([pos1, pos2], dim=0), None)
    e_pred, f_pred = model(torch.cat([z1, z2]).to(DEV), torch.cat([pos1, pos2], dim=0).to(DEV),
                           torch.cat([torch.zeros(len(z1)), torch.ones(len(z2))]).long().to(DEV))
    assert e_calc.shape == (2, 1) and f_calc.shape == (2, 6, 3)
    _close(_np(e_calc), _np(e_pred), "energy")
    _close(_np(f_calc), _np(f_pred.view(-1, len(z1), 3)), "forces")
