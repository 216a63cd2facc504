"""GPU tests of the graph-network model (models/torchmd_gn.py on tmdnet_cfconv_*): the reference's recorded
outputs (expected_outputs.json, gn_ref.npz) and the dense restatement tests/gn_ref.py.

Tolerances (the project's, tests/test_gpu_pair_priors.py): float64 rtol = atol = 1e-9; float32
max|d| <= 1e-4 max|ref|; expected_outputs.json at test_expected_pkl_on_gpu's rtol / atol."""
import json
import os

import numpy as np
import pytest
import torch

import gn_ref
from conftest import GOLDEN, golden, yaml_args
from test_gn_cpu import _case

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _seed(s=1234):  # test_gpu_parity._seed
    import random
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _close(a, ref, dtype, what):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d, top = np.abs(a - ref).max(), np.abs(ref).max()
    print(f"{what}: max|d| = {d:.3e}, max|ref| = {top:.3e}")
    if dtype == torch.float64:
        assert np.allclose(a, ref, rtol=1e-9, atol=1e-9), what
    else:
        assert d <= 1e-4 * top, what


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("head", ["Scalar", "DipoleMoment", "ElectronicSpatialExtent"])
def test_expected_outputs_graph_network(head):
    from torchmdnet.models.model import create_model
    exp = json.load(open(os.path.join(GOLDEN, "expected_outputs.json")))["graph-network"][head]
    _seed()
    m = create_model(yaml_args("graph-network", output_model=head, derivative=head == "Scalar"))
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


def test_tensornet_secondary_heads_keep_their_own_pre_reduce():
    """DipoleMoment and ElectronicSpatialExtent on a non-equivariant model in float32 on the GPU: the Scalar head's
    fused reduction must not replace a subclass's own per-atom term (expected_outputs.json, tensornet)."""
    from torchmdnet.models.model import create_model
    exp = json.load(open(os.path.join(GOLDEN, "expected_outputs.json")))["tensornet"]
    for head in ("DipoleMoment", "ElectronicSpatialExtent"):
        _seed()
        m = create_model(yaml_args("tensornet", output_model=head, derivative=False))
        zs = torch.tensor([1, 6, 7, 8, 9], dtype=torch.long)
        z = zs[torch.randint(0, len(zs), (5,))]
        pos = torch.randn(len(z), 3)
        batch = torch.zeros(len(z), dtype=torch.long)
        batch[len(batch) // 2:] = 1
        m.representation_model.static_shapes = False  # as test_expected_pkl_on_gpu: the unpadded semantics
        m = m.to(DEV)
        y, _ = m(z.to(DEV), pos.to(DEV), batch.to(DEV))
        assert np.allclose(_np(y).ravel(), exp[head]["pred"]["values"], rtol=1e-4, atol=1e-5), head


def _quantities(model, z, pos, batch):
    """y, forces, d(sum F^2)/dpos and the parameter gradients of sum y + sum F^2 (the fixture's quantities)."""
    pos = pos.clone().requires_grad_(True)
    y, _ = model(z, pos, batch)
    f, = torch.autograd.grad(-y.sum(), pos, create_graph=True)
    f2 = (f ** 2).sum()
    h, = torch.autograd.grad(f2, pos, retain_graph=True)
    params = dict(model.named_parameters())
    gp = torch.autograd.grad(y.sum() + f2, list(params.values()), allow_unused=True)
    return y, f, h, {k: (torch.zeros_like(params[k]) if g is None else g) for k, g in zip(params, gp)}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_reference_fixture(name, dtype):
    """Every stored quantity of every case.  (Case c, max: the fixture's two largest messages of every atom and
    channel differ by at least 1e-4 of the larger one -- asserted by gen_gn_fixtures.py and by
    test_gn_cpu.test_max_case_winners_are_float32_proof -- so float32 picks the float64 winners.)"""
    from torchmdnet.models.model import create_model
    d = golden("gn_ref.npz")
    args, sd, gp_ref = _case(d, name)
    args["precision"] = 64 if dtype == torch.float64 else 32
    model = create_model(args)
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
    """40 atoms, 4 molecules, the last one a single atom (row length 0)."""
    gen = torch.Generator().manual_seed(7)
    sizes = [17, 13, 9, 1]
    z = torch.tensor([1, 6, 7, 8])[torch.randint(0, 4, (40,), generator=gen)]
    pos = torch.randn(40, 3, generator=gen, dtype=torch.float64) * 1.5
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor(sizes))
    return z, pos, batch


def _small_args(aggr, **kw):
    base = dict(embedding_dimension=32, num_layers=2, num_rbf=16, aggr=aggr, derivative=True,
                output_model="Scalar", precision=64, max_z=10)
    base.update(kw)
    return yaml_args("graph-network", **base)


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
def test_outside_fixture_against_restatement(aggr):
    from torchmdnet.models.model import create_model
    torch.manual_seed(11)
    args = _small_args(aggr)
    model = create_model(args)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    z, pos, batch = _outside_input()
    p = pos.clone().requires_grad_(True)
    y_ref = gn_ref.energy(sd, args, z, p, batch)
    f_ref, = torch.autograd.grad(-y_ref.sum(), p)
    model = model.to(DEV)
    y, f = model(z.to(DEV), pos.to(DEV), batch.to(DEV))
    _close(_np(y), _np(y_ref), torch.float64, f"{aggr} y")
    _close(_np(f), _np(f_ref), torch.float64, f"{aggr} forces")


@pytest.mark.parametrize("aggr", ["add", "max"])
def test_graphed_replay_equals_eager(aggr):
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_model
    torch.manual_seed(11)
    args = _small_args(aggr, precision=32)
    model = create_model(args).to(DEV)
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    pos = pos.float()
    gm = GraphedEnergyForces(model, z, pos, batch)
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    y, f = gm(moved)
    gm.check_capacity()
    y, f = y.clone(), f.clone()
    gm.release()
    y_e, f_e = model(z, moved.clone(), batch)
    _close(_np(y), _np(y_e), torch.float32, f"{aggr} graphed y")
    _close(_np(f), _np(f_e), torch.float32, f"{aggr} graphed forces")


def test_graph_capture_refuses_wrapped_model():
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_model
    model = create_model(_small_args("add", derivative=False, atom_filter=1, precision=32)).to(DEV)
    model.derivative = True  # (create_model refuses the pair; the capture must refuse the wrapper by itself)
    z, pos, batch = (t.to(DEV) for t in _outside_input())
    with pytest.raises(ValueError, match="wrapped representation model"):
        GraphedEnergyForces(model, z, pos.float(), batch)


def test_torchscript_is_refused():
    from torchmdnet.models.model import create_model
    model = create_model(_small_args("add", precision=32)).to(DEV)
    with pytest.raises(RuntimeError, match="runs eagerly"):
        torch.jit.script(model)
