"""CPU tests of the graph-network model: the dense restatement (tests/gn_ref.py) against the reference's recorded
results (tests/golden/gn_ref.npz, from tests/golden/gen_gn_fixtures.py), the cfconv composite, and the
construction contract (state_dict keys, checkpoints, refusals)."""
import json

import numpy as np
import pytest
import torch

import gn_ref
from conftest import golden

CASES = ["a", "b", "c", "d"]


def _case(d, name):
    args = json.loads(str(d[name + "/args"]))
    sd = {k[len(name) + 4:]: torch.tensor(d[k]) for k in d.files if k.startswith(name + "/sd/")}
    gp = {k[len(name) + 4:]: d[k] for k in d.files if k.startswith(name + "/gp/")}
    return args, sd, gp


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    """Every stored quantity, float64, gated at 1e-10 of the largest entry (no float32 step in the reference's
    graph network forces a looser gate)."""
    d = golden("gn_ref.npz")
    args, sd, gp = _case(d, name)
    z, batch = torch.tensor(d["z"]), torch.tensor(d["batch"])
    pos = torch.tensor(d["pos"]).requires_grad_(True)
    sd = {k: (v.clone().requires_grad_(True) if k in gp else v) for k, v in sd.items()}
    y = gn_ref.energy(sd, args, z, pos, batch)
    f, = torch.autograd.grad(-y.sum(), pos, create_graph=True)
    f2 = (f ** 2).sum()
    h, = torch.autograd.grad(f2, pos, retain_graph=True)
    keys = list(gp)
    grads = torch.autograd.grad(y.sum() + f2, [sd[k] for k in keys], allow_unused=True)
    errs = {"y": _rel(y.detach(), d[name + "/y"]), "forces": _rel(f.detach(), d[name + "/forces"]),
            "dF2": _rel(h, d[name + "/dF2"])}
    for k, g in zip(keys, grads):
        ref = gp[k]
        if np.abs(ref).max() == 0:
            assert g is None or float(g.abs().max()) == 0, k
            continue
        errs["gp/" + k] = _rel(g.detach(), ref)
    for k, e in errs.items():
        print(f"case {name} {k}: {e:.3e}")
    assert max(errs.values()) < 1e-10, errs


def test_max_case_winners_are_float32_proof():
    """The max fixture's condition on its input (gen_gn_fixtures.py): in every layer the two largest messages of
    every (atom, channel) differ by at least 1e-4 of the larger one, far above float32's error on a message, so a
    float32 evaluation picks the float64 winners.  Recomputed here from the stored state_dict."""
    d = golden("gn_ref.npz")
    args, sd, _ = _case(d, "c")
    inputs = (torch.tensor(d["z"]), torch.tensor(d["pos"]), torch.tensor(d["batch"]))
    gaps = gn_ref.top2_pair_gaps(sd, args, *inputs)
    print("top-two pair gaps per layer", gaps, "stored", float(d["c/top2_pair_gap"]),
          "; relative to the layer maximum", gn_ref.top2_gaps(sd, args, *inputs))
    assert min(gaps) >= 1e-4
    assert min(gaps) == pytest.approx(float(d["c/top2_pair_gap"]), rel=1e-6)


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
def test_cfconv_composite_matches_three_line_form(aggr):
    from torchmdnet.kernels import EdgeGraph, cfconv, cfconv_composite
    gen = torch.Generator().manual_seed(0)
    n, nf = 6, 5
    ei = torch.tensor([[0, 1, 1, 2, 0, 3, 2, 2], [1, 0, 2, 1, 3, 0, 2, 4]])  # a self loop; atom 5 has no edge
    E = ei.shape[1]
    h = torch.randn(n, nf, generator=gen, dtype=torch.float64)
    w = torch.randn(E, nf, generator=gen, dtype=torch.float64)
    C = torch.rand(E, generator=gen, dtype=torch.float64)
    m = h[ei[0]] * w * C[:, None]
    if aggr == "max":
        ref = torch.stack([m[ei[1] == t].amax(0) if (ei[1] == t).any() else torch.zeros(nf, dtype=m.dtype)
                           for t in range(n)])
    else:
        ref = torch.zeros(n, nf, dtype=m.dtype).index_add(0, ei[1], m)
        if aggr == "mean":
            ref = ref / torch.bincount(ei[1], minlength=n).clamp(min=1)[:, None]
    assert torch.allclose(cfconv_composite(h, w, C, ei[0], ei[1], n, aggr), ref, rtol=1e-14, atol=1e-14)
    g, perm = EdgeGraph.from_edge_index(ei, n)  # the public op on CPU tensors takes the composite
    assert torch.allclose(cfconv(h, w[perm], C[perm], g, aggr), ref, rtol=1e-14, atol=1e-14)
    with pytest.raises(ValueError):
        cfconv(h, w[perm], C[perm], g, "min")


@pytest.mark.parametrize("name", CASES)
def test_construction_contract(name, tmp_path):
    from torchmdnet.models.model import create_model, load_model
    d = golden("gn_ref.npz")
    args, sd, gp = _case(d, name)
    model = create_model(dict(args))
    assert set(model.state_dict()) == set(sd)
    assert set(dict(model.named_parameters())) == set(gp)
    model.load_state_dict(sd, strict=True)
    assert model.fused_eval is False
    path = str(tmp_path / "gn.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(args)}, path)
    loaded = load_model(path)
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_seeded_initialisation_matches_reference():
    from torchmdnet.models.model import create_model
    d = golden("gn_ref.npz")
    for name in ("a", "b"):
        args, sd, _ = _case(d, name)
        torch.manual_seed(int(d[name + "/seed"]))
        model = create_model(dict(args))
        for k, v in model.state_dict().items():
            assert torch.allclose(v, sd[k], rtol=0, atol=1e-15), (name, k)


def test_refusals():
    from conftest import yaml_args
    from torchmdnet.models.model import create_model
    from torchmdnet.models.torchmd_gn import TorchMD_GN
    with pytest.raises(AssertionError, match="aggr"):
        TorchMD_GN(hidden_channels=8, num_filters=8, num_layers=1, num_rbf=4, aggr="min")
    with pytest.raises(NotImplementedError):
        create_model(yaml_args("transformer"))
    with pytest.raises(ValueError, match="atom filter"):
        create_model(yaml_args("graph-network", derivative=True, atom_filter=1))


def test_atom_filter_on_stub_model():
    from torchmdnet.models.wrappers import AtomFilter, BaseWrapper

    class Stub(torch.nn.Module):
        def forward(self, z, pos, batch=None, q=None, s=None):
            return pos.sum(1, keepdim=True) * 2, pos[:, None, :].expand(-1, 3, -1), z, pos, batch

    f = AtomFilter(Stub(), 1)
    assert isinstance(f, BaseWrapper)
    z = torch.tensor([1, 6, 1, 8, 1])
    pos = torch.arange(15, dtype=torch.float32).view(5, 3)
    batch = torch.tensor([0, 0, 0, 1, 1])
    x, v, z2, pos2, batch2 = f(z, pos, batch)
    keep = torch.tensor([1, 3])
    assert torch.equal(z2, z[keep]) and torch.equal(pos2, pos[keep]) and torch.equal(batch2, batch[keep])
    assert torch.equal(x, pos[keep].sum(1, keepdim=True) * 2) and v.shape == (2, 3, 3)
    with pytest.raises(AssertionError, match="completely filtered out"):
        f(torch.tensor([1, 6, 1, 1, 1]), pos, batch)
