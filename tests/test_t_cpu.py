"""CPU tests of the invariant Transformer: the dense restatement (tests/t_ref.py) against the reference's recorded
results (tests/golden/t_ref.npz, from tests/golden/gen_t_fixtures.py), the message composite, and the
construction contract (state_dict keys, checkpoints, seeded initialisation, refusals)."""
import json

import numpy as np
import pytest
import torch

import t_ref
from conftest import golden, yaml_args
from torchmdnet._native import ET_SCALAR
from torchmdnet.kernels import EdgeGraph, et_act_flags, t_message, t_message_composite
from torchmdnet.models.model import create_model, create_transformer_model, load_model

CASES = ["a", "b", "c", "d"]


def _case(d, name):
    args = json.loads(str(d[name + "/args"]))
    sd = {k[len(name) + 4:]: torch.tensor(d[k]) for k in d.files if k.startswith(name + "/sd/")}
    gp = {k[len(name) + 4:]: d[k] for k in d.files if k.startswith(name + "/gp/")}
    return args, sd, gp


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_flag_value():
    assert ET_SCALAR == 0x10000


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    """Every stored quantity, float64, gated at 1e-10 of the largest entry (test_gn_cpu.py's bar for gn_ref)."""
    d = golden("t_ref.npz")
    args, sd, gp = _case(d, name)
    z, batch = torch.tensor(d["z"]), torch.tensor(d["batch"])
    pos = torch.tensor(d["pos"]).requires_grad_(True)
    sd = {k: (v.clone().requires_grad_(True) if k in gp else v) for k, v in sd.items()}
    y = t_ref.energy(sd, args, z, pos, batch)
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


@pytest.mark.parametrize("has", [(True, True), (True, False), (False, True), (False, False)])
def test_message_composite_matches_three_line_form(has):
    """A random symmetric list with self loops, an atom without edges and padding slots (src = dst = -1)."""
    gen = torch.Generator().manual_seed(0)
    n, heads, H = 7, 2, 8
    und = [(0, 1), (1, 2), (0, 3), (2, 4), (3, 4), (1, 4)]  # atom 5 has its self loop only, atom 6 nothing
    ei = torch.tensor([[a for a, b in und] + [b for a, b in und] + [0, 2, 5],
                       [b for a, b in und] + [a for a, b in und] + [0, 2, 5]])
    E = ei.shape[1]
    q, k, v = (torch.randn(n, H, generator=gen, dtype=torch.float64) for _ in range(3))
    pk = torch.randn(E, H, generator=gen, dtype=torch.float64) if has[0] else None
    pv = torch.randn(E, H, generator=gen, dtype=torch.float64) if has[1] else None
    C = torch.rand(E, generator=gen, dtype=torch.float64)
    acts = et_act_flags(2, 1)  # tanh on dk / dv, shifted softplus in the attention
    act, attn = t_ref.ACTS["tanh"], t_ref.ACTS["ssp"]
    ref = t_ref.message(q, k, v, None if pk is None else act(pk), None if pv is None else act(pv), C, ei[0], ei[1],
                        n, heads, attn)
    out = t_message_composite(q, k, v, pk, pv, C, ei[0], ei[1], n, heads, acts)
    assert torch.allclose(out, ref, rtol=1e-14, atol=1e-14)
    assert float(out[6].abs().max()) == 0
    # padding slots carry nothing, whatever their rows hold
    pad = 3
    eip = torch.cat([ei, torch.full((2, pad), -1)], 1)
    grow = lambda t: None if t is None else torch.cat([t, torch.randn(pad, *t.shape[1:], generator=gen,
                                                                      dtype=t.dtype)])
    outp = t_message_composite(q, k, v, grow(pk), grow(pv), grow(C), eip[0], eip[1], n, heads, acts)
    assert torch.allclose(outp, ref, rtol=1e-14, atol=1e-14)  # (a longer index_add may sum in another order)
    # the public op on CPU tensors takes the composite
    g, perm = EdgeGraph.from_edge_index(ei, n)
    sel = lambda t: None if t is None else t[perm]
    assert torch.allclose(t_message(q, k, v, sel(pk), sel(pv), C[perm], g, heads, acts), ref, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("name", CASES)
def test_construction_contract(name, tmp_path):
    d = golden("t_ref.npz")
    args, sd, gp = _case(d, name)
    model = create_transformer_model(dict(args))
    assert set(model.state_dict()) == set(sd)
    assert set(dict(model.named_parameters())) == set(gp)
    model.load_state_dict(sd, strict=True)
    assert model.fused_eval is False
    path = str(tmp_path / "t.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(args)}, path)
    loaded = load_model(path)
    assert type(loaded.representation_model).__name__ == "TorchMD_T"
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_seeded_initialisation_matches_reference():
    d = golden("t_ref.npz")
    for name in ("a", "b"):
        args, sd, _ = _case(d, name)
        torch.manual_seed(int(d[name + "/seed"]))
        model = create_transformer_model(dict(args))
        for k, v in model.state_dict().items():
            assert torch.allclose(v, sd[k], rtol=0, atol=1e-15), (name, k)


def test_refusals():
    with pytest.raises(NotImplementedError, match="create_transformer_model"):
        create_model(yaml_args("transformer"))
    for other in ("equivariant-transformer", "tensornet", "graph-network"):
        with pytest.raises(ValueError, match="transformer"):
            create_transformer_model(yaml_args(other))
