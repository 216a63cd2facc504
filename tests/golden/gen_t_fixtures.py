"""Golden fixture of the invariant Transformer (``model: transformer``) from the REFERENCE implementation on
the CPU, float64.

Same recipe and isolation as ``gen_gn_fixtures.py`` (``run_t_fixtures.sh`` sets them up).  The reference's
``Distance`` takes its neighbour list from ``torch_cluster.radius_graph``, which the committed shim only refuses;
it is replaced in-process by the dense ``radius_graph`` stand-in of ``gen_prior_fixtures.py``, which takes
``loop=True`` (the Transformer's list holds every atom's self loop).

Written: ``tests/golden/t_ref.npz`` -- the inputs and, per case, the model args (JSON), the seed, the
``state_dict``, the energy ``y``, the forces ``-dy/dpos``, ``d(sum F^2)/dpos`` and the gradient of
``sum y + sum F^2`` with respect to every parameter.  Data only.

Cases (embedding dimension 32, 2 layers, 16 RBFs, 4 heads, max_z 10, ``qm9_like(3, gen_seed=1)``):
  a  distance_influence both, neighbour embedding, expnorm, silu / silu
  b  keys, no neighbour embedding, gauss, cutoff_lower 1.0, activation tanh, attn_activation ssp
  c  values, trainable_rbf, attn_activation sigmoid
  d  none
"""
import json
import os

import numpy as np
import torch

import torchmdnet.models.utils as ref_utils  # the reference
from gen_prior_fixtures import dense_radius_graph
from gen_reference_fixtures import base_args, qm9_like

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 1234
CASES = {
    "a": dict(distance_influence="both", neighbor_embedding=True, rbf_type="expnorm", activation="silu",
              attn_activation="silu"),
    "b": dict(distance_influence="keys", neighbor_embedding=False, rbf_type="gauss", cutoff_lower=1.0,
              activation="tanh", attn_activation="ssp"),
    "c": dict(distance_influence="values", trainable_rbf=True, attn_activation="sigmoid"),
    "d": dict(distance_influence="none"),
}


def case_args(kw):
    args = base_args("transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4, precision=64,
                     derivative=False, output_model="Scalar", atom_filter=-1, cutoff_lower=0.0, max_z=10)
    args.update(kw)
    return args


def main():
    ref_utils.radius_graph = dense_radius_graph
    from torchmdnet.models.model import create_model
    z, pos, batch = qm9_like(3, gen_seed=1)
    res = {"z": z.numpy(), "pos": pos.numpy(), "batch": batch.numpy()}
    for name, kw in CASES.items():
        args = case_args(kw)
        torch.manual_seed(SEED)
        model = create_model(args)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        params = dict(model.named_parameters())
        p = pos.clone().requires_grad_(True)
        y, _ = model(z, p, batch)
        f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
        f2 = (f ** 2).sum()
        h, = torch.autograd.grad(f2, p, retain_graph=True)
        gp = torch.autograd.grad(y.sum() + f2, list(params.values()), allow_unused=True)
        res[name + "/args"] = np.array(json.dumps({k: v for k, v in args.items()
                                                   if isinstance(v, (int, float, str, bool, type(None)))}))
        res[name + "/seed"] = np.array(SEED)
        res[name + "/y"] = y.detach().numpy()
        res[name + "/forces"] = f.detach().numpy()
        res[name + "/dF2"] = h.numpy()
        for k, v in sd.items():
            res[f"{name}/sd/{k}"] = v.numpy()
        for k, g in zip(params, gp):
            res[f"{name}/gp/{k}"] = (torch.zeros_like(params[k]) if g is None else g).detach().numpy()
        print(name, "y", y.detach().reshape(-1).tolist(), "|F|max", float(f.abs().max()))
    path = os.path.join(OUT, "t_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
