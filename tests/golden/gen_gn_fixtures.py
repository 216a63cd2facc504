"""Golden fixture of the graph-network model from the REFERENCE implementation on the CPU, float64.

Same recipe and isolation as ``gen_prior_fixtures.py`` (``run_gn_fixtures.sh`` sets them up).  The reference's
``Distance`` takes its neighbour list from ``torch_cluster.radius_graph``, which the committed shim only refuses,
and the committed ``torch_scatter`` shim has no ``max``; both are replaced in-process: the dense
``radius_graph`` stand-in of ``gen_prior_fixtures.py``, and a ``scatter`` with ``max`` (empty rows 0, as
torch_scatter gives) bound into the ``torch_geometric.nn`` shim module.

Written: ``tests/golden/gn_ref.npz`` -- the inputs and, per case, the model args (JSON), the ``state_dict``, the
energy ``y``, the forces ``-dy/dpos``, ``d(sum F^2)/dpos`` and the gradient of ``sum y + sum F^2`` with respect to
every parameter.  Data only.

Cases (embedding dimension 32, 2 layers, 16 RBFs, max_z 10 to keep the tables small, ``qm9_like(3, gen_seed=1)``):
  a  aggr add,  neighbour embedding, expnorm
  b  aggr mean, no neighbour embedding, gauss, cutoff_lower 1.0
  c  aggr max,  neighbour embedding, expnorm, trainable_rbf
  d  as (a) with atom_filter = 1 (hydrogens dropped before the head).  The reference refuses derivative=True with
     an atom filter (models/model.py:89-92), so the model is built with derivative=False and the forces are
     taken here, by autograd on the input positions, exactly as for the other cases.
The max case has a condition on the input, checked here on the CPU: in every layer the two largest messages of
every (atom, channel) with at least two edges differ by at least MIN_PAIR_GAP = 1e-4 of the larger of the two
(``gn_ref.top2_pair_gaps``).  A float32 evaluation carries a message with a relative error of a few 1e-7 to 1e-6,
so it picks the same winners (two orders of magnitude of margin).  The first parameter seed from 1234 on that meets it is
used; the seed and the gap are stored (``c/seed``, ``c/top2_pair_gap``).  The gap relative to the LAYER's largest
message (``gn_ref.top2_gaps``, stored as ``c/top2_gap``) cannot reach 1e-4 with these inputs and is not the
condition: it is ~1e-9 for every seed, because rows whose messages are all negative end with their two
near-cutoff edges (both ~0) on top, and ordinary pairs come as close as 1e-6 of the layer maximum.
"""
import json
import os
import sys

import numpy as np
import torch

import torchmdnet.models.utils as ref_utils  # the reference
import torch_geometric.nn as pyg_nn  # the committed shim
from gen_prior_fixtures import dense_radius_graph
from gen_reference_fixtures import base_args, qm9_like

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import gn_ref  # noqa: E402  (tests/gn_ref.py: the top-two gap of the max case)

MIN_PAIR_GAP = 1e-4
SEEDS_TRIED = 64
CASES = {
    "a": dict(aggr="add", neighbor_embedding=True, rbf_type="expnorm"),
    "b": dict(aggr="mean", neighbor_embedding=False, rbf_type="gauss", cutoff_lower=1.0),
    "c": dict(aggr="max", neighbor_embedding=True, rbf_type="expnorm", trainable_rbf=True),
    "d": dict(aggr="add", neighbor_embedding=True, rbf_type="expnorm", atom_filter=1),
}


def scatter_with_max(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    """torch_scatter.scatter over dim 0 of [E, F] rows: sum / mean / max, rows without entries 0."""
    assert src.dim() == 2 and dim % src.dim() == 0 and index.dim() == 1
    idx = index.view(-1, 1).expand_as(src)
    zeros = torch.zeros((dim_size, src.shape[1]), dtype=src.dtype)
    if reduce in ("sum", "add"):
        return zeros.scatter_add(0, idx, src)
    cnt = torch.zeros(dim_size, dtype=src.dtype).index_add(0, index, torch.ones_like(index, dtype=src.dtype))
    if reduce == "mean":
        return zeros.scatter_add(0, idx, src) / cnt.clamp(min=1).unsqueeze(1)
    if reduce == "max":
        top = zeros.scatter_reduce(0, idx, src, "amax", include_self=False)
        return top * (cnt > 0).to(src.dtype).unsqueeze(1)
    raise NotImplementedError(reduce)


def case_args(kw):
    args = base_args("graph-network", embedding_dimension=32, num_layers=2, num_rbf=16, precision=64,
                     derivative=False, output_model="Scalar", atom_filter=-1, cutoff_lower=0.0, max_z=10)
    args.update(kw)
    return args


def main():
    ref_utils.radius_graph = dense_radius_graph
    pyg_nn.scatter = scatter_with_max
    from torchmdnet.models.model import create_model
    z, pos, batch = qm9_like(3, gen_seed=1)
    res = {"z": z.numpy(), "pos": pos.numpy(), "batch": batch.numpy()}
    for name, kw in CASES.items():
        args = case_args(kw)
        seed = 1234
        while True:
            torch.manual_seed(seed)
            model = create_model(args)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if args["aggr"] != "max":
                break
            gap = min(gn_ref.top2_pair_gaps(sd, args, z, pos, batch))
            print(name, "seed", seed, "smallest top-two pair gap", gap, flush=True)
            if gap >= MIN_PAIR_GAP:
                res[name + "/top2_pair_gap"] = np.array(gap)
                res[name + "/top2_gap"] = np.array(min(gn_ref.top2_gaps(sd, args, z, pos, batch)))
                break
            seed += 1
            assert seed < 1234 + SEEDS_TRIED, "no parameter seed meets the max case's pair-gap condition"
        assert args["aggr"] != "max" or float(res[name + "/top2_pair_gap"]) >= MIN_PAIR_GAP
        params = dict(model.named_parameters())
        p = pos.clone().requires_grad_(True)
        y, _ = model(z, p, batch)
        f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
        f2 = (f ** 2).sum()
        h, = torch.autograd.grad(f2, p, retain_graph=True)
        gp = torch.autograd.grad(y.sum() + f2, list(params.values()), allow_unused=True)
        res[name + "/args"] = np.array(json.dumps({k: v for k, v in args.items()
                                                   if isinstance(v, (int, float, str, bool, type(None)))}))
        res[name + "/seed"] = np.array(seed)
        res[name + "/y"] = y.detach().numpy()
        res[name + "/forces"] = f.detach().numpy()
        res[name + "/dF2"] = h.numpy()
        for k, v in sd.items():
            res[f"{name}/sd/{k}"] = v.numpy()
        for k, g in zip(params, gp):
            res[f"{name}/gp/{k}"] = (torch.zeros_like(params[k]) if g is None else g).detach().numpy()
        print(name, "y", y.detach().reshape(-1).tolist(), "|F|max", float(f.abs().max()))
    path = os.path.join(OUT, "gn_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
