"""Dense restatement of the graph-network energy in plain torch (the yardstick of the graph-network tests).

From a ``state_dict`` and the ``create_model`` args: every ordered pair of distinct atoms of one molecule with
``cutoff_lower <= r < cutoff_upper`` (reference models/utils.py:409-446), the basis and cosine cutoff
(utils.py:272-390), the neighbour embedding (utils.py:90-108), the interaction blocks (torchmd_gn.py:229-272:
filter network, lin1, message ``x_j * W``, ``index_add`` / mean / ``amax`` aggregation, lin2, act, lin, the
residual), an optional atom filter (wrappers.py:45-62) and the heads' math (output_modules.py).  Runs in the dtype
and on the device of ``pos`` (the tests feed float64) and is differentiable to any order."""
import math

import torch
import torch.nn.functional as F

ACTS = {"silu": F.silu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
        "ssp": lambda x: F.softplus(x) - math.log(2.0)}


def _cos_cut(r, cl, cu):
    if cl > 0:
        c = 0.5 * (torch.cos(math.pi * (2 * (r - cl) / (cu - cl) + 1.0)) + 1.0)
        return c * (r < cu).to(r.dtype) * (r > cl).to(r.dtype)
    return 0.5 * (torch.cos(r * math.pi / cu) + 1.0) * (r < cu).to(r.dtype)


def pairs(pos, batch, cl, cu):
    """(src, dst, r) of every ordered pair of distinct atoms of one molecule with cl <= r < cu, grouped by dst."""
    n = pos.shape[0]
    d = (pos.detach()[:, None, :] - pos.detach()[None, :, :]).norm(dim=-1)
    keep = (batch[:, None] == batch[None, :]) & (d < cu) & (d >= cl)
    keep &= ~torch.eye(n, dtype=torch.bool, device=pos.device)
    dst, src = keep.nonzero(as_tuple=True)
    return src, dst, (pos[src] - pos[dst]).norm(dim=-1)


def _lin(sd, key, x):
    b = sd.get(key + ".bias")
    return F.linear(x, sd[key + ".weight"], b)


def aggregate(m, dst, n, aggr):
    if aggr == "max":
        # winners by amax (lowest edge index among equals), then a gather: differentiable to any order
        E, nf = m.shape
        if E == 0:
            return m.new_zeros((n, nf))
        with torch.no_grad():
            top = m.new_full((n, nf), -math.inf).index_reduce(0, dst, m, "amax")
            e = torch.arange(E, device=m.device).unsqueeze(1).expand(E, nf)
            cand = torch.where(m == top[dst], e, torch.full_like(e, E))
            arg = torch.full((n, nf), E, dtype=e.dtype, device=m.device).index_reduce(0, dst, cand, "amin")
        return m.gather(0, arg.clamp(max=E - 1)) * (arg < E).to(m.dtype)
    out = m.new_zeros((n, m.shape[1])).index_add(0, dst, m)
    if aggr == "mean":
        deg = torch.zeros(n, dtype=m.dtype, device=m.device).index_add(0, dst, torch.ones_like(dst, dtype=m.dtype))
        out = out / deg.clamp(min=1).unsqueeze(1)
    return out


def _prefix(sd):
    return "representation_model.model." if any(k.startswith("representation_model.model.") for k in sd) \
        else "representation_model."


def representation(sd, args, z, pos, batch, messages=None):
    """Node features [N, H] of the graph network; ``messages`` (a list): filled with (m, dst) per layer."""
    dt = pos.dtype
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    p = _prefix(sd)
    cl, cu = float(args["cutoff_lower"]), float(args["cutoff_upper"])
    act = ACTS[args["activation"]]
    src, dst, r = pairs(pos, batch, cl, cu)
    d = r.unsqueeze(-1)
    if args["rbf_type"] == "expnorm":
        alpha = 5.0 / (cu - cl)
        f = _cos_cut(d, 0.0, cu) * torch.exp(-sd[p + "distance_expansion.betas"] * (
            torch.exp(alpha * (-d + cl)) - sd[p + "distance_expansion.means"]) ** 2)
    else:
        f = torch.exp(sd[p + "distance_expansion.coeff"] * (d - sd[p + "distance_expansion.offset"]) ** 2)
    C = _cos_cut(r, cl, cu)
    n = z.shape[0]
    x = sd[p + "embedding.weight"][z]
    if args["neighbor_embedding"]:
        q = p + "neighbor_embedding."
        W = _lin(sd, q + "distance_proj", f) * C.unsqueeze(1)
        x_nb = aggregate(W * sd[q + "embedding.weight"][z][src], dst, n, "add")
        x = _lin(sd, q + "combine", torch.cat([x, x_nb], dim=1))
    for layer in range(args["num_layers"]):
        q = p + f"interactions.{layer}."
        W = _lin(sd, q + "mlp.2", act(_lin(sd, q + "mlp.0", f))) * C.unsqueeze(1)
        m = _lin(sd, q + "conv.lin1", x)[src] * W
        if messages is not None:
            messages.append((m, dst))
        h = _lin(sd, q + "conv.lin2", aggregate(m, dst, n, args["aggr"]))
        x = x + _lin(sd, q + "lin", act(h))
    return x


def _offsets(masses, z, pos, batch, n_mol):
    m = masses.to(pos.dtype)[z].unsqueeze(1)
    acc = pos.new_zeros(n_mol, 4).index_add(0, batch, torch.cat([pos * m, m], dim=1))
    return pos - (acc[:, :3] / acc[:, 3:])[batch]


def energy(sd, args, z, pos, batch):
    """The model output y [n_mol, 1] for the Scalar, DipoleMoment and ElectronicSpatialExtent heads."""
    x = representation(sd, args, z, pos, batch)
    n_mol = int(batch.max()) + 1
    if args.get("atom_filter", -1) > -1:
        keep = z > args["atom_filter"]
        x, z, pos, batch = x[keep], z[keep], pos[keep], batch[keep]
    dt = pos.dtype
    sdh = {k: v.to(dt) for k, v in sd.items() if k.startswith("output_model.") or k in ("mean", "std")}
    act = ACTS[args["activation"]]
    x = _lin(sdh, "output_model.output_network.2", act(_lin(sdh, "output_model.output_network.0", x)))
    head = args["output_model"]
    if head == "DipoleMoment":
        x = x * _offsets(sdh["output_model.atomic_mass"], z, pos, batch, n_mol)
    elif head == "ElectronicSpatialExtent":
        x = x * _offsets(sdh["output_model.atomic_mass"], z, pos, batch, n_mol).pow(2).sum(dim=1, keepdim=True)
    x = x * sdh["std"]
    y = x.new_zeros((n_mol, x.shape[1])).index_add(0, batch, x)
    if args.get("reduce_op", "add") == "mean":
        y = y / torch.bincount(batch, minlength=n_mol).clamp(min=1).to(dt).unsqueeze(1)
    y = y + sdh["mean"]
    return y.norm(dim=-1, keepdim=True) if head == "DipoleMoment" else y


def _top2(sd, args, z, pos, batch):
    """Per layer: (top two messages [2, R, F] of every row with at least two edges, max|m| of the layer)."""
    msgs = []
    with torch.no_grad():
        representation(sd, args, z, pos, batch, messages=msgs)
    out = []
    for m, dst in msgs:
        tops = [m[dst == t].topk(2, dim=0).values for t in torch.unique(dst).tolist() if int((dst == t).sum()) >= 2]
        out.append((torch.stack(tops, dim=1) if tops else m.new_zeros((2, 0, m.shape[1])),
                    float(m.abs().max()) if m.numel() else 0.0))
    return out


def top2_gaps(sd, args, z, pos, batch):
    """Per layer: the smallest gap between the two largest messages of a row, relative to max|m| of the layer,
    over every (atom, channel) whose row has at least two edges (inf when no row has two)."""
    return [float((t[0] - t[1]).min()) / top if t.numel() else math.inf for t, top in _top2(sd, args, z, pos, batch)]


def top2_pair_gaps(sd, args, z, pos, batch):
    """Per layer: the smallest gap between the two largest messages of a row relative to the PAIR itself,
    (m1 - m2) / max(|m1|, |m2|), over the same (atom, channel) set.  A float32 evaluation carries a message with a
    relative error of a few 1e-7 to 1e-6 (two product roundings of 6e-8 on factors that come out of float32 GEMM
    sums), so a pair gap of 1e-4 keeps the same winner with a margin of two orders of magnitude."""
    return [float(((t[0] - t[1]) / torch.maximum(t[0].abs(), t[1].abs())).min()) if t.numel() else math.inf
            for t, _ in _top2(sd, args, z, pos, batch)]
