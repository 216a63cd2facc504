"""Dense restatement of the invariant Transformer's energy in plain torch (the yardstick of the Transformer tests).

From a ``state_dict`` and the model args: every ordered pair of atoms of one molecule with ``cutoff_lower <= r <
cutoff_upper`` plus every atom's self loop, kept at distance 0 whatever the lower cutoff and excluded from the
neighbour embedding (reference models/utils.py:409-446, 90-92), the basis and cosine cutoff (utils.py:272-390), the
attention layers (torchmd_t.py:246-283: LayerNorm, q / k / v, the activated dk / dv projections, the message
``v_j dv act(sum q_i k_j dk) C``, ``index_add``, o_proj, the residual), out_norm and the heads' math
(output_modules.py).  Runs in the dtype and on the device of ``pos`` (the tests feed float64) and is differentiable
to any order."""
import torch
import torch.nn.functional as F

from gn_ref import _cos_cut, _lin, _offsets, _prefix, aggregate

SSP_SHIFT = 0.693147182464599609375  # log 2 rounded to float32, as the reference's ShiftedSoftplus.shift
ACTS = {"silu": F.silu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "ssp": lambda x: F.softplus(x) - SSP_SHIFT}


def pairs(pos, batch, cl, cu):
    """(src, dst, r) grouped by dst: ordered pairs of distinct atoms of one molecule with cl <= r < cu, and every
    self loop with r = 0 (no gradient through it)."""
    n = pos.shape[0]
    d = (pos.detach()[:, None, :] - pos.detach()[None, :, :]).norm(dim=-1)
    eye = torch.eye(n, dtype=torch.bool, device=pos.device)
    keep = ((batch[:, None] == batch[None, :]) & (d < cu) & (d >= cl) & ~eye) | eye
    dst, src = keep.nonzero(as_tuple=True)
    off = (src != dst).nonzero(as_tuple=True)[0]
    r = pos.new_zeros(src.shape[0]).index_put((off,), (pos[src[off]] - pos[dst[off]]).norm(dim=-1))
    return src, dst, r


def message(q, k, v, dk, dv, C, src, dst, n, heads, attn_act):
    """The three-line reference form: dk / dv are the ACTIVATED projections [E, H] or None."""
    d = q.shape[1] // heads
    s = q[dst].view(-1, heads, d) * k[src].view(-1, heads, d)
    if dk is not None:
        s = s * dk.view(-1, heads, d)
    attn = attn_act(s.sum(-1)) * C.unsqueeze(1)
    vj = v[src].view(-1, heads, d)
    if dv is not None:
        vj = vj * dv.view(-1, heads, d)
    return q.new_zeros((n, heads, d)).index_add(0, dst, vj * attn.unsqueeze(2)).view(n, -1)


def _ln(sd, key, x):
    return F.layer_norm(x, (x.shape[1],), sd[key + ".weight"], sd[key + ".bias"], 1e-5)


def representation(sd, args, z, pos, batch):
    """Node features [N, H] of the Transformer."""
    dt = pos.dtype
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    p = _prefix(sd)
    cl, cu = float(args["cutoff_lower"]), float(args["cutoff_upper"])
    act, attn_act = ACTS[args["activation"]], ACTS[args["attn_activation"]]
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
        off = src != dst
        W = _lin(sd, q + "distance_proj", f[off]) * C[off].unsqueeze(1)
        x_nb = aggregate(W * sd[q + "embedding.weight"][z][src[off]], dst[off], n, "add")
        x = _lin(sd, q + "combine", torch.cat([x, x_nb], dim=1))
    infl = args["distance_influence"]
    for layer in range(args["num_layers"]):
        a = p + f"attention_layers.{layer}."
        h = _ln(sd, a + "layernorm", x)
        dk = act(_lin(sd, a + "dk_proj", f)) if infl in ("keys", "both") else None
        dv = act(_lin(sd, a + "dv_proj", f)) if infl in ("values", "both") else None
        m = message(_lin(sd, a + "q_proj", h), _lin(sd, a + "k_proj", h), _lin(sd, a + "v_proj", h), dk, dv, C,
                    src, dst, n, args["num_heads"], attn_act)
        x = x + _lin(sd, a + "o_proj", m)
    return _ln(sd, p + "out_norm", x)


def energy(sd, args, z, pos, batch):
    """The model output y [n_mol, 1] for the Scalar, DipoleMoment and ElectronicSpatialExtent heads."""
    x = representation(sd, args, z, pos, batch)
    n_mol = int(batch.max()) + 1
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
