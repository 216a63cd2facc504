"""Yardstick of the stress-training tests: gradients of a loss on the virial of the fp64 oracle (no GPU).

tests/virial_ref.py makes the oracle's virial exact by substituting ``oracle.model_oracle.edge_geometry`` with a
strained wrapper (``dl -> dl + dl @ eps^T``) and differentiating the energies w.r.t. ``eps`` at ``eps = 0``.  Here the
same substitution runs with the state-dict entries as leaves and ``create_graph=True``, so that
``W[m] = -dE_m/d eps`` is itself differentiable, and a loss on (y, neg_dy, W) is differentiated to the leaves -- as
tests/test_gpu_train_parity._oracle_grads does for the energy and force terms -- and, on request, to the positions.

The oracle's own rounding error matters at the float64 bar (rtol = atol = 1e-9).  Its per-atom sums over the edges
are ``index_add`` calls, which add one edge after the other.  With static_shapes a few thousand identical padding
copies of atom 0's self loop land in one such sum, and adding one value thousands of times in sequence rounds the
same way every time (4700 copies: 1.2e-13 relative, against a few 1e-15 for a pairwise sum).  On the static_shapes
TensorNet fixture the stress-loss gradients (|g| up to 1.3e3) move by 2.8e-8 (tensor_embedding.linears_tensor.0.weight),
1.2e-8 (distance_proj1) and 9.6e-9 (emb2.weight) when only the order of these sums changes -- more than the bar, and
the whole gap between the one-after-the-other oracle and the GPU there; on the other fixtures the same change moves
them by ~1e-13.  So the oracle is evaluated here with its dim-0 ``index_add`` / ``index_select`` calls summed
pairwise (``pairwise_edge_sums``: the same sums and gathers, forward and every backward order, written out with
elementwise adds so that the order does not depend on a library), for every case alike.  The oracle file itself
stays as it is.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import model_oracle as O


_CHUNK = 32


def _pairwise_index_add(src, idx, n):
    """zeros(n, ...).index_add(0, idx, src) with the edges added pairwise: chunks of 32 edges are scattered into
    their own [n, ...] slab, and the slabs are added two by two (a binary tree of elementwise adds)."""
    E, tail = src.shape[0], tuple(src.shape[1:])
    s = src.reshape(E, -1)
    F_ = s.shape[1]
    C = max(1, -(-E // _CHUNK))
    pad = C * _CHUNK - E
    if pad:
        s = torch.cat([s, s.new_zeros(pad, F_)])
        idx = torch.cat([idx, idx.new_zeros(pad)])
    part = s.new_zeros(C, n, F_).scatter_add_(1, idx.view(C, _CHUNK, 1).expand(C, _CHUNK, F_), s.view(C, _CHUNK, F_))
    while part.shape[0] > 1:
        if part.shape[0] % 2:
            part = torch.cat([part, part.new_zeros((1,) + tuple(part.shape[1:]))])
        part = part[0::2] + part[1::2]
    return part[0].view((n,) + tail)


class _PairwiseAdd(torch.autograd.Function):
    """(src [E, ...], idx, n) -> [n, ...]; its backward is the gather, whose backward is this again."""

    @staticmethod
    def forward(ctx, src, idx, n):
        ctx.idx = idx
        return _pairwise_index_add(src, idx, n)

    @staticmethod
    def backward(ctx, g):
        return _Gather.apply(g, ctx.idx), None, None


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        ctx.idx, ctx.n = idx, x.shape[0]
        return _ORIG["index_select"](x, 0, idx)

    @staticmethod
    def backward(ctx, g):
        return _PairwiseAdd.apply(g.contiguous(), ctx.idx, ctx.n), None


_ORIG = {"index_add": torch.Tensor.index_add, "index_select": torch.Tensor.index_select}


@contextlib.contextmanager
def pairwise_edge_sums():
    """Inside the block, ``t.index_add(0, idx, src)`` and ``t.index_select(0, idx)`` of floating tensors (1-D index)
    go through ``_PairwiseAdd`` / ``_Gather``: mathematically the same, differentiable to any order, but every sum
    over the edges -- the forward scatter and the backward of every gather -- is pairwise instead of one edge
    after the other."""

    def index_add(self, dim, idx, src, *a, **k):
        if dim != 0 or a or k or idx.dim() != 1 or not src.is_floating_point() or idx.numel() == 0:
            return _ORIG["index_add"](self, dim, idx, src, *a, **k)
        return self + _PairwiseAdd.apply(src, idx.long(), self.shape[0])

    def index_select(self, dim, idx):
        if dim != 0 or idx.dim() != 1 or not self.is_floating_point() or idx.numel() == 0:
            return _ORIG["index_select"](self, dim, idx)
        return _Gather.apply(self, idx.long())

    torch.Tensor.index_add, torch.Tensor.index_select = index_add, index_select
    try:
        yield
    finally:
        torch.Tensor.index_add, torch.Tensor.index_select = _ORIG["index_add"], _ORIG["index_select"]


def oracle_stress_grads(model, cfg, z, pos, batch, virial, w_v=1.0, y=None, neg_dy=None, w_y=0.0, w_f=0.0,
                        static_shapes=True):
    """(loss, {parameter name: d loss / d parameter}, d loss / d pos, W) of
    ``loss = w_v MSE(W, virial) + w_y MSE(y) + w_f MSE(neg_dy)`` in float64 on the CPU, with the parameters of
    ``model`` (its state dict, upcast) as leaves.  ``cfg``: the oracle configuration (create_model arguments plus
    ``box`` for a periodic system)."""
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
    sd.update(leaves)
    eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    orig = O.edge_geometry
    seen = {}

    def strained(p, *a, **k):
        seen["pos"] = p  # the oracle's own position leaf
        src, dst, dl, r, self_edge = orig(p, *a, **k)
        dl = dl + dl @ eps.T.to(dl.dtype)
        sq = (dl * dl).sum(1)
        r = torch.where(self_edge, torch.zeros_like(sq), torch.where(self_edge, torch.ones_like(sq), sq).sqrt())
        return src, dst, dl, r, self_edge

    O.edge_geometry = strained
    try:
        with pairwise_edge_sums():
            y_ref, f_ref = O.energy_forces(sd, dict(cfg), z, pos, batch, static_shapes=static_shapes,
                                           create_graph=True)
            rows = [torch.autograd.grad(y_ref[m, 0], eps, create_graph=True)[0] for m in range(y_ref.shape[0])]
    finally:
        O.edge_geometry = orig
    W = -torch.stack(rows)
    loss = w_v * F.mse_loss(W, virial.detach().cpu().double())
    if w_y > 0:
        loss = loss + w_y * F.mse_loss(y_ref, y.detach().cpu().double())
    if w_f > 0:
        loss = loss + w_f * F.mse_loss(f_ref, neg_dy.detach().cpu().double())
    g = torch.autograd.grad(loss, [leaves[n] for n in names] + [seen["pos"]], allow_unused=True)
    grads = {n: (torch.zeros_like(leaves[n]) if gi is None else gi) for n, gi in zip(names, g)}
    return float(loss.detach()), grads, g[-1], W.detach()
