"""Dense fp64 minimum-image restatement of the periodic pair priors (the yardstick of test_gpu_periodic_priors.py,
itself pinned on the CPU by test_open_molecules_cpu.py).

The formulas are those of tests/pair_prior_ref.py, evaluated by that file's own functions: only its pair
enumeration is substituted (``periodic_pairs``), by one that images every pair in the box of its molecule.

The image is the neighbour list's (csrc/neighbors.hip ``Tric::apply``, the reference's common.cuh:183-194): the
delta is reduced by round() multiples of c, then b, then a.  The integer multiples are constants of a
configuration, so the distances stay differentiable in the positions to any order, and a homogeneous strain
``eps`` (pos -> pos (I + eps)^T, box -> box (I + eps)^T) acts on the imaged delta: ``delta -> delta (I + eps)^T``.
``-dE_m / d eps`` at ``eps = 0`` is the virial of molecule m.

``boxes``: ``None`` (no box), a ``(3, 3)`` box for every molecule, or one per molecule ``(n_mol, 3, 3)``; among
several boxes an all-zero one means that molecule is open (no image)."""
import contextlib

import torch

import pair_prior_ref as R


def imaged_deltas(pos, batch, i, j, boxes, eps=None):
    """pos[i] - pos[j], imaged in the box of batch[i] (= batch[j]), strained by ``eps`` when given."""
    d = pos[i] - pos[j]
    if boxes is not None:
        b = torch.as_tensor(boxes, dtype=pos.dtype, device=pos.device)
        bm = b.expand(len(i), 3, 3) if b.dim() == 2 else b[batch[i]]
        with torch.no_grad():
            opened = (bm == 0).all(dim=2).all(dim=1)
            one = torch.ones_like(d[:, 0])
            dd = d.detach().clone()
            shift = torch.zeros_like(dd)
            for k in (2, 1, 0):  # c, then b, then a
                s = torch.where(opened, torch.zeros_like(one),
                                torch.round(dd[:, k] / torch.where(opened, one, bm[:, k, k])))
                step = s.unsqueeze(1) * bm[:, k, :]
                dd = dd - step
                shift = shift - step
        d = d + shift
    if eps is not None:
        d = d + d @ eps.T.to(d.dtype)
    return d


def pairs(pos, batch, cutoff, boxes, eps=None):
    """``pair_prior_ref._pairs`` under ``boxes``: (i, j, r) of both directions of every same-molecule pair whose
    imaged distance is below ``cutoff``."""
    n = pos.shape[0]
    i, j = torch.triu_indices(n, n, offset=1, device=pos.device)
    same = batch[i] == batch[j]
    i, j = i[same], j[same]
    r = imaged_deltas(pos, batch, i, j, boxes, eps).norm(dim=-1)
    keep = r.detach() < cutoff
    i, j, r = i[keep], j[keep], r[keep]
    return torch.cat([i, j]), torch.cat([j, i]), torch.cat([r, r])


@contextlib.contextmanager
def periodic_pairs(boxes, eps=None):
    """Inside the block the energies of pair_prior_ref enumerate their pairs under ``boxes`` (and ``eps``)."""
    orig = R._pairs
    R._pairs = lambda pos, batch, cutoff: pairs(pos, batch, cutoff, boxes, eps)
    try:
        yield
    finally:
        R._pairs = orig


def zbl_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale, boxes=None, eps=None):
    with periodic_pairs(boxes, eps):
        return R.zbl_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale)


def zbl_energy_reference_rounding(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale,
                                  boxes=None, eps=None):
    """``zbl_energy`` with the screening length rounded as the reference rounds it (priors/zbl.py:52: integer
    atomic numbers ** 0.23 is float32, and so is ``a``), which ``pair_prior_ref.zbl_energy`` -- and the package, in
    a float64 model -- deliberately do not (2e-8 relative).  Only for comparing this file's pair enumeration with
    the reference's recorded float64 run below that."""
    import math
    i, j, r = pairs(pos, batch, cutoff, boxes, eps)
    Z = torch.as_tensor(atomic_number, device=pos.device)[z].long()
    a = 0.8854 * R.BOHR / (Z[i] ** 0.23 + Z[j] ** 0.23)
    assert a.dtype == torch.float32
    d = r * distance_scale / a
    f = (0.1818 * torch.exp(-3.2 * d) + 0.5099 * torch.exp(-0.9423 * d) + 0.2802 * torch.exp(-0.4029 * d)
         + 0.02817 * torch.exp(-0.2016 * d))
    f = f * 0.5 * (torch.cos(r * math.pi / cutoff) + 1.0) * (r < cutoff)
    e = f * Z[i] * Z[j] / r
    return (2.30707755e-28 / energy_scale / distance_scale) * R._reduce(e, batch[i], n_mol)


def d2_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale, c6, r_r, boxes=None,
              eps=None):
    with periodic_pairs(boxes, eps):
        return R.d2_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale, c6, r_r)


def virial(energy, pos):
    """``-dE_m / d eps`` at eps = 0, [n_mol, 3, 3], of ``energy(pos, eps) -> (n_mol,)``; differentiable in
    ``pos`` when ``pos`` requires grad."""
    eps = torch.zeros(3, 3, dtype=pos.dtype, device=pos.device, requires_grad=True)
    y = energy(pos, eps).reshape(-1)
    rows = [torch.autograd.grad(y[m], eps, create_graph=True, allow_unused=True)[0] for m in range(y.shape[0])]
    return -torch.stack([torch.zeros_like(eps) if g is None else g for g in rows])
