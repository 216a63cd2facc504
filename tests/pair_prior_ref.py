"""Dense restatement of the pair priors in plain torch (the yardstick of the pair-prior tests).

Every ordered pair of distinct atoms of one molecule, a mask on ``r < cutoff``, and the formulas of the
reference (priors/zbl.py:46-63, d2.py:163-193, coulomb.py:38-50) term by term; 1/2 for the double counting.
Runs in the dtype and on the device of ``pos`` (the tests feed float64) and is differentiable to any order."""
import math

import torch

BOHR = 5.29177210903e-11


def _pairs(pos, batch, cutoff):
    n = pos.shape[0]
    i, j = torch.triu_indices(n, n, offset=1, device=pos.device)
    same = batch[i] == batch[j]
    i, j = i[same], j[same]
    r = (pos[i] - pos[j]).norm(dim=-1)
    keep = r.detach() < cutoff
    # both directions, as the symmetric list has them
    i, j, r = i[keep], j[keep], r[keep]
    return torch.cat([i, j]), torch.cat([j, i]), torch.cat([r, r])


def _reduce(e_pair, mol, n_mol):
    return 0.5 * torch.zeros(n_mol, dtype=e_pair.dtype, device=e_pair.device).index_add(0, mol, e_pair)


def zbl_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale):
    i, j, r = _pairs(pos, batch, cutoff)
    Z = torch.as_tensor(atomic_number, device=pos.device)[z].to(pos.dtype)
    a = 0.8854 * BOHR / (Z[i] ** 0.23 + Z[j] ** 0.23)
    d = r * distance_scale / a
    f = (0.1818 * torch.exp(-3.2 * d) + 0.5099 * torch.exp(-0.9423 * d) + 0.2802 * torch.exp(-0.4029 * d)
         + 0.02817 * torch.exp(-0.2016 * d))
    f = f * 0.5 * (torch.cos(r * math.pi / cutoff) + 1.0) * (r < cutoff)
    e = f * Z[i] * Z[j] / r
    return (2.30707755e-28 / energy_scale / distance_scale) * _reduce(e, batch[i], n_mol)


def d2_energy(pos, z, batch, n_mol, cutoff, atomic_number, distance_scale, energy_scale, c6, r_r, d=20, s6=1):
    """``c6`` / ``r_r``: the prior's tables indexed by atomic number (J/mol nm^6, nm)."""
    i, j, r = _pairs(pos, batch, cutoff)
    R = r * (distance_scale * 1e9)
    Z = torch.as_tensor(atomic_number, device=pos.device)[z]
    c6, r_r = c6.to(pos.device, pos.dtype), r_r.to(pos.device, pos.dtype)
    C = (c6[Z[i]] * c6[Z[j]]).sqrt()
    Rr = r_r[Z[i]] + r_r[Z[j]]
    damp = 1 / (1 + torch.exp(-d * (R / Rr - 1)))
    e = C / R ** 6 * damp
    return -s6 * _reduce(e, batch[i], n_mol) / (energy_scale * 6.02214076e23)


def coulomb_energy(pos, q, batch, n_mol, alpha, distance_scale, energy_scale):
    i, j, r = _pairs(pos, batch, math.inf)
    R = r * (1e9 * distance_scale)
    a = alpha / (1e9 * distance_scale)
    q = q.to(pos.dtype)
    e = torch.erf(a * R) * q[i] * q[j] / R
    return (2.30707e-28 / energy_scale / distance_scale) * _reduce(e, batch[i], n_mol)


def energy_forces_second(fn, pos):
    """(y, F = -dy/dpos, d(sum F^2)/dpos) of ``fn(pos) -> (n_mol,)``."""
    p = pos.detach().clone().requires_grad_(True)
    y = fn(p)
    f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
    h, = torch.autograd.grad((f ** 2).sum(), p)
    return y.detach(), f.detach(), h
