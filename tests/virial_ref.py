"""Yardstick of the virial tests: the exact strain derivative of the fp64 oracle (no GPU).

The oracle's energy depends on the positions and the box only through ``oracle.model_oracle.edge_geometry``'s
per-edge ``dl`` (the image shift is a constant).  Under the homogeneous strain pos -> pos (I + eps)^T,
box -> box (I + eps)^T every ``dl`` becomes ``dl (I + eps)^T``, so replacing ``edge_geometry`` in-process by a
wrapper that returns ``dl + dl @ eps^T`` (and the distances recomputed from it with the original's self-edge
guards) makes ``autograd.grad(E_m, eps)`` at ``eps = 0`` the exact ``dE_m/d eps = sum_e g_e (x) dl_e``.  The
oracle file itself stays as it is.  The convention (which index of eps is which) is pinned against finite
differences of the untouched oracle in tests/test_virial_cpu.py.
"""
import numpy as np
import torch

from conftest import golden, state_dict_from, yaml_args
from oracle import model_oracle as O

PERIODIC_FIXTURES = ("et_tiny_periodic_f64", "tn_tiny_periodic_dyn_f64", "tn_tiny_periodic_static_f64")


def fixture_args(name, precision=64):
    """create_model arguments of a reference-run periodic fixture (tests/test_gpu_periodic_oracle.py)."""
    if name.startswith("et"):
        return yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                         max_num_neighbors=64, derivative=True, output_model="Scalar", precision=precision)
    return yaml_args("tensornet", embedding_dimension=32, num_layers=2, num_rbf=16, max_num_neighbors=64,
                     cutoff_upper=4.5, derivative=True, output_model="Scalar", precision=precision)


def fixture_case(name):
    """(state dict, oracle cfg with the box, z, pos, batch, static_shapes) of a periodic fixture."""
    d = golden(name + ".npz")
    cfg = dict(fixture_args(name))
    cfg["box"] = np.asarray(d["box"], dtype=np.float64)
    return (state_dict_from(d), cfg, torch.as_tensor(d["z"]), torch.as_tensor(d["pos"]).double(),
            torch.as_tensor(d["batch"]), "static" in name)


def oracle_energy(sd, cfg, z, pos, batch, static_shapes=True):
    """Per-molecule energies [n_mol] of the untouched oracle (float64)."""
    y, _ = O.energy_forces(sd, cfg, z, pos, batch, static_shapes=static_shapes)
    return y.detach().reshape(-1)


def oracle_virial(sd, cfg, z, pos, batch, static_shapes=True):
    """(y [n_mol, 1], neg_dy [N, 3], virial [n_mol, 3, 3]) of the fp64 oracle, virial[m] = -dE_m/d eps."""
    eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    orig = O.edge_geometry

    def strained(*a, **k):
        src, dst, dl, r, self_edge = orig(*a, **k)
        dl = dl + dl @ eps.T.to(dl.dtype)
        sq = (dl * dl).sum(1)
        r = torch.where(self_edge, torch.zeros_like(sq), torch.where(self_edge, torch.ones_like(sq), sq).sqrt())
        return src, dst, dl, r, self_edge

    O.edge_geometry = strained
    try:
        y, f = O.energy_forces(sd, cfg, z, pos, batch, static_shapes=static_shapes, create_graph=True)
        rows = [torch.autograd.grad(y[m, 0], eps, retain_graph=True)[0] for m in range(y.shape[0])]
    finally:
        O.edge_geometry = orig
    return y.detach(), f.detach(), -torch.stack(rows)


_CACHE = {}


def fixture_virial(name):
    """oracle_virial of a periodic fixture, computed once per session and shared (read-only)."""
    if name not in _CACHE:
        sd, cfg, z, pos, batch, static = fixture_case(name)
        _CACHE[name] = oracle_virial(sd, cfg, z, pos, batch, static_shapes=static)
    return _CACHE[name]
