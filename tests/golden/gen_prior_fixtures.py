"""Golden fixture of the pair priors (ZBL, D2, Coulomb) from the REFERENCE implementation on the CPU.

Same recipe and isolation as ``gen_reference_fixtures.py`` (``run_prior_fixtures.sh`` sets them up).  The
reference's priors take their neighbour list from ``torch_cluster.radius_graph``, which the committed shim only
refuses; here it is replaced in-process by a dense stand-in: every ordered pair of distinct atoms of one
molecule within ``r``.  Written: ``tests/golden/priors_ref.npz`` -- inputs and, per prior, the energy ``y``, the
forces ``-dy/dpos`` and ``d(sum F^2)/dpos``, all float64.  Data only.
"""
import os

import numpy as np
import torch

import torchmdnet.models.utils as ref_utils  # the reference
from gen_reference_fixtures import qm9_like

OUT = os.path.dirname(os.path.abspath(__file__))
SCALES = dict(distance_scale=1e-10, energy_scale=4.35974e-18)


def dense_radius_graph(pos, r, batch=None, loop=False, max_num_neighbors=32):
    n = pos.shape[0]
    batch = torch.zeros(n, dtype=torch.long) if batch is None else batch
    d = (pos.detach()[:, None, :] - pos.detach()[None, :, :]).norm(dim=-1)
    keep = (batch[:, None] == batch[None, :]) & (d < r)
    if not loop:
        keep &= ~torch.eye(n, dtype=torch.bool)
    dst, src = keep.nonzero(as_tuple=True)
    return torch.stack([src, dst])


def main():
    ref_utils.radius_graph = dense_radius_graph
    from torchmdnet.priors import ZBL, D2, Coulomb
    z, pos, batch = qm9_like(3, gen_seed=1)
    # a generator of the same seed as the inputs'; the exact charges are stored in the fixture
    charges = torch.randn(len(z), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.4
    numbers = list(range(100))
    priors = {"zbl": (ZBL(5.0, 40, atomic_number=numbers, **SCALES), None),
              "d2": (D2(10.0, 128, atomic_number=numbers, dtype=torch.float64, **SCALES), None),
              "coulomb": (Coulomb(0.3, 40, **SCALES), {"partial_charges": charges})}
    res = {"z": z.numpy(), "pos": pos.numpy(), "batch": batch.numpy(), "partial_charges": charges.numpy()}
    n_mol = int(batch.max()) + 1
    for name, (prior, extra) in priors.items():
        p = pos.clone().requires_grad_(True)
        y = prior.post_reduce(torch.zeros(n_mol, 1, dtype=torch.float64), z, p, batch, extra)
        f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
        h, = torch.autograd.grad((f ** 2).sum(), p)
        res[name + "/y"] = y.detach().numpy()
        res[name + "/forces"] = f.detach().numpy()
        res[name + "/dF2"] = h.numpy()
        print(name, "y", y.detach().reshape(-1).tolist())
    path = os.path.join(OUT, "priors_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
