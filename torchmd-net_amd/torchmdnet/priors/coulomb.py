"""Coulomb interaction damped by erf(alpha r) at short range (interface of the reference's Coulomb prior,
torchmdnet/priors/coulomb.py:7-50).

    E = 1/2 sum_pairs k_e erf(alpha' R) q_i q_j / R,   R = r * distance_scale * 1e9 (nm), alpha' = alpha per nm

Every sample carries ``partial_charges`` (``extra_args["partial_charges"]``, one per atom); the dataset (or the
arguments) give ``distance_scale`` (positions -> metres) and ``energy_scale`` (energies -> joules).  Gradients
flow to the positions only: charges that require grad are refused, not detached silently.

The cutoff is infinite, as in the reference: the brute neighbour build compares squared distances with
``inf`` (csrc/neighbors.hip ``d2 < cu2``), so every same-molecule pair is listed.  No box, total-pairs
overflow, own ``static_capacity``: see ``priors/pair.py``.  ``post_reduce`` does not script
(``torch.jit.unused``): a scripted model holding this prior compiles and raises when called."""
import math
from typing import Dict, Optional

import torch
from torch import Tensor

from .pair import PairPrior, box_options


class Coulomb(PairPrior):
    periodic_refusal = ("this prior has an infinite cutoff, which has no meaning under periodic images (a periodic "
                        "Coulomb sum needs an Ewald method)")

    @box_options
    def __init__(self, alpha, max_num_neighbors, distance_scale=None, energy_scale=None, dataset=None):
        super().__init__()
        if distance_scale is None:
            distance_scale = dataset.distance_scale
        if energy_scale is None:
            energy_scale = dataset.energy_scale
        self.alpha = alpha
        self.max_num_neighbors = max_num_neighbors
        self.distance_scale = float(distance_scale)
        self.energy_scale = float(energy_scale)

    def get_init_args(self):
        return {"alpha": self.alpha,
                "max_num_neighbors": self.max_num_neighbors,
                "distance_scale": self.distance_scale,
                "energy_scale": self.energy_scale}

    def constants(self):
        """(k_e, r -> nm, alpha per nm) in double: phi = k_e erf(alpha' R) q_i q_j / R, R = c1 r."""
        to_nm = 1e9 * self.distance_scale
        return (2.30707e-28 / self.energy_scale / self.distance_scale, to_nm, float(self.alpha) / to_nm)

    @torch.jit.unused
    def post_reduce(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor,
                    extra_args: Optional[Dict[str, Tensor]]):
        if extra_args is None or "partial_charges" not in extra_args:
            raise RuntimeError("Coulomb prior: extra_args['partial_charges'] (one charge per atom) is required")
        q = extra_args["partial_charges"]
        if q.requires_grad:
            raise RuntimeError("Coulomb prior: partial_charges require grad, but gradients flow to the positions "
                               "only; pass detached charges")
        if q.dim() != 1 or q.shape[0] != pos.shape[0]:
            raise RuntimeError("Coulomb prior: partial_charges must hold one charge per atom")
        graph = self._graph(pos, batch, math.inf)
        return self._add_energy(y, "coulomb", graph, q.to(pos.dtype), None, self.constants(), batch)
