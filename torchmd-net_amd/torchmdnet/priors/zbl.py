"""Ziegler-Biersack-Littmark screened nuclear repulsion (interface of the reference's ZBL prior,
torchmdnet/priors/zbl.py:7-63; https://doi.org/10.1007/978-3-642-68779-2_5, equations 9 and 10).

    E = 1/2 sum_pairs k_e Z_i Z_j / r * f(r / a_ij) * C(r),   a_ij = 0.8854 a_0 / (Z_i^0.23 + Z_j^0.23)

with f the four-exponential screening function and C the cosine cutoff (0, cutoff_distance).  The dataset (or
the arguments) give ``atomic_number`` (atom type -> atomic number), ``distance_scale`` (positions -> metres)
and ``energy_scale`` (energies -> joules, not J/mol).  ``atomic_number`` is the one state_dict buffer.

Z^0.23 is formed in the dtype of the positions (the reference rounds it to float32 even in a float64 model).
Non-periodic unless ``periodic=True`` (then the list is built under the call's box, by ``neighbor_strategy``),
total-pairs overflow, own ``static_capacity``: see ``priors/pair.py``.  ``post_reduce`` does not
script (``torch.jit.unused``): a scripted model holding this prior compiles and raises when called."""
import math
from typing import Dict, Optional

import torch
from torch import Tensor

from .pair import PairPrior, box_options

_BOHR = 5.29177210903e-11  # metres


class ZBL(PairPrior):
    @box_options
    def __init__(self, cutoff_distance, max_num_neighbors, atomic_number=None, distance_scale=None,
                 energy_scale=None, dataset=None):
        super().__init__()
        if atomic_number is None:
            atomic_number = dataset.atomic_number
        if distance_scale is None:
            distance_scale = dataset.distance_scale
        if energy_scale is None:
            energy_scale = dataset.energy_scale
        self.register_buffer("atomic_number", torch.as_tensor(atomic_number, dtype=torch.long))
        self.cutoff_distance = cutoff_distance
        self.max_num_neighbors = max_num_neighbors
        self.distance_scale = float(distance_scale)
        self.energy_scale = float(energy_scale)

    def get_init_args(self):
        return {"cutoff_distance": self.cutoff_distance,
                "max_num_neighbors": self.max_num_neighbors,
                "atomic_number": self.atomic_number.tolist(),
                "distance_scale": self.distance_scale,
                "energy_scale": self.energy_scale,
                **self._periodic_args()}

    def constants(self):
        """(k_e, k_a, cutoff, pi / cutoff) in double: phi = k_e Z_i Z_j / r * f(r k_a (b_i + b_j)) * C(r)."""
        cut = float(self.cutoff_distance)
        return (2.30707755e-28 / self.energy_scale / self.distance_scale,
                self.distance_scale / (0.8854 * _BOHR), cut, math.pi / cut)

    @torch.jit.unused
    def post_reduce(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor,
                    extra_args: Optional[Dict[str, Tensor]]):
        return self.post_reduce_box(y, z, pos, batch, extra_args, None)

    @torch.jit.unused
    def post_reduce_box(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor,
                        extra_args: Optional[Dict[str, Tensor]], box: Optional[Tensor]):
        """``post_reduce`` under the call's box (``None``, or a prior built without ``periodic=True``: no box)."""
        graph = self._graph(pos, batch, float(self.cutoff_distance), box, y.shape[0])
        Z = self.atomic_number.index_select(0, z).to(pos.dtype)
        return self._add_energy(y, "zbl", graph, Z, Z.pow(0.23), self.constants(), batch)
