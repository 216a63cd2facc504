"""DFT-D2 dispersion correction (interface of the reference's D2 prior, torchmdnet/priors/d2.py:7-193).

Grimme, "Semiempirical GGA-type density functional constructed with a long-range dispersion correction",
J. Comput. Chem. 27 (2006) 1787, https://doi.org/10.1002/jcc.20495:

    E = -s_6 / 2 sum_pairs sqrt(C6_i C6_j) / R^6 / (1 + exp(-d (R / (R_r,i + R_r,j) - 1))),  d = 20, s_6 = 1

in J/mol with R in nm, then converted with ``energy_scale`` (energies -> joules, not J/mol).
``atomic_number`` maps atom types to atomic numbers, ``distance_scale`` converts positions to metres.
``Z_map``, ``C_6`` and ``R_r`` are the state_dict buffers.  Elements beyond Xe have no parameters (NaN, as in
the reference: their energy is NaN rather than silently zero).

Non-periodic unless ``periodic=True`` (then the list is built under the call's box, by ``neighbor_strategy``),
total-pairs overflow, own ``static_capacity``: see ``priors/pair.py``.  ``post_reduce`` does not
script (``torch.jit.unused``): a scripted model holding this prior compiles and raises when called."""
from typing import Dict, Optional

import torch
from torch import Tensor

from .pair import PairPrior, box_options

_NAN = float("nan")
# Table 1 of Grimme 2006, H .. Xe: C6 in J mol^-1 nm^6 and the van der Waals radius R_0 in Angstrom
# (Sc-Zn and Y-Cd share one entry per row of the periodic table)
_C6 = ([0.14, 0.08,
        1.61, 1.61, 3.13, 1.75, 1.23, 0.70, 0.75, 0.63,
        5.71, 5.71, 10.79, 9.23, 7.84, 5.57, 5.07, 4.61,
        10.80, 10.80] + [10.80] * 10 + [16.99, 17.10, 16.37, 12.64, 12.47, 12.01,
        24.67, 24.67] + [24.67] * 10 + [37.32, 38.71, 38.44, 31.74, 31.50, 29.99])
_R0 = ([1.001, 1.012,
        0.825, 1.408, 1.485, 1.452, 1.397, 1.342, 1.287, 1.243,
        1.144, 1.364, 1.639, 1.716, 1.705, 1.683, 1.639, 1.595,
        1.485, 1.474] + [1.562] * 10 + [1.650, 1.727, 1.760, 1.771, 1.749, 1.727,
        1.628, 1.606] + [1.639] * 10 + [1.672, 1.804, 1.881, 1.892, 1.892, 1.881])
assert len(_C6) == len(_R0) == 54


def _table() -> Tensor:
    """(55, 2) float64: row Z = (C6, R_r in nm); row 0 is NaN (no element)."""
    t = torch.tensor([[_NAN, _NAN]] + [[c, r] for c, r in zip(_C6, _R0)], dtype=torch.float64)
    t[:, 1] *= 0.1  # Angstrom -> nm
    return t


class D2(PairPrior):
    C_6_R_r = _table()

    @box_options
    def __init__(self, cutoff_distance, max_num_neighbors, atomic_number=None, distance_scale=None,
                 energy_scale=None, dataset=None, dtype=torch.float32):
        super().__init__()
        one = torch.tensor(1.0, dtype=dtype).item()
        self.cutoff_distance = cutoff_distance * one
        self.max_num_neighbors = int(max_num_neighbors)
        self.C_6_R_r = self.C_6_R_r.to(dtype=dtype)
        self.atomic_number = list(dataset.atomic_number if atomic_number is None else atomic_number)
        self.distance_scale = one * (dataset.distance_scale if distance_scale is None else distance_scale)
        self.energy_scale = one * (dataset.energy_scale if energy_scale is None else energy_scale)
        self.register_buffer("Z_map", torch.tensor(self.atomic_number, dtype=torch.long))
        self.register_buffer("C_6", self.C_6_R_r[:, 0])
        self.register_buffer("R_r", self.C_6_R_r[:, 1])
        self.d = 20
        self.s_6 = 1

    def get_init_args(self):
        return {"cutoff_distance": self.cutoff_distance,
                "max_num_neighbors": self.max_num_neighbors,
                "atomic_number": self.atomic_number,
                "distance_scale": self.distance_scale,
                "energy_scale": self.energy_scale,
                **self._periodic_args()}

    def constants(self):
        """(k_e, r -> nm, d) in double: phi = -k_e a_i a_j / R^6 / (1 + exp(-d (R / (b_i + b_j) - 1)))."""
        return (self.s_6 / (self.energy_scale * 6.02214076e23), self.distance_scale * 1e9, float(self.d))

    @torch.jit.unused
    def post_reduce(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor,
                    extra_args: Optional[Dict[str, Tensor]]):
        return self.post_reduce_box(y, z, pos, batch, extra_args, None)

    @torch.jit.unused
    def post_reduce_box(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor,
                        extra_args: Optional[Dict[str, Tensor]], box: Optional[Tensor]):
        """``post_reduce`` under the call's box (``None``, or a prior built without ``periodic=True``: no box)."""
        graph = self._graph(pos, batch, float(self.cutoff_distance), box, y.shape[0])
        Z = self.Z_map.index_select(0, z)
        a = self.C_6.index_select(0, Z).to(pos.dtype).sqrt()
        b = self.R_r.index_select(0, Z).to(pos.dtype)
        return self._add_energy(y, "d2", graph, a, b, self.constants(), batch)
