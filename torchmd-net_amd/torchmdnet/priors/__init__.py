"""Priors on the hot path: Atomref (per-element offsets before the molecular sum) and the pair potentials
D2, ZBL and Coulomb (added after it), which run on the native neighbour list and csrc/pair_prior.hip."""
from .atomref import Atomref
from .base import BasePrior
from .coulomb import Coulomb
from .d2 import D2
from .zbl import ZBL

__all__ = ["Atomref", "D2", "ZBL", "Coulomb"]
