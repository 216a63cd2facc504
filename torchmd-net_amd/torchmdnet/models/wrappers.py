"""Representation-model wrappers (mirror of reference ``torchmdnet/models/wrappers.py``).

A wrapped model runs eagerly: ``AtomFilter`` reads the molecule count on the host (``batch.unique()``) and
selects atoms by a boolean mask, neither of which a HIP graph can capture (``GraphedEnergyForces`` refuses
wrapped models) or the fused TorchScript evaluation implements (``TorchMD_Net.fused_eval`` is False).
"""
from abc import ABCMeta, abstractmethod
from typing import Optional, Tuple

from torch import Tensor, nn


class BaseWrapper(nn.Module, metaclass=ABCMeta):
    r"""Base class for model wrappers (reference wrappers.py:6-26).

    Children implement ``forward``, which calls ``self.model(z, pos, batch=batch)`` at some point.  Wrappers
    applied before the reduction return the model's output, ``z``, ``pos``, ``batch`` and the vector
    features ``v`` (or None).
    """

    def __init__(self, model):
        super().__init__()
        self.model = model

    def reset_parameters(self):
        self.model.reset_parameters()

    @abstractmethod
    def forward(self, z, pos, batch=None):
        return


class AtomFilter(BaseWrapper):
    """Remove atoms with Z <= remove_threshold from the model's output (reference wrappers.py:29-62)."""

    def __init__(self, model, remove_threshold):
        super().__init__(model)
        self.remove_threshold = remove_threshold

    def forward(self, z: Tensor, pos: Tensor, batch: Tensor, q: Optional[Tensor] = None,
                s: Optional[Tensor] = None, box: Optional[Tensor] = None
                ) -> Tuple[Tensor, Optional[Tensor], Tensor, Tensor, Tensor]:
        if box is None:
            x, v, z, pos, batch = self.model(z, pos, batch=batch, q=q, s=s)
        else:
            x, v, z, pos, batch = self.model(z, pos, batch=batch, q=q, s=s, box=box)

        n_samples = len(batch.unique())

        # drop atoms according to the filter
        atom_mask = z > self.remove_threshold
        x = x[atom_mask]
        if v is not None:
            v = v[atom_mask]
        z = z[atom_mask]
        pos = pos[atom_mask]
        batch = batch[atom_mask]

        assert len(batch.unique()) == n_samples, (
            "Some samples were completely filtered out by the atom filter. "
            f"Make sure that at least one atom per sample exists with Z > {self.remove_threshold}.")
        return x, v, z, pos, batch
