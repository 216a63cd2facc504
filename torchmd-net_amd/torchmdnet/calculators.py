"""MD-facing calculator (mirror of reference ``torchmdnet/calculators.py``): energies and forces of a
checkpointed model for a set of replicas of one molecule.

Difference from the reference: an ``output_transform`` string that is not one of the preset names raises a
``ValueError``; the reference passes it to ``eval``.  Hand in a callable ``(energy, forces) -> (energy,
forces)`` instead.
"""
import torch

from .models.model import load_model

# dict of preset transforms (the reference's names, including the dict's own)
tranforms = {
    "eV/A -> kcal/mol/A": lambda energy, forces: (energy * 23.0609, forces * 23.0609),
    "Hartree/Bohr -> kcal/mol/A": lambda energy, forces: (energy * 627.509, forces * 627.509 / 0.529177),
    "Hartree/A -> kcal/mol/A": lambda energy, forces: (energy * 627.509, forces * 627.509),
}
transforms = tranforms


class External:
    """Energy and forces of an external potential (a checkpoint ``netfile``) for ``embeddings``
    ``[replicas, n_atoms]`` (atomic numbers, one molecule per row).  ``output_transform``: None (identity), a
    preset name of ``tranforms`` or a callable taking and returning ``(energy, forces)`` -- the network's units
    to the simulation's."""

    def __init__(self, netfile, embeddings, device="cpu", output_transform=None):
        self.model = load_model(netfile, device=device, derivative=True)
        self.device = device
        self.n_atoms = embeddings.size(1)
        self.embeddings = embeddings.reshape(-1).to(device)
        self.batch = torch.arange(embeddings.size(0), device=device).repeat_interleave(embeddings.size(1))
        self.model.eval()

        if not output_transform:
            self.output_transformer = lambda energy, forces: (energy, forces)  # identity
        elif callable(output_transform):
            self.output_transformer = output_transform
        elif isinstance(output_transform, str) and output_transform in tranforms:
            self.output_transformer = tranforms[output_transform]
        else:
            raise ValueError(f"External: unknown output_transform {output_transform!r}; choose one of "
                             f"{sorted(tranforms)} or pass a callable (strings are not evaluated)")

    def calculate(self, pos, box):
        pos = pos.to(self.device).type(torch.float32).reshape(-1, 3)
        energy, forces = self.model(self.embeddings, pos, self.batch)
        return self.output_transformer(energy.detach(), forces.reshape(-1, self.n_atoms, 3).detach())
