"""What the pair-potential priors (ZBL, D2, Coulomb) share: their own neighbour list and the HIP pair kernel.

The reference builds the list with ``Distance`` (torch_cluster).  Here every pair prior calls
``kernels.build_graph`` -- the native, symmetric, destination-sorted CSR list without self loops -- and
``kernels.pair_prior`` (csrc/pair_prior.hip), whose distances carry first- and second-order autograd to the
positions through the neighbour op's backward kernels.

Differences from the reference, on purpose:

* No box: the reference's priors ignore periodicity, and so do these.
* Overflow: the reference asserts ``max_num_neighbors`` per atom; here the list holds at most
  ``max_num_neighbors * n_atoms`` directed pairs in total and ``build_graph`` raises ``RuntimeError`` beyond
  that.  With ``static_capacity`` set (HIP-graph capture, ``graphs.GraphedEnergyForces``) nothing is raised
  in the call; the device flag ``last_overflow`` reports it on demand.
* A molecule without pairs gets 0 (the reference pads in ZBL only).
* The prior holds no ``OptimizedDistance`` submodule: its capacity is its own ``static_capacity``, not the
  representation model's.
"""
from torch import Tensor

from .base import BasePrior


class PairPrior(BasePrior):
    # host-side status of the last list build, not model state: a model that already ran eagerly still scripts
    __jit_ignored_attributes__ = ["static_capacity", "last_overflow", "last_num_pairs"]

    def __init__(self):
        super().__init__()
        # HIP-graph mode: fixed pair capacity of this prior's own list, no host synchronisation
        self.static_capacity = None
        self.last_overflow = None
        self.last_num_pairs = None

    def reset_parameters(self):
        pass

    def _graph(self, pos: Tensor, batch: Tensor, cutoff: float):
        from .. import kernels
        g = kernels.build_graph(pos, batch, 0.0, cutoff, int(self.max_num_neighbors) * pos.shape[0], loop=False,
                                strategy="brute", check_errors=True, static_capacity=self.static_capacity)
        # the device-side status only (see OptimizedDistance.graph): not the graph and its autograd history
        self.last_overflow = getattr(g, "overflow", None)
        self.last_num_pairs = g.num_pairs_dev if g.num_pairs_dev is not None else g.num_pairs
        return g

    def _add_energy(self, y: Tensor, kind: str, graph, a, b, consts, batch: Tensor):
        from .. import kernels
        e = kernels.pair_prior(kind, graph, a, b, consts, batch, y.shape[0])
        return y + e.to(y.dtype).reshape(y.shape)
