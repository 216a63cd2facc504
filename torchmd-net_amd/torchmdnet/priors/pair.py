"""What the pair-potential priors (ZBL, D2, Coulomb) share: their own neighbour list and the HIP pair kernel.

The reference builds the list with ``Distance`` (torch_cluster).  Here every pair prior calls
``kernels.build_graph`` -- the native, symmetric, destination-sorted CSR list without self loops -- and
``kernels.pair_prior`` (csrc/pair_prior.hip), whose distances carry first- and second-order autograd to the
positions through the neighbour op's backward kernels.

Differences from the reference, on purpose:

* The box is opt-in.  The reference's priors ignore periodicity, and so do these by default
  (``periodic=False``: the result is what it was, whatever box the call carries).  ``periodic=True`` (ZBL,
  D2) builds the list under the call's box -- ``forward(..., box=)`` if given, else the representation
  model's distance module's own -- with the prior's cutoff: the reference box checks apply with that cutoff, a
  ``(3, 3)`` box, per-molecule boxes ``(n_molecules, 3, 3)``, open molecules (all-zero boxes) and triclinic
  boxes all work, and the pairs reach the virial.  Given no box, a periodic prior evaluates as a non-periodic
  one.  ``neighbor_strategy`` chooses the build of a periodic list: ``"brute"`` (``build_graph`` moves it to
  ``"shared"`` at 32,768 atoms) or ``"cell"`` (one box only; ``cell_bound`` as ``OptimizedDistance``'s).  The
  non-periodic list is always the all-pairs one.
* Overflow: the reference asserts ``max_num_neighbors`` per atom; here the list holds at most
  ``max_num_neighbors * n_atoms`` directed pairs in total and ``build_graph`` raises ``RuntimeError`` beyond
  that.  With ``static_capacity`` set (HIP-graph capture, ``graphs.GraphedEnergyForces``) nothing is raised
  in the call; the device flag ``last_overflow`` reports it on demand.
* A molecule without pairs gets 0 (the reference pads in ZBL only).
* The prior holds no ``OptimizedDistance`` submodule: its capacity is its own ``static_capacity``, not the
  representation model's.
"""
import functools
from typing import Optional

from torch import Tensor

from .base import BasePrior


def box_options(init):
    """Decorator of a pair prior's ``__init__``: the keywords every pair prior shares -- ``periodic=False`` and
    ``neighbor_strategy="brute"`` -- are taken here and set on the module once ``init`` has run, so each
    constructor keeps the parameters of the reference's (tests/test_pair_priors_cpu.py pins them by name)."""
    @functools.wraps(init)
    def with_options(self, *args, periodic=False, neighbor_strategy="brute", **kwargs):
        if periodic and self.periodic_refusal is not None:
            raise ValueError(f"{type(self).__name__}(periodic=True): {self.periodic_refusal}")
        if neighbor_strategy != "brute" and self.periodic_refusal is not None:
            raise ValueError(f"{type(self).__name__}(neighbor_strategy={neighbor_strategy!r}): the keyword chooses the "
                             f"build of a periodic list, and {self.periodic_refusal}")
        if neighbor_strategy not in ("brute", "shared", "cell"):
            raise ValueError(f"Unknown neighbor_strategy {neighbor_strategy!r}: brute, shared or cell")
        init(self, *args, **kwargs)
        self.periodic = bool(periodic)
        self.neighbor_strategy = neighbor_strategy
    return with_options


class PairPrior(BasePrior):
    # host-side status of the last list build, not model state: a model that already ran eagerly still scripts
    __jit_ignored_attributes__ = ["static_capacity", "last_overflow", "last_num_pairs", "cell_bound"]

    # a prior that cannot be periodic says why here (Coulomb)
    periodic_refusal: Optional[str] = None

    def __init__(self):
        super().__init__()
        self.periodic = False
        self.neighbor_strategy = "brute"
        # strategy "cell" with a device box (1, 3, 3): the host (3, 3) box that bounds the cells the build gets
        # room for (kernels.build_graph; required with static_capacity, where nothing is read back)
        self.cell_bound = None
        # HIP-graph mode: fixed pair capacity of this prior's own list, no host synchronisation
        self.static_capacity = None
        self.last_overflow = None
        self.last_num_pairs = None

    def reset_parameters(self):
        pass

    def post_reduce_box(self, y: Tensor, z: Tensor, pos: Tensor, batch: Tensor, extra_args, box: Optional[Tensor]):
        """``post_reduce`` with the call's box, the entry ``TorchMD_Net`` uses for the pair priors.  It is a method
        of its own because a scripted model calls ``post_reduce`` with the five reference arguments, and TorchScript
        binds the stub of a ``torch.jit.unused`` method without its defaults: a sixth parameter there, keyword or
        not, stops a model holding the prior from compiling.  Here: a prior that never takes a box (Coulomb)."""
        return self.post_reduce(y, z, pos, batch, extra_args)

    def _periodic_args(self):
        """The part of ``get_init_args`` that exists only when it is not the default, so the saved
        hyperparameters of a non-periodic prior are what they were."""
        args = {}
        if self.periodic:
            args["periodic"] = True
        if self.neighbor_strategy != "brute":
            args["neighbor_strategy"] = self.neighbor_strategy
        return args

    def _graph(self, pos: Tensor, batch: Tensor, cutoff: float, box: Optional[Tensor] = None, n_mol: int = 1):
        from .. import kernels
        if not self.periodic or box is None or box.numel() == 0:
            box, strategy, bound = None, "brute", None
        else:
            strategy, bound = self.neighbor_strategy, self.cell_bound
            if strategy != "cell" and box.dim() == 3 and box.shape[0] == 1 and n_mol > 1:
                # the one device box of a model on the cell list serves every molecule: the all-pairs builds
                # take one box per molecule (the build makes its contiguous float64 copy: n_mol * 72 bytes per call)
                box = box.expand(n_mol, 3, 3)
        g = kernels.build_graph(pos, batch, 0.0, cutoff, int(self.max_num_neighbors) * pos.shape[0], loop=False,
                                strategy=strategy, box=box, check_errors=True,
                                static_capacity=self.static_capacity, cell_bound=bound)
        # the device-side status only (see OptimizedDistance.graph): not the graph and its autograd history
        self.last_overflow = getattr(g, "overflow", None)
        self.last_num_pairs = g.num_pairs_dev if g.num_pairs_dev is not None else g.num_pairs
        return g

    def _add_energy(self, y: Tensor, kind: str, graph, a, b, consts, batch: Tensor):
        from .. import kernels
        e = kernels.pair_prior(kind, graph, a, b, consts, batch, y.shape[0])
        return y + e.to(y.dtype).reshape(y.shape)
