"""HIP-graph capture of the energy + force evaluation (replaces the reference's CUDA-graph path,
tests/test_model.py:87-126 / benchmarks/neighbors.py:89-99, for the ET and TensorNet models).

The reference ET is not graph-capturable (host syncs in OptimizedDistance.check_errors/resize_to_fit,
output_modules.py:33, utils.py:93).  Here the neighbour graph switches to its static-capacity mode
(no host synchronisation, padded CSR), the molecule count of ``reduce`` is frozen from a warm-up
call (the reference's own capture rule, output_modules.py:27-43), and one HIP graph replays the
whole forward + autograd force pass: ~600 launches become one graph launch.

    gm = GraphedEnergyForces(model, z, pos, batch)      # warm-up + capture
    y, neg_dy = gm(pos_new)                              # copy-in + replay (same z/batch layout)
    gm.check_capacity()                                  # raises if a replay overflowed capacity

``GraphedEnergyForces(..., box=boxes)`` captures a periodic evaluation whose cell can change between replays:
the box -- ``(3, 3)`` or one per molecule ``(n_molecules, 3, 3)`` -- is kept as a static per-molecule device copy
the captured neighbour build reads, and ``gm(pos_new, box=box_new)`` copies a new one into it before the replay
(no box is validated during a replay).  A model whose distance module uses ``strategy="cell"`` keeps ONE device
box ``(1, 3, 3)`` for all molecules and builds its cell list from it on the device; the cell table has room for the
construction box with every lattice vector scaled by ``cell_margin``, and a cell that outgrows it is built on a
coarser grid (exact, slower), not refused.

``GraphedEnergyForces(..., virial=True)`` also keeps the per-molecule virial of every replay in ``gm.virial``.

Pair priors (ZBL, D2, Coulomb) build a neighbour list of their own: each gets its own static capacity from its
own warm-up pair count (``prior_capacity`` overrides it for all of them) and its own overflow flag, which
``check_capacity`` reads besides the representation model's.  A prior built with ``periodic=True`` reads the same
static box as the model, so its list follows ``gm(pos, box=new)`` too; one with ``neighbor_strategy="cell"`` needs
that box to be a single one, and gets the same ``cell_margin`` bound for its cell table.  A model on brute / shared
keeps one static box per molecule, also when one ``(3, 3)`` box was given, so beside such a model a ``"cell"`` prior is
captured over a single molecule only (the eager call has no such limit); put the model on the cell list too.
"""
import math

import torch


def _distance_modules(model):
    from .models.utils import OptimizedDistance
    return [m for m in model.modules() if isinstance(m, OptimizedDistance)]


def pair_priors(model):
    """The model's pair-potential priors (ZBL, D2, Coulomb): each builds a neighbour list of its own."""
    from .priors.pair import PairPrior
    return [p for p in (getattr(model, "prior_model", None) or []) if isinstance(p, PairPrior)]


def cell_bound_of(box, cell_margin):
    """The host ``(3, 3)`` float64 box that sizes a captured cell list: the first (the only) box of ``box`` with
    every lattice vector scaled by ``cell_margin``."""
    b = box.detach().to(device="cpu", dtype=torch.float64).reshape(-1, 3, 3)[0]
    return b * float(cell_margin)


def refuse_pair_priors(model):
    if pair_priors(model):
        raise ValueError("captured training with pair priors (ZBL, D2, Coulomb) is not supported; train "
                         "eagerly with LNNPStep")


class GraphedEnergyForces:
    def __init__(self, model, z, pos, batch, edge_capacity=None, margin=1.25, warmup=3, prior_capacity=None,
                 virial=False, box=None, cell_margin=1.25):
        if not model.derivative:
            raise ValueError("GraphedEnergyForces captures TorchMD_Net(derivative=True)")
        rep = model.representation_model
        from .models.wrappers import BaseWrapper
        if isinstance(rep, BaseWrapper):
            raise ValueError(f"GraphedEnergyForces cannot capture a wrapped representation model "
                             f"({type(rep).__name__} reads the molecule count on the host); run it eagerly")
        self.model = model
        dev = pos.device
        self.z = z.clone()
        self.batch = batch.clone()
        self.pos = pos.detach().clone()
        # the static box the captured build reads: always one float64 box per molecule on the device (a
        # (3, 3) box is repeated), so a replay follows whatever __call__ copies into it
        self.box = None
        self.cell_dists = []  # the modules whose cell_bound this object set: distance modules and "cell" priors
        kw = {}
        if box is not None:
            b = box.detach().to(device=dev, dtype=torch.float64)
            if getattr(rep.distance, "strategy", None) == "cell":
                # the cell list takes one box: (1, 3, 3) for every molecule (the kernels clamp the molecule
                # index), built on the device with room for the construction box scaled by cell_margin
                if b.dim() == 3 and b.shape[0] != 1:
                    from .kernels import _MOLBOX_CELL_ERROR
                    raise RuntimeError(_MOLBOX_CELL_ERROR)
                self.box = b.reshape(1, 3, 3).contiguous().clone()
                self.cell_dists = [rep.distance]
                rep.distance.cell_bound = cell_bound_of(self.box, cell_margin)
            else:
                n_mol = int(self.batch.max()) + 1
                self.box = (b.expand(n_mol, 3, 3) if b.dim() == 2 else b).contiguous().clone()
            # a periodic prior on the cell list builds from the same static box, which must then be one box
            cell_priors = [p for p in pair_priors(model) if p.periodic and p.neighbor_strategy == "cell"]
            if cell_priors and self.box.shape[0] != 1:
                from .kernels import _MOLBOX_CELL_ERROR
                for d in self.cell_dists:
                    d.cell_bound = None
                if b.dim() == 2:
                    # one box was given, but a model on brute / shared reads it as one static box per molecule,
                    # and the prior reads what the model reads
                    raise RuntimeError('a pair prior with neighbor_strategy="cell" is captured with one box beside a '
                                       'model whose distance module is on the cell list too, or over a single '
                                       f'molecule: this batch has {self.box.shape[0]} molecules and the model\'s '
                                       f'strategy is "{getattr(rep.distance, "strategy", None)}", which keeps one '
                                       'static box per molecule')
                raise RuntimeError(_MOLBOX_CELL_ERROR)
            for p in cell_priors:  # the bound is set here and cleared where the distance module's is
                p.cell_bound = cell_bound_of(self.box, cell_margin)
            self.cell_dists = self.cell_dists + cell_priors
            kw = {"box": self.box}
        try:
            self._warm_up_and_capture(model, rep, dev, kw, edge_capacity, margin, warmup, prior_capacity, virial)
        except BaseException:  # no object, so no release(): the bound must not stay on the model's distance module
            for d in self.cell_dists:
                d.cell_bound = None
            raise

    def _warm_up_and_capture(self, model, rep, dev, kw, edge_capacity, margin, warmup, prior_capacity, virial):
        # eager warm-up: sizes the edge capacity and the molecule count (and validates the boxes)
        y, f = model(self.z, self.pos.clone(), self.batch, **kw)
        dists = _distance_modules(model)
        if edge_capacity is None:
            from .models.utils import OptimizedDistance  # noqa: F401
            g = rep.distance.graph(self.pos, self.batch, self.box)
            edge_capacity = int(math.ceil(g.num_pairs * margin / 256.0) * 256)
        self.edge_capacity = int(edge_capacity)
        for d in dists:
            d.static_capacity = self.edge_capacity
        # every pair prior sizes its own list from its own warm-up pair count (same margin and rounding)
        self.priors = pair_priors(model)
        for p in self.priors:
            cap = int(math.ceil(int(p.last_num_pairs) * margin / 256.0) * 256) if prior_capacity is None \
                else int(prior_capacity)
            p.static_capacity = max(cap, 256)  # a warm-up without pairs still gets a list to fill
        self.pos.requires_grad_(True)
        try:  # pos is a leaf created outside the capture stream; its AccumulateGrad is never used
            torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        except AttributeError:
            pass
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(warmup):  # the captured call itself, so every kernel it launches has run once
                (model.energy_forces_virial if virial else model)(self.z, self.pos, self.batch, **kw)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # virial=True: the capture goes through energy_forces_virial; ``self.virial`` is the static
        # [n_mol, 3, 3] tensor (-dE_m/d eps) every replay refreshes, n_mol the warm-up's frozen molecule count
        self.virial = None
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            if virial:
                self.y, self.neg_dy, self.virial = model.energy_forces_virial(self.z, self.pos, self.batch, **kw)
            else:
                self.y, self.neg_dy = model(self.z, self.pos, self.batch, **kw)
        torch.cuda.synchronize(dev)
        # device flag written by every replay (lives in the graph's memory pool)
        self.overflow = rep.distance.last_overflow
        self.prior_overflows = [(type(p).__name__, p.last_overflow) for p in self.priors]
        self.dists = dists

    def __call__(self, pos=None, box=None):
        if pos is not None:
            with torch.no_grad():
                self.pos.copy_(pos)
        if box is not None:
            if self.box is None:
                raise ValueError("GraphedEnergyForces was captured without a box: pass box= at construction")
            with torch.no_grad():
                self.box.copy_(box)  # (3, 3) broadcasts over the molecules
        self.graph.replay()
        return self.y, self.neg_dy

    def check_capacity(self):
        """Host check (synchronises): the last replay's neighbour list fit the static capacity."""
        if bool(self.overflow.item()):
            raise RuntimeError(f"neighbour pairs exceed the captured edge capacity {self.edge_capacity}")
        for name, ov in self.prior_overflows:
            if bool(ov.item()):
                raise RuntimeError(f"neighbour pairs of the {name} prior exceed its captured capacity {ov.capacity}")

    def release(self):
        for d in self.dists:
            d.static_capacity = None
        for d in self.cell_dists:
            d.cell_bound = None
        for p in self.priors:
            p.static_capacity = None
