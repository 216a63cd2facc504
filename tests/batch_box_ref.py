"""Inputs and the yardstick of the per-molecule-box tests (test_batch_boxes_cpu.py checks this file on the
CPU, test_gpu_batch_boxes.py runs the HIP build and the models over it).

``reference`` calls ``neighbor_cases.reference`` -- the dense fp64 all-pairs restatement -- once per molecule
with that molecule's box and concatenates the lists with the molecules' atom indices put back.  It shares no
code with the kernels.

The main input: four molecules of 70, 33, 1 and 65 atoms (a row longer than one 64-candidate iteration, a
single atom, a wave-boundary size), cutoff 3.0, boxes cubic 7.0, orthorhombic (6.5, 8, 11), a reduced
triclinic box with all three skew entries non-zero and a 30.0 cube.  A third of the atoms are displaced by
+-1 and +-3 box vectors of their own box.  The seeds keep every pair distance ``neighbor_cases.MARGIN * cutoff``
away from the cutoff (asserted on the CPU), so pair sets are compared exactly.
"""
import functools
import types

import numpy as np

import neighbor_cases as NC

CUTOFF = 3.0
SIZES = (70, 33, 1, 65)
BOXES = np.array([
    [[7.0, 0.0, 0.0], [0.0, 7.0, 0.0], [0.0, 0.0, 7.0]],
    [[6.5, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 11.0]],
    [[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-2.0, 2.5, 10.0]],
    [[30.0, 0.0, 0.0], [0.0, 30.0, 0.0], [0.0, 0.0, 30.0]],
])
SEEDS = {"main": 1, "interleaved": 2}  # fixed so that MARGIN holds in both dtypes (asserted on the CPU)


def _molecule(n, box, rng):
    """n atoms spread over a region of at most 8 length units per lattice axis around the cell's far corner
    (so that pairs cross the faces, in the 30.0 cube too); every third atom moved by +-1 or +-3 box vectors."""
    lengths = np.array([box[0, 0], box[1, 1], box[2, 2]])
    frac = 1.0 + rng.uniform(-0.5, 0.5, (n, 3)) * np.minimum(1.0, 8.0 / lengths)
    pos = frac @ box
    k = np.arange(n) % 3 == 0
    shifts = rng.choice(np.array([-3, -1, 1, 3]), (n, 3))
    pos[k] += shifts[k] @ box
    return pos


def _case(sizes, box_ids, seed, interleave, dt):
    rng = np.random.default_rng(seed)
    boxes = np.ascontiguousarray(BOXES[list(box_ids)])
    pos = np.concatenate([_molecule(n, boxes[m], rng) for m, n in enumerate(sizes)])
    batch = np.repeat(np.arange(len(sizes)), sizes)
    if interleave:  # atoms of the molecules alternate: the batch descends at every other atom
        order = np.argsort(np.concatenate([np.arange(n) for n in sizes]), kind="stable")
        pos, batch = pos[order], batch[order]
        assert (np.diff(batch) < 0).any()
    c = types.SimpleNamespace(pos=np.ascontiguousarray(pos.astype(dt)), batch=batch.astype(np.int64), boxes=boxes,
                              cutoff=CUTOFF, lower=0.0, sizes=tuple(sizes))
    c.pos.setflags(write=False)
    c.batch.setflags(write=False)
    c.boxes.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def get(name, dtype):
    """Inputs of ``name`` ("main": the four molecules, sorted batch; "interleaved": 40 and 37 atoms alternating,
    the cubic and the triclinic box) in ``dtype`` ("f32" / "f64").  Shared: treat as read-only."""
    dt = NC.DTYPES[dtype]
    if name == "main":
        c = _case(SIZES, (0, 1, 2, 3), SEEDS[name], False, dt)
    else:
        c = _case((40, 37), (0, 2), SEEDS[name], True, dt)
    c.name, c.dtype = name, dtype
    return c


def reference(pos, batch, boxes, cutoff_lower, cutoff_upper, loop=True, include_transpose=True):
    """Per-molecule-box neighbour list in fp64: ``neighbor_cases.reference`` over the atoms of each molecule
    with ``boxes[m]``, the molecule's atom indices put back, all lists concatenated and ordered by
    (destination, source).  Returns (pairs [2, P], deltas [P, 3], distances [P])."""
    pos, batch = np.asarray(pos), np.asarray(batch)
    pairs, deltas, dists = [], [], []
    for m in np.unique(batch):
        idx = np.flatnonzero(batch == m)
        p, d, r = NC.reference(pos[idx], np.zeros(len(idx), dtype=np.int64), boxes[m], cutoff_lower, cutoff_upper,
                               loop, include_transpose)
        pairs.append(idx[p])
        deltas.append(d)
        dists.append(r)
    pairs = np.concatenate(pairs, axis=1).astype(np.int64)
    return NC.sort_edges(pairs, np.concatenate(deltas), np.concatenate(dists))


@functools.lru_cache(maxsize=None)
def ref(name, dtype, loop=True, include_transpose=True):
    """``reference`` over the inputs ``name``, computed once per process.  Shared: treat as read-only."""
    c = get(name, dtype)
    out = reference(c.pos, c.batch, c.boxes, c.lower, c.cutoff, loop, include_transpose)
    for a in out:
        a.setflags(write=False)
    return out


def margin_ok(c):
    """No pair distance within MARGIN * cutoff of the cutoff, on the fp64 reference built with the cutoff
    widened by two margins (distances just outside matter as much)."""
    band = NC.MARGIN * c.cutoff
    d = reference(c.pos, c.batch, c.boxes, 0.0, c.cutoff + 2 * band, False, True)[2]
    return not np.any(np.abs(d - c.cutoff) <= band)
