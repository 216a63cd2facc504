"""Inputs and the yardstick of the open-molecule tests: one batch in which a molecule without a box (an all-zero
entry of the ``(n_molecules, 3, 3)`` boxes) sits between periodic ones.  test_open_molecules_cpu.py checks this
file on the CPU; test_gpu_open_molecules.py and test_gpu_periodic_priors.py run the HIP build, the models and the
pair priors over it.

``reference`` is tests/batch_box_ref.py's, molecule by molecule through ``neighbor_cases.reference`` (the dense fp64
all-pairs restatement), with ``box=None`` for an open molecule.

The batch, cutoff 3.0:

    molecule 0   70 atoms   rectangular (7.0, 7.5, 8.0)   a row's candidates span two 64-lane iterations
    molecule 1    9 atoms   open                          a 14-long chain
    molecule 2   33 atoms   triclinic, all three skews
    molecule 3    1 atom    rectangular (7.0, 7.0, 7.0)

The boxed molecules are ``batch_box_ref._molecule``'s (spread around the cell's far corner, a third of the atoms in
other images).  The seed keeps every pair distance ``neighbor_cases.MARGIN * cutoff`` away from the cutoff in both
dtypes (asserted on the CPU), so pair sets are compared exactly.
"""
import functools
import types

import numpy as np

import batch_box_ref as BB
import neighbor_cases as NC

CUTOFF = 3.0
SIZES = (70, 9, 33, 1)
OPEN = 1
BOXES = np.array([
    [[7.0, 0.0, 0.0], [0.0, 7.5, 0.0], [0.0, 0.0, 8.0]],
    [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]],
    [[8.0, 0.0, 0.0], [1.5, 7.5, 0.0], [-2.0, 2.5, 8.0]],
    [[7.0, 0.0, 0.0], [0.0, 7.0, 0.0], [0.0, 0.0, 7.0]],
])
SEED = 3


def is_open(box):
    return not np.any(np.asarray(box) != 0)


def _chain(n, length, rng):
    """n atoms along x over ``length``, jittered by up to 0.3 in every direction, somewhere off the origin."""
    pos = np.zeros((n, 3))
    pos[:, 0] = np.linspace(0.0, length, n)
    return pos + rng.uniform(-0.3, 0.3, (n, 3)) + np.array([2.0, -1.0, 0.5])


@functools.lru_cache(maxsize=None)
def get(dtype, shuffled=False):
    """The batch in ``dtype`` ("f32" / "f64"); ``shuffled``: its atoms in a fixed random order, so the batch vector
    descends and the build scans every atom for every destination.  Shared: treat as read-only."""
    dt = NC.DTYPES[dtype]
    rng = np.random.default_rng(SEED)
    mols = [_chain(n, 14.0, rng) if is_open(BOXES[m]) else BB._molecule(n, BOXES[m], rng)
            for m, n in enumerate(SIZES)]
    pos = np.concatenate(mols)
    batch = np.repeat(np.arange(len(SIZES)), SIZES)
    z = rng.choice([1, 6, 7, 8], len(pos))
    if shuffled:
        order = np.random.default_rng(SEED + 1).permutation(len(pos))
        pos, batch, z = pos[order], batch[order], z[order]
        assert (np.diff(batch) < 0).any()
    c = types.SimpleNamespace(pos=np.ascontiguousarray(pos.astype(dt)), batch=batch.astype(np.int64),
                              z=z.astype(np.int64), boxes=BOXES.copy(), cutoff=CUTOFF, lower=0.0, sizes=SIZES,
                              dtype=dtype, shuffled=shuffled)
    for a in (c.pos, c.batch, c.z, c.boxes):
        a.setflags(write=False)
    return c


def reference(pos, batch, boxes, cutoff_lower, cutoff_upper, loop=True, include_transpose=True):
    """``batch_box_ref.reference`` with ``box=None`` for the molecules whose box is all zero."""
    pos, batch = np.asarray(pos), np.asarray(batch)
    pairs, deltas, dists = [], [], []
    for m in np.unique(batch):
        idx = np.flatnonzero(batch == m)
        box = None if is_open(boxes[m]) else boxes[m]
        p, d, r = NC.reference(pos[idx], np.zeros(len(idx), dtype=np.int64), box, cutoff_lower, cutoff_upper,
                               loop, include_transpose)
        pairs.append(idx[p])
        deltas.append(d)
        dists.append(r)
    pairs = np.concatenate(pairs, axis=1).astype(np.int64)
    return NC.sort_edges(pairs, np.concatenate(deltas), np.concatenate(dists))


@functools.lru_cache(maxsize=None)
def ref(dtype, shuffled=False, loop=True, include_transpose=True):
    """``reference`` over ``get(dtype, shuffled)``, computed once per process.  Shared: treat as read-only."""
    c = get(dtype, shuffled)
    out = reference(c.pos, c.batch, c.boxes, c.lower, c.cutoff, loop, include_transpose)
    for a in out:
        a.setflags(write=False)
    return out


def margin_ok(c):
    band = NC.MARGIN * c.cutoff
    d = reference(c.pos, c.batch, c.boxes, 0.0, c.cutoff + 2 * band, False, True)[2]
    return not np.any(np.abs(d - c.cutoff) <= band)


def pair_set(pos, box, cutoff):
    """The unordered pairs of one molecule under ``box`` (None: open) as a set of (i, j), i < j."""
    p = NC.reference(pos, np.zeros(len(pos), dtype=np.int64), box, 0.0, cutoff, loop=False, include_transpose=False)[0]
    return {(int(min(a, b)), int(max(a, b))) for a, b in p.T}


def check_fixture(c):
    """What the tests rely on, from the oracle: wrapping the open molecule in either neighbouring box would change
    its pair set, and every boxed molecule with more than one atom has a pair that exists only through a face."""
    assert not c.shuffled
    starts = np.concatenate([[0], np.cumsum(c.sizes)])
    mol = lambda m: np.asarray(c.pos[starts[m]:starts[m + 1]], dtype=np.float64)
    open_pairs = pair_set(mol(OPEN), None, c.cutoff)
    assert len(open_pairs) >= len(mol(OPEN)) - 1  # a chain: every atom has a neighbour
    for m in (OPEN - 1, OPEN + 1):
        assert not is_open(c.boxes[m]) and pair_set(mol(OPEN), c.boxes[m], c.cutoff) != open_pairs
    for m, n in enumerate(c.sizes):
        if n > 1 and not is_open(c.boxes[m]):
            assert pair_set(mol(m), c.boxes[m], c.cutoff) - pair_set(mol(m), None, c.cutoff)
    ext = mol(OPEN).max(0) - mol(OPEN).min(0)
    assert ext.max() >= 13.0
