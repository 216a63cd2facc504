"""Inputs and the yardstick of the neighbour-list edge tests (test_neighbor_cases_cpu.py checks this file
on the CPU, test_gpu_neighbor_edges.py runs the HIP builders over it).

``reference`` is a dense fp64 all-pairs restatement of the op; it shares no code with the kernels, with
the reference project's cell list (whose ``getCell`` the kernels restate, face defect included) or with
the C oracle.  The generators put atoms where uniformly random positions never land: on the box faces,
on the cell boundaries, one ulp either side of them and on their periodic images, each value formed in
the dtype the GPU will see.  Every case is seeded so that no pair distance comes within
``MARGIN * cutoff`` of a cutoff: pair sets are then compared exactly.
"""
import functools
import types

import numpy as np

MARGIN = 1e-4  # of the cutoff; the fp32 error of a delta at |coordinate| <= ~110 is about 1e-5
SHIFTS = (0, -3, -1, 1, 3)  # periodic images (in box lengths) every probed value is repeated at
DTYPES = {"f32": np.float32, "f64": np.float64}


# ----------------------------------------------------------------------------- dense reference
def _round(x):
    """Half away from zero, as C ``round`` (np.round is half-to-even)."""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def reference(pos, batch, box, cutoff_lower, cutoff_upper, loop=True, include_transpose=True, block=256):
    """All-pairs neighbour list in fp64.  ``pos`` holds exactly the values the GPU sees; ``box`` is a
    (3, 3) array of box vectors (rows a, b, c) or None.  Returns (pairs [2, P] = (source, destination),
    deltas [P, 3] = pos[s] - pos[t] (minimum image), distances [P]), destinations ascending and the
    sources ascending within each (rows of destinations are formed ``block`` at a time)."""
    p = np.asarray(pos, dtype=np.float64)
    b = np.asarray(batch)
    n = p.shape[0]
    src, dst, dlt = [], [], []
    for t0 in range(0, n, block):
        t = np.arange(t0, min(n, t0 + block))
        d = p[None, :, :] - p[t, None, :]
        if box is not None:  # triclinic minimum image: round(), c then b then a
            va, vb, vc = np.asarray(box, dtype=np.float64)
            d = d - _round(d[..., 2:3] / vc[2]) * vc
            d = d - _round(d[..., 1:2] / vb[1]) * vb
            d = d - _round(d[..., 0:1] / va[0]) * va
        r = np.sqrt((d * d).sum(-1))
        s = np.arange(n)[None, :]
        same = s == t[:, None]
        keep = (b[None, :] == b[t][:, None]) & (r >= cutoff_lower) & (r < cutoff_upper) & ~same
        if loop:
            keep |= same  # the self pair is kept whatever the lower cutoff
        if not include_transpose:
            keep &= s >= t[:, None]
        ti, si = np.nonzero(keep)
        src.append(si)
        dst.append(t[ti])
        dlt.append(d[ti, si])
    pairs = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    deltas = np.concatenate(dlt).reshape(-1, 3)
    return pairs, deltas, np.sqrt((deltas * deltas).sum(-1))


def row_ptr_of(pairs, n):
    """CSR row pointer of a destination-grouped list: cumulative pair counts per destination."""
    return np.concatenate([[0], np.cumsum(np.bincount(pairs[1], minlength=n))]).astype(np.int64)


def sort_edges(pairs, *per_edge):
    """Edges ordered by (destination, source); the pairs must be unique."""
    n = int(pairs.max()) + 1 if pairs.size else 1
    key = pairs[1].astype(np.int64) * n + pairs[0]
    assert len(np.unique(key)) == len(key), "duplicate pairs"
    o = np.argsort(key)
    return (pairs[:, o],) + tuple(a[o] for a in per_edge)


# ----------------------------------------------------------------------------- cell arithmetic
def grid(L, cut):
    """Cells per axis of the cell list (csrc/neighbors.hip cell_dims)."""
    return max(3, int(L / cut))


def _cell_raw(x, L, cut, dt):
    """The kernel's wrap and cell arithmetic in its operation order, every operation rounded to ``dt``."""
    x, L, cut, half = np.asarray(x, dtype=dt), dt(L), dt(cut), dt(0.5)
    w = x - np.floor(x / L + half) * L
    return np.floor((w + half * L) / cut)


def cell_index_parent(x, L, cut, dt):
    """Cell index before the fix: only an index equal to the cell count is folded (to 0)."""
    c = _cell_raw(x, L, cut, dt).astype(np.int64)
    return np.where(c == grid(L, cut), 0, c)


def cell_index(x, L, cut, dt):
    """Cell index of csrc/neighbors.hip cell_axis: anything not below the count -> 0, negative -> n - 1."""
    f, n = _cell_raw(x, L, cut, dt), grid(L, cut)
    return np.where(~(f < n), 0, np.where(f < 0, n - 1, f)).astype(np.int64)


# ----------------------------------------------------------------------------- generators
def probe_centres(L, cut):
    """Faces, the origin, every interior cell boundary and the start of the folded partial cell."""
    n = grid(L, cut)
    c = {-L / 2, L / 2, 0.0, int(L / cut) * cut - L / 2}
    c |= {k * cut - L / 2 for k in range(1, n) if k * cut < L}
    return sorted(c)


def _ulps(v, dt):
    v = dt(v)
    return [np.nextafter(v, dt(-np.inf)), v, np.nextafter(v, dt(np.inf))]


def face_atoms(Ls, cut, dt, rng):
    """Probe atoms: per axis, each centre and one ulp either side of it, at every image; the other two
    coordinates random.  Then, per axis, atoms one ulp below the +L/2 face (and its images) whose other
    two coordinates lie inside the first cell: the parent's key for them is negative."""
    out = []
    for ax in range(3):
        L = Ls[ax]
        others = [a for a in range(3) if a != ax]
        for first_cell in (False, True):
            centres = [L / 2] if first_cell else probe_centres(L, cut)
            for c in centres:
                for k in SHIFTS:
                    vals = _ulps(c + k * L, dt)
                    for v in (vals[:1] if first_cell else vals):
                        p = np.zeros(3, dtype=dt)
                        p[ax] = v
                        for o in others:
                            lo, hi = (-Ls[o] / 2 + 0.1 * cut, -Ls[o] / 2 + 0.9 * cut) if first_cell \
                                else (-Ls[o] / 2, Ls[o] / 2)
                            p[o] = dt(rng.uniform(lo, hi))
                        out.append(p)
    return np.stack(out)


def _case(pos, batch, box, cutoff, strategies, lower=0.0, loop=True, transpose=True):
    Ls = None if box is None else tuple(float(v) for v in box)
    return types.SimpleNamespace(
        pos=np.ascontiguousarray(pos), batch=np.ascontiguousarray(batch, dtype=np.int64), lengths=Ls,
        box=None if box is None else np.diag(np.asarray(box, dtype=np.float64)), cutoff=float(cutoff),
        lower=float(lower), loop=loop, transpose=transpose, strategies=tuple(strategies))


ALL3 = ("cell", "brute", "shared")
FACE_BOXES = {"b15": ((15.0, 15.0, 15.0), 5.0), "b31": ((31.0, 23.0, 17.5), 5.0), "b12": ((12.0, 12.0, 12.0), 3.0),
              "nobox": (None, 5.0)}


def _face(boxname, rem):
    def make(dt, rng):
        Ls, cut = FACE_BOXES[boxname]
        bin_L = Ls if Ls is not None else (3 * cut,) * 3  # build_graph's substitute box
        probes = face_atoms(bin_L, cut, dt, rng)
        nfill = 100 + (rem - len(probes) - 100) % 4
        # fillers reach past the faces (periodic boxes wrap them; without a box the outer ones are far)
        fill = np.stack([rng.uniform(-0.6 * L, 0.6 * L, nfill) for L in bin_L], axis=1).astype(dt)
        pos = np.concatenate([probes, fill])
        assert len(pos) % 4 == rem
        return _case(pos, np.zeros(len(pos)), Ls, cut, ALL3 if Ls is not None else ("cell",))
    return make


def _uniform(n, Ls, rng, dt, spread=0.75):
    return np.stack([rng.uniform(-spread * L, spread * L, n) for L in Ls], axis=1).astype(dt)


def _one_cell(dt, rng):  # every atom in cell (0, 0, 0) or a periodic image of it
    Ls, cut = (15.0,) * 3, 5.0
    pos = rng.uniform(-7.4, -2.6, (48, 3))
    pos += rng.integers(-2, 3, (48, 3)) * 15.0
    return _case(pos.astype(dt), np.zeros(48), Ls, cut, ("cell",))


def _sparse(dt, rng):  # 8x8x8 cells, 36 atoms in distinct cells plus two close pairs (one across a face)
    Ls, cut = (40.0,) * 3, 5.0
    cells = rng.choice(512, 36, replace=False)
    ijk = np.stack([cells % 8, (cells // 8) % 8, cells // 64], axis=1)
    pos = (ijk + 0.5) * cut - 20.0 + rng.uniform(-2.0, 2.0, (36, 3))
    extra = np.array([[19.0, 1.0, 1.0], [-19.0, 1.5, 1.0], [-0.2, -11.0, -12.0], [0.3, -10.0, -11.0]])
    return _case(np.concatenate([pos, extra]).astype(dt), np.zeros(40), Ls, cut, ("cell",))


def _tiny(n):
    def make(dt, rng):
        pos = np.array([[7.3, 0.2, -0.4], [-7.4, 0.1, 0.3]])[:n]
        return _case(pos.astype(dt), np.zeros(n), (15.0,) * 3, 5.0, ("cell",))
    return make


def _boxed(n, **kw):
    def make(dt, rng):
        Ls = (15.0, 15.0, 15.0)
        return _case(_uniform(n, Ls, rng, dt), np.zeros(n), Ls, 5.0, ("cell",), **kw)
    return make


def _molecules(shuffled):
    def make(dt, rng):
        Ls = (15.0, 15.0, 15.0)
        batch = np.repeat(np.arange(3), [70, 90, 60])
        pos = _uniform(220, Ls, rng, dt)
        if shuffled:
            batch = batch[rng.permutation(220)]
            assert (np.diff(batch) < 0).any()
        return _case(pos, batch, Ls, 5.0, ("cell",))
    return make


ROWS = ("brute", "shared")


def _blobs(sizes, rng, dt, sigma=2.0):
    return np.concatenate([rng.normal(0.0, sigma, (m, 3)) + 9.0 * i for i, m in enumerate(sizes)]).astype(dt)


def _segments(**kw):
    def make(dt, rng):
        sizes = [63, 64, 65, 129, 1]
        return _case(_blobs(sizes, rng, dt), np.repeat(np.arange(5), sizes), None, 5.0, ROWS, **kw)
    return make


def _descent_mid(dt, rng):  # n = 600: the only descent sits between atoms 255 and 256
    batch = np.concatenate([np.repeat([0, 2], [128, 128]), np.repeat([1, 3], [200, 144])])
    assert np.flatnonzero(np.diff(batch) < 0).tolist() == [255]
    return _case(rng.uniform(-6.0, 6.0, (600, 3)).astype(dt), batch, None, 3.0, ROWS)


def _descent_last(dt, rng):  # the only descent sits between atoms n-2 and n-1
    n = 321
    batch = np.concatenate([np.repeat([0, 1], [150, n - 151]), [0]])
    assert np.flatnonzero(np.diff(batch) < 0).tolist() == [n - 2]
    return _case(rng.uniform(-5.0, 5.0, (n, 3)).astype(dt), batch, None, 3.0, ROWS)


def _scan(n):  # a few pairs per atom: density 0.72 at cutoff 1 -> about three neighbours
    def make(dt, rng):
        L = max(4.0, round(2 * (n / 0.72) ** (1 / 3)) / 2)
        Ls = (L, L, L)
        return _case(_uniform(n, Ls, rng, dt, spread=0.5), np.zeros(n), Ls, 1.0, ("brute", "cell"))
    return make


# name -> (maker, seed).  The seeds are fixed so that MARGIN holds in both dtypes (asserted on the CPU).
CASES = {
    "face_b15_n0": (_face("b15", 0), 655), "face_b15_n1": (_face("b15", 1), 213),
    "face_b31_n0": (_face("b31", 0), 9), "face_b31_n1": (_face("b31", 1), 9),
    "face_b12_n0": (_face("b12", 0), 6), "face_b12_n1": (_face("b12", 1), 1),
    "face_nobox_n0": (_face("nobox", 0), 5), "face_nobox_n1": (_face("nobox", 1), 1),
    "grid_one_cell": (_one_cell, 2), "grid_sparse": (_sparse, 1),
    "grid_n1": (_tiny(1), 1), "grid_n2": (_tiny(2), 1), "grid_n257": (_boxed(257), 60),
    "grid_mols_sorted": (_molecules(False), 2), "grid_mols_shuffled": (_molecules(True), 6),
    "grid_noloop": (_boxed(150, loop=False), 1), "grid_half": (_boxed(150, transpose=False), 1),
    "grid_half_noloop": (_boxed(150, loop=False, transpose=False), 1),
    "grid_lower": (_boxed(150, lower=2.0), 1),
    "rows_segments": (_segments(), 30), "rows_descent_mid": (_descent_mid, 1),
    "rows_descent_last": (_descent_last, 3), "rows_half": (_segments(transpose=False), 30),
    "rows_lower_loop": (_segments(lower=2.0, loop=True), 30),
    "scan_1": (_scan(1), 1), "scan_1023": (_scan(1023), 6), "scan_1024": (_scan(1024), 2),
    "scan_1025": (_scan(1025), 3), "scan_2049": (_scan(2049), 2),
}
FACE_CASES = [k for k in CASES if k.startswith("face_")]


def names(prefix=""):
    return [k for k in CASES if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def get(name, dtype):
    """The inputs of case ``name`` in ``dtype`` ("f32" / "f64").  Shared: treat as read-only."""
    make, seed = CASES[name]
    c = make(DTYPES[dtype], np.random.default_rng(seed))
    c.name, c.dtype = name, dtype
    c.pos.setflags(write=False)
    c.batch.setflags(write=False)
    return c


def strategies(name):
    """The builders case ``name`` is meant for."""
    return get(name, "f32").strategies


@functools.lru_cache(maxsize=None)
def ref(name, dtype):
    """``reference`` over case ``name``, computed once per process.  Shared: treat as read-only."""
    c = get(name, dtype)
    out = reference(c.pos, c.batch, c.box, c.lower, c.cutoff, c.loop, c.transpose)
    for a in out:
        a.setflags(write=False)
    return out


def margin_ok(c, distances):
    """No pair distance within MARGIN * cutoff of the upper cutoff or of a non-zero lower one.  Distances
    just OUTSIDE a cutoff matter as much, so this is evaluated on a list built with widened cutoffs."""
    band = MARGIN * c.cutoff
    d = distances[distances > 0]
    ok = not np.any(np.abs(d - c.cutoff) <= band)
    if c.lower > 0:
        ok = ok and not np.any(np.abs(d - c.lower) <= band)
    return ok


def widened(c):
    """Distances of every pair inside the cutoffs widened by two margins (the input of margin_ok)."""
    band = 2 * MARGIN * c.cutoff
    return reference(c.pos, c.batch, c.box, max(c.lower - band, 0.0), c.cutoff + band, False, True)[2]
