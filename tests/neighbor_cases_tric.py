"""Inputs of the triclinic cell-list tests (test_neighbor_cases_tric_cpu.py checks this file on the CPU,
test_gpu_neighbor_tric.py runs the HIP builders over it).

The yardstick is ``neighbor_cases.reference`` (dense fp64, all pairs, the triclinic ``round()`` image).  This
file adds the boxes, a NumPy restatement of the grid rule (csrc/neighbors.hip ``cell_dims``) and of the
binning (``cell_of_tric`` / ``cell_frac``) in the kernel's operation order with every operation rounded to
the dtype, and generators that put atoms on the faces of the fractional cells: at fractional coordinate 0,
1 and every k / n along each lattice axis, converted to Cartesian in the dtype, with the Cartesian
neighbours one ulp either side, each repeated at the lattice images of ``neighbor_cases.SHIFTS``.  Every
case is seeded so that no pair distance comes within ``MARGIN * cutoff`` of a cutoff in either dtype.
"""
import functools
import types

import numpy as np

import neighbor_cases as NC

DTYPES = NC.DTYPES

# name -> (box rows a, b, c; cutoff; cells per lattice axis)
BOXES = {
    "t15": (((15.0, 0.0, 0.0), (3.0, 15.0, 0.0), (-2.0, 4.0, 15.0)), 5.0, (3, 3, 3)),
    "t31": (((31.0, 0.0, 0.0), (7.0, 23.0, 0.0), (-5.0, 6.0, 17.5)), 4.0, (6, 5, 4)),
    "tmax": (((24.0, 0.0, 0.0), (12.0, 24.0, 0.0), (12.0, 12.0, 24.0)), 3.0, (6, 7, 8)),
    "tneg": (((24.0, 0.0, 0.0), (-12.0, 24.0, 0.0), (12.0, -12.0, 24.0)), 3.0, (6, 7, 8)),
}


def box_of(name):
    return np.array(BOXES[name][0], dtype=np.float64)


# ----------------------------------------------------------------------------- grid and binning
def widths(box):
    """Perpendicular widths of the cell along a, b, c: V/|b x c|, V/|c x a|, V/|a x b|, in the host
    arithmetic of cell_dims (double)."""
    (a0, _, _), (b0, b1, _), (c0, c1, c2) = np.asarray(box, dtype=np.float64).tolist()
    bc = (b1 * c2, -b0 * c2, b0 * c1 - b1 * c0)
    return (abs(a0 * b1 * c2) / np.sqrt(bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]),
            abs(b1 * c2) / np.sqrt(c1 * c1 + c2 * c2), abs(c2))


def grid(box, cut):
    """Cells per lattice axis: max(3, floor(width / cutoff))."""
    return tuple(max(3, int(w / cut)) for w in widths(box))


def fractional(pos, box, dt):
    """Fractional coordinates (sx, sy, sz) by forward substitution, each operation rounded to ``dt``."""
    p = np.asarray(pos, dtype=dt)
    (a0, _, _), (b0, b1, _), (c0, c1, c2) = [[dt(v) for v in row] for row in np.asarray(box).tolist()]
    sz = p[:, 2] / c2
    sy = (p[:, 1] - sz * c1) / b1
    sx = (p[:, 0] - sz * c0 - sy * b0) / a0
    assert sx.dtype == sy.dtype == sz.dtype == dt
    return sx, sy, sz


def cell_frac(s, n, dt):
    """cell_frac of csrc/neighbors.hip: floor((s - floor(s)) * n); not below n -> 0, negative -> n - 1."""
    s = np.asarray(s, dtype=dt)
    f = np.floor((s - np.floor(s)) * dt(n))
    return np.where(~(f < n), 0, np.where(f < 0, n - 1, f)).astype(np.int64)


def cells(pos, box, cut, dt):
    """([cx, cy, cz], (nx, ny, nz)) of every atom, as k_cell_assign<T, true> keys them."""
    ns = grid(box, cut)
    with np.errstate(invalid="ignore", over="ignore"):
        return [cell_frac(s, n, dt) for s, n in zip(fractional(pos, box, dt), ns)], ns


# ----------------------------------------------------------------------------- generators
def to_cartesian(frac, box, dt):
    """frac @ box with every operation in ``dt`` (x = fx a0 + fy b0 + fz c0, ...)."""
    f = np.asarray(frac, dtype=dt)
    b = np.asarray(box).astype(dt)
    out = np.zeros(f.shape, dtype=dt)
    for j in range(3):
        out[..., j] = f[..., 0] * b[0, j] + f[..., 1] * b[1, j] + f[..., 2] * b[2, j]
    return out


def probe_fractions(n):
    """Both faces of the box and every cell boundary between them."""
    return [k / n for k in range(n + 1)]


def face_atoms(box, cut, dt, rng):
    """Per lattice axis i: fractional coordinate i at 0, 1 and every k / n_i, shifted by every image of
    SHIFTS, the other two fractional coordinates random in [0, 1); the Cartesian position in ``dt``, and
    its neighbours one ulp below and above in Cartesian component i (the component that moves s_i alone
    among the coordinates the substitution has not fixed yet)."""
    out = []
    for ax, n in enumerate(grid(box, cut)):
        for f in probe_fractions(n):
            for k in NC.SHIFTS:
                frac = rng.uniform(0.0, 1.0, 3)
                frac[ax] = f + k
                p = to_cartesian(frac, box, dt)
                for v in NC._ulps(p[ax], dt):
                    q = p.copy()
                    q[ax] = v
                    out.append(q)
    return np.stack(out)


def _case(pos, batch, boxname, strategies, lower=0.0, loop=True, transpose=True):
    cut = BOXES[boxname][1]
    box = box_of(boxname)
    return types.SimpleNamespace(
        pos=np.ascontiguousarray(pos), batch=np.ascontiguousarray(batch, dtype=np.int64),
        lengths=tuple(float(box[i, i]) for i in range(3)), box=box, boxname=boxname, cutoff=float(cut),
        lower=float(lower), loop=loop, transpose=transpose, strategies=tuple(strategies))


def _face(boxname):
    def make(dt, rng):
        _, cut, _ = BOXES[boxname]
        box = box_of(boxname)
        probes = face_atoms(box, cut, dt, rng)
        fill = to_cartesian(rng.uniform(-0.6, 0.6, (100, 3)), box, dt)  # wrapped by the periodic box
        pos = np.concatenate([probes, fill])
        return _case(pos, np.zeros(len(pos)), boxname, NC.ALL3)
    return make


def _uniform(n, boxname, rng, dt, spread=0.75):
    return to_cartesian(rng.uniform(-spread, spread, (n, 3)), box_of(boxname), dt)


# fractional coordinates of the two atoms of n2: they differ by about (-0.95, -0.93, +0.94), so the
# image takes one c off, then (the c step moved y by c1) one b on, then one a on: every step of the
# c-then-b-then-a order acts, and the pair sits across the skewed c face
N2_FRAC = np.array([[0.02, 0.03, 0.97], [0.97, 0.96, 0.03]])


def _tiny(n):
    def make(dt, rng):
        pos = to_cartesian(N2_FRAC[:n], box_of("t31"), dt)
        return _case(pos, np.zeros(n), "t31", ("cell",))
    return make


def _boxed(n, **kw):
    def make(dt, rng):
        return _case(_uniform(n, "t31", rng, dt), np.zeros(n), "t31", ("cell",), **kw)
    return make


def _molecules(shuffled):
    def make(dt, rng):
        batch = np.repeat(np.arange(3), [70, 90, 60])
        pos = _uniform(220, "t31", rng, dt)
        if shuffled:
            batch = batch[rng.permutation(220)]
            assert (np.diff(batch) < 0).any()
        return _case(pos, batch, "t31", ("cell",))
    return make


# name -> (maker, seed).  The seeds are the first for which MARGIN holds in both dtypes (found by search
# on the CPU; test_neighbor_cases_tric_cpu.py asserts the condition).
CASES = {
    "face_t15": (_face("t15"), 7), "face_t31": (_face("t31"), 1),
    "face_tmax": (_face("tmax"), 0), "face_tneg": (_face("tneg"), 0),
    "grid_n1": (_tiny(1), 0), "grid_n2": (_tiny(2), 0), "grid_n257": (_boxed(257), 0),
    "grid_mols_sorted": (_molecules(False), 0), "grid_mols_shuffled": (_molecules(True), 0),
    "grid_noloop": (_boxed(150, loop=False), 0), "grid_half": (_boxed(150, transpose=False), 0),
    "grid_half_noloop": (_boxed(150, loop=False, transpose=False), 0),
    "grid_lower": (_boxed(150, lower=2.0), 0),
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
    """``neighbor_cases.reference`` over case ``name``, computed once per process.  Read-only."""
    c = get(name, dtype)
    out = NC.reference(c.pos, c.batch, c.box, c.lower, c.cutoff, c.loop, c.transpose)
    for a in out:
        a.setflags(write=False)
    return out
