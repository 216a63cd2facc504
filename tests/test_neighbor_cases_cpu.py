"""CPU checks of tests/neighbor_cases.py: the dense reference against the C oracle, the conditions the
GPU tests rely on (no pair near a cutoff, pairs and cross-boundary pairs present) and -- without a GPU --
that the face cases hold atoms the cell list binned at index -1 before `cell_axis` folded it."""
import numpy as np
import pytest

import neighbor_cases as NC
from oracle import model_oracle as O

ALL = [(name, dt) for name in NC.CASES for dt in NC.DTYPES]
FACES = [(name, dt) for name in NC.FACE_CASES for dt in NC.DTYPES]


@pytest.mark.parametrize("name,dt", ALL)
def test_reference_matches_c_oracle(name, dt):
    """Two independent restatements (dense numpy, C double loop): equal pair sets, distances and deltas
    to 1e-12."""
    c = NC.get(name, dt)
    pairs, deltas, dist = NC.sort_edges(*NC.ref(name, dt))
    onb, odl, ods = O.neighbors(np.asarray(c.pos, dtype=np.float64), c.batch, c.lower, c.cutoff, loop=c.loop,
                                include_transpose=c.transpose, box=c.box, sq_compare=True)
    onb, odl, ods = NC.sort_edges(onb, odl, ods)
    assert np.array_equal(pairs, onb)
    assert np.abs(dist - ods).max() <= 1e-12
    assert np.abs(deltas - odl).max() <= 1e-12


@pytest.mark.parametrize("name,dt", ALL)
def test_no_pair_near_a_cutoff(name, dt):
    c = NC.get(name, dt)
    assert NC.margin_ok(c, NC.widened(c))
    assert NC.margin_ok(c, NC.ref(name, dt)[2])


@pytest.mark.parametrize("name,dt", ALL)
def test_cases_have_pairs_and_cross_boundary_pairs(name, dt):
    c = NC.get(name, dt)
    pairs, deltas, _ = NC.ref(name, dt)
    assert pairs.shape[1] >= 1 and len(c.strategies) >= 1
    assert np.array_equal(NC.row_ptr_of(pairs, len(c.pos))[-1:], [pairs.shape[1]])
    if c.box is not None and len(c.pos) > 1:  # a lone atom has no partner to wrap to
        p = np.asarray(c.pos, dtype=np.float64)
        shift = deltas - (p[pairs[0]] - p[pairs[1]])
        assert (np.abs(shift).max(axis=1) > 0.5 * min(c.lengths)).any()
    if name.startswith("scan_") and len(c.pos) > 1:  # a few pairs per atom, not a dense list
        assert 1 <= (pairs.shape[1] - len(c.pos)) / len(c.pos) <= 8


def _cells(c, fn):
    dt = NC.DTYPES[c.dtype]
    Ls = c.lengths if c.lengths is not None else (3 * c.cutoff,) * 3
    return [fn(c.pos[:, a], Ls[a], c.cutoff, dt) for a in range(3)], [NC.grid(L, c.cutoff) for L in Ls]


@pytest.mark.parametrize("name,dt", FACES)
def test_parent_cell_arithmetic_bins_face_atoms_at_minus_one(name, dt):
    """The parent's `cell_of`, restated at the case's dtype, gives cx = -1 for atoms of every face case:
    some with cy = cz = 0 (key -1: `k_cell_bounds` wrote cstart[-1]) and some with cy > 0 (a valid key
    naming the wrong cell).  So the parent fails these cases, and the generator still sits on the face."""
    c = NC.get(name, dt)
    (cx, cy, cz), (nx, ny, nz) = _cells(c, NC.cell_index_parent)
    assert ((cx == -1) & (cy == 0) & (cz == 0)).any()
    assert ((cx == -1) & (cy > 0)).any()
    assert (cx + nx * (cy + ny * cz)).min() < 0
    assert len(c.pos) % 4 == int(name[-1])  # n % 4 decides what the stray cstart[-1] / cend[-1] writes hit


@pytest.mark.parametrize("name,dt", ALL)
def test_fixed_cell_arithmetic_stays_in_range(name, dt):
    """`cell_axis` restated the same way: every atom of every case lands in [0, n) on every axis, and
    only the -1 atoms move (to the top cell)."""
    c = NC.get(name, dt)
    new, ns = _cells(c, NC.cell_index)
    old, _ = _cells(c, NC.cell_index_parent)
    for a in range(3):
        assert new[a].min() >= 0 and new[a].max() < ns[a]
        moved = new[a] != old[a]
        assert np.array_equal(moved, old[a] == -1)
        assert (new[a][moved] == ns[a] - 1).all()


def _cell_search_finds(c, pairs, fn):
    """Which reference pairs the 27-cell search reaches when atoms are binned by ``fn``: the source is
    filed under the cell its key decodes to (a negative key files it nowhere), the destination scans
    its own index - 1, 0, + 1 per axis, each wrapped once by the cell count as k_cell_pairs does."""
    (cx, cy, cz), (nx, ny, nz) = _cells(c, fn)
    key = cx + nx * (cy + ny * cz)
    filed = np.stack([key % nx, (key // nx) % ny, key // (nx * ny)])
    found = key[pairs[0]] >= 0
    for own, at, n in zip((cx, cy, cz), filed, (nx, ny, nz)):
        reach = own[pairs[1]][None, :] + np.array([-1, 0, 1])[:, None]
        reach = np.where(reach < 0, reach + n, np.where(reach >= n, reach - n, reach))
        found &= (reach == at[pairs[0]][None, :]).any(axis=0)
    return found


@pytest.mark.parametrize("name,dt", FACES)
def test_cell_search_over_fixed_bins_reaches_every_pair(name, dt):
    """The 27-cell search restated over the bins: with `cell_axis` every reference pair is reached; with
    the parent's arithmetic pairs are lost, and lost in one direction only (the list was asymmetric)."""
    c = NC.get(name, dt)
    pairs = NC.ref(name, dt)[0]
    assert _cell_search_finds(c, pairs, NC.cell_index).all()
    lost = ~_cell_search_finds(c, pairs, NC.cell_index_parent)
    assert lost.any()
    n = len(c.pos)
    lost_keys = set((pairs[0][lost] * n + pairs[1][lost]).tolist())
    assert any(int(t) * n + int(s) not in lost_keys for s, t in pairs[:, lost].T if s != t)


def test_fixed_cell_arithmetic_survives_any_value():
    for dt in NC.DTYPES.values():
        x = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 7.4999995, -7.5, 7.5, 0.0], dtype=dt)
        with np.errstate(invalid="ignore", over="ignore"):
            c = NC.cell_index(x, 15.0, 5.0, dt)
        assert c.min() >= 0 and c.max() < 3


@pytest.mark.parametrize("dt", list(NC.DTYPES))
def test_probes_sit_on_every_boundary(dt):
    """The generator really places atoms at each face, cell boundary and fold, one ulp either side and at
    each image (the values the issue lists), in the case's dtype."""
    t = NC.DTYPES[dt]
    for boxname, rem in (("b31", 0), ("b12", 1)):
        c = NC.get(f"face_{boxname}_n{rem}", dt)
        assert c.pos.dtype == t
        for a, L in enumerate(c.lengths):
            centres = NC.probe_centres(L, c.cutoff)
            assert {-L / 2, 0.0, L / 2, int(L / c.cutoff) * c.cutoff - L / 2} <= set(centres)
            have = set(c.pos[:, a].tolist())
            for ctr in centres:
                for k in NC.SHIFTS:
                    v = t(ctr + k * L)
                    assert float(v) == ctr + k * L  # the centres are exact in both dtypes
                    for x in (np.nextafter(v, t(-np.inf)), v, np.nextafter(v, t(np.inf))):
                        assert float(x) in have
    assert NC.probe_centres(31.0, 5.0) == [-15.5, -10.5, -5.5, -0.5, 0.0, 4.5, 9.5, 14.5, 15.5]
    assert NC.probe_centres(17.5, 5.0) == [-8.75, -3.75, 0.0, 1.25, 6.25, 8.75]


def test_row_limit_cases_have_the_stated_shapes():
    seg = NC.get("rows_segments", "f32")
    assert np.bincount(seg.batch).tolist() == [63, 64, 65, 129, 1]
    mid = NC.get("rows_descent_mid", "f32")
    assert len(mid.pos) == 600 and np.flatnonzero(np.diff(mid.batch) < 0).tolist() == [255]
    last = NC.get("rows_descent_last", "f64")
    assert np.flatnonzero(np.diff(last.batch) < 0).tolist() == [len(last.pos) - 2]
    assert not NC.get("rows_half", "f32").transpose
    low = NC.get("rows_lower_loop", "f32")
    pairs, _, dist = NC.ref("rows_lower_loop", "f32")
    assert low.lower == 2.0 and low.loop and (pairs[0] == pairs[1]).sum() == len(low.pos)
    assert dist[pairs[0] != pairs[1]].min() >= 2.0
    assert [len(NC.get(n, "f32").pos) for n in NC.names("scan_")] == [1, 1023, 1024, 1025, 2049]
    assert (np.diff(NC.get("grid_mols_shuffled", "f32").batch) < 0).any()
    assert not (np.diff(NC.get("grid_mols_sorted", "f32").batch) < 0).any()


def test_reference_hand_checked():
    """Three atoms on a line in a 10-box: a wrapped pair, an unwrapped one, the lower cutoff, the self
    pairs and the half list, against values worked by hand."""
    pos = np.array([[4.5, 0, 0], [-4.5, 0, 0], [-2.0, 0, 0]])
    box = np.diag([10.0, 10.0, 10.0])
    pairs, deltas, dist = NC.reference(pos, np.zeros(3, dtype=np.int64), box, 0.0, 3.0, loop=False)
    assert pairs.T.tolist() == [[1, 0], [0, 1], [2, 1], [1, 2]]
    assert np.allclose(deltas[:, 0], [1.0, -1.0, 2.5, -2.5], atol=1e-15) and np.allclose(dist, [1, 1, 2.5, 2.5])
    pairs, _, _ = NC.reference(pos, np.zeros(3, dtype=np.int64), box, 2.0, 3.0, loop=True, include_transpose=False)
    assert pairs.T.tolist() == [[0, 0], [1, 1], [2, 1], [2, 2]]
    pairs, _, _ = NC.reference(pos, np.array([0, 1, 1]), None, 0.0, 3.0, loop=False)
    assert pairs.T.tolist() == [[2, 1], [1, 2]]
    assert NC.row_ptr_of(pairs, 3).tolist() == [0, 0, 1, 2]
