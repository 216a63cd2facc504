"""CPU checks of tests/neighbor_cases_tric.py and of kernels.wrap_into_box: the conditions the GPU tests
of the triclinic cell list rely on (no pair near a cutoff, the grid of each box), the coverage argument of
the 27-cell search stated on the real inputs through the restated binning, and the box wrap."""
import numpy as np
import pytest
import torch

import neighbor_cases as NC
import neighbor_cases_tric as TC

ALL = [(name, dt) for name in TC.CASES for dt in TC.DTYPES]


@pytest.mark.parametrize("name,dt", ALL)
def test_no_pair_near_a_cutoff(name, dt):
    c = TC.get(name, dt)
    assert NC.margin_ok(c, NC.widened(c))
    assert NC.margin_ok(c, TC.ref(name, dt)[2])


def test_grid_matches_the_table():
    want_w = {"t15": (14.47, 14.49, 15.0), "t31": (27.79, 21.76, 17.5), "tmax": (20.95, 21.47, 24.0),
              "tneg": (20.95, 21.47, 24.0)}
    for name, (rows, cut, ns) in TC.BOXES.items():
        box = TC.box_of(name)
        assert TC.grid(box, cut) == ns
        assert np.allclose(TC.widths(box), want_w[name], atol=0.006)
        # the widths against their definition: the box volume over the area of each face
        a, b, c = box
        vol = abs(np.dot(a, np.cross(b, c)))
        areas = [np.linalg.norm(np.cross(b, c)), np.linalg.norm(np.cross(c, a)), np.linalg.norm(np.cross(a, b))]
        assert np.allclose(TC.widths(box), [vol / s for s in areas], rtol=1e-14)
        # neither computed width sits at a multiple of the cutoff, where floor() would hang on a rounding
        # (w_c = c2 is not computed: 15 / 5 and 24 / 3 are exact)
        assert all(abs(w / cut - round(w / cut)) > 1e-3 for w in TC.widths(box)[:2])
    assert TC.grid(np.diag([15.0, 23.0, 17.5]), 5.0) == (3, 4, 3)  # a diagonal box: the rule on lengths


@pytest.mark.parametrize("name,dt", ALL)
def test_cases_have_pairs_and_cross_boundary_pairs(name, dt):
    c = TC.get(name, dt)
    pairs, deltas, _ = TC.ref(name, dt)
    assert pairs.shape[1] >= 1 and c.strategies[0] == "cell"
    if len(c.pos) > 1:
        p = np.asarray(c.pos, dtype=np.float64)
        k = np.rint((deltas - (p[pairs[0]] - p[pairs[1]])) @ np.linalg.inv(c.box))  # lattice shift of each pair
        assert (k != 0).all(axis=1).any()  # some image moves along a, b and c at once
    if name == "grid_n2":
        assert pairs.T.tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
        assert sorted(np.abs(k[1]).tolist()) == [1, 1, 1]


@pytest.mark.parametrize("name,dt", ALL)
def test_restated_bins_stay_in_range(name, dt):
    c = TC.get(name, dt)
    idx, ns = TC.cells(c.pos, c.box, c.cutoff, TC.DTYPES[dt])
    assert ns == TC.BOXES[c.boxname][2]
    for i, n in zip(idx, ns):
        assert i.min() >= 0 and i.max() < n


@pytest.mark.parametrize("name,dt", ALL)
def test_every_reference_pair_lies_in_adjacent_cells(name, dt):
    """The coverage argument on the real inputs, ulp probes included: for every reference pair, the
    restated cell indices of source and destination differ by at most one (mod n) on every axis with
    n >= 4 (an axis with n = 3 is scanned whole)."""
    c = TC.get(name, dt)
    pairs = TC.ref(name, dt)[0]
    idx, ns = TC.cells(c.pos, c.box, c.cutoff, TC.DTYPES[dt])
    for i, n in zip(idx, ns):
        if n >= 4:
            d = (i[pairs[0]] - i[pairs[1]]) % n
            assert np.isin(d, (0, 1, n - 1)).all()


@pytest.mark.parametrize("dt", list(TC.DTYPES))
def test_probes_sit_on_every_cell_face(dt):
    """The face cases hold atoms in the cell below and in the cell above every cell boundary and box face
    of every lattice axis (the ulp neighbours fall on both sides), at every image."""
    t = TC.DTYPES[dt]
    for name in TC.FACE_CASES:
        c = TC.get(name, dt)
        assert c.pos.dtype == t and c.strategies == NC.ALL3
        idx, ns = TC.cells(c.pos, c.box, c.cutoff, t)
        nprobe = 15 * sum(n + 1 for n in ns)
        assert len(c.pos) == nprobe + 100
        at = 0
        for ax, n in enumerate(ns):
            for k in range(n + 1):
                got = set(idx[ax][at:at + 15].tolist())
                assert got == {(k - 1) % n, k % n}, (name, ax, k, got)
                at += 15


def test_binning_survives_any_value():
    for t in TC.DTYPES.values():
        x = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, -1e-30, 1.0, -1.0, 0.0, 0.99999994], dtype=t)
        with np.errstate(invalid="ignore", over="ignore"):
            for n in (3, 6, 1024):
                i = TC.cell_frac(x, n, t)
                assert i.min() >= 0 and i.max() < n
        assert TC.cell_frac(np.array([-1e-30], dtype=t), 6, t)[0] == 0  # s - floor(s) rounds to 1: cell 0


# ----------------------------------------------------------------------------- kernels.wrap_into_box
def _positions(box, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    frac = (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 7.0  # +-3.5 boxes
    return (frac @ torch.tensor(box)).to(dtype)


@pytest.mark.parametrize("boxname", list(TC.BOXES))
def test_wrap_into_box_moves_by_lattice_vectors_into_the_cell(boxname):
    from torchmdnet import kernels
    box = TC.box_of(boxname)
    pos = _positions(box, 500, torch.float64, 3)
    out = kernels.wrap_into_box(pos, torch.tensor(box))
    assert out.shape == pos.shape and out.dtype == pos.dtype
    k = (out - pos).numpy() @ np.linalg.inv(box)
    assert np.abs(k - np.rint(k)).max() < 1e-9 and np.abs(np.rint(k)).max() >= 3
    assert np.abs((out - pos).numpy() - np.rint(k) @ box).max() < 1e-9
    frac = out.numpy() @ np.linalg.inv(box)
    assert frac.min() >= 0.0 and frac.max() < 1.0
    # fp32 positions, the box given in fp32: inside the cell to the rounding of the coordinates
    out32 = kernels.wrap_into_box(pos.float(), torch.tensor(box, dtype=torch.float32))
    assert out32.dtype == torch.float32
    frac32 = out32.double().numpy() @ np.linalg.inv(box)
    assert frac32.min() > -1e-5 and frac32.max() < 1.0 + 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_wrap_into_box_diagonal_is_remainder(dtype):
    from torchmdnet import kernels
    Ls = (15.0, 23.0, 17.5)
    box = torch.diag(torch.tensor(Ls, dtype=dtype))
    pos = _positions(np.diag(Ls), 500, dtype, 4)
    out = kernels.wrap_into_box(pos, box)
    want = torch.stack([torch.remainder(pos[:, i], Ls[i]) for i in range(3)], dim=1)
    assert torch.equal(out, want)


def test_spatial_permutation_unchanged_for_a_diagonal_box():
    """The Morton renumbering with a diagonal box, against the parent's statement written out."""
    from torchmdnet import kernels
    Ls = (15.0, 23.0, 17.5)
    box = torch.diag(torch.tensor(Ls))
    pos = _positions(np.diag(Ls), 700, torch.float32, 5)
    batch = torch.repeat_interleave(torch.arange(2), 350)
    p = torch.stack([torch.remainder(pos[:, i], Ls[i]) for i in range(3)], dim=1)
    c = torch.clamp(((p - p.min(dim=0).values) / 5.0).long(), 0, 1023)
    key = kernels._spread10(c[:, 0]) | (kernels._spread10(c[:, 1]) << 1) | (kernels._spread10(c[:, 2]) << 2)
    want = torch.argsort(key + batch * (1 << 31), stable=True)
    assert torch.equal(kernels.spatial_permutation(pos, batch, 5.0, box), want)
    # a triclinic box: still a permutation, molecule-major
    perm = kernels.spatial_permutation(pos, batch, 4.0, torch.tensor(TC.box_of("t31")))
    assert torch.equal(torch.sort(perm).values, torch.arange(700)) and (torch.diff(batch[perm]) >= 0).all()
