"""Open molecules among per-molecule boxes, and the periodic pair priors' yardstick, without a GPU:
``kernels.validate_boxes`` with an all-zero box, the fixture of tests/open_mol_ref.py, the prior constructors'
``periodic`` contract, and tests/periodic_prior_ref.py against the reference's recorded run
(tests/golden/priors_ref.npz) in a box far larger than the molecules."""
import numpy as np
import pytest
import torch

import open_mol_ref as OM
import pair_prior_ref as R
import periodic_prior_ref as PR
from conftest import golden
from torchmdnet import kernels
from torchmdnet.priors import D2, ZBL, Coulomb

SCALES = dict(distance_scale=1e-10, energy_scale=4.35974e-18)
NUMBERS = list(range(100))


# ----------------------------------------------------------------------------- validate_boxes
def test_validate_boxes_passes_an_open_molecule():
    boxes = torch.tensor(OM.BOXES)
    assert OM.is_open(OM.BOXES[OM.OPEN])
    kernels.validate_boxes(boxes, OM.CUTOFF)
    kernels.validate_boxes(boxes, OM.CUTOFF, torch.tensor([0, 1, 1, 2, 3]))
    kernels.validate_boxes(boxes.float(), OM.CUTOFF)
    kernels.validate_boxes(torch.zeros(3, 3, 3, dtype=torch.float64), OM.CUTOFF)  # every molecule open
    # the read-back still brings the first box
    back = kernels.validate_boxes(boxes, OM.CUTOFF, read_back=True)
    assert torch.equal(back, boxes[0])


def test_validate_boxes_names_a_partly_zero_box_as_before():
    boxes = torch.tensor(OM.BOXES)
    for (i, j), msg in (((0, 0), r"box_vectors\[0\]\[0\] < 2\*cutoff"), ((1, 1), r"box_vectors\[1\]\[1\] < 2\*cutoff"),
                        ((2, 2), r"box_vectors\[2\]\[2\] < 2\*cutoff")):
        bad = boxes.clone()
        bad[OM.OPEN] = torch.tensor(OM.BOXES[0])
        bad[OM.OPEN, i, j] = 0.0  # one length missing
        with pytest.raises(RuntimeError, match=r"molecule 1: Invalid box vectors: " + msg):
            kernels.validate_boxes(bad, OM.CUTOFF)
    bad = boxes.clone()
    bad[OM.OPEN, 0, 1] = 1e-300  # the smallest entry off the reduced form: not an open molecule
    with pytest.raises(RuntimeError, match=r"molecule 1: Invalid box vectors: box_vectors\[0\]\[1\] != 0"):
        kernels.validate_boxes(bad, OM.CUTOFF)
    bad = boxes.clone()
    bad[OM.OPEN, 2, 0] = 0.5  # a lone skew entry
    with pytest.raises(RuntimeError, match=r"molecule 1: Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"):
        kernels.validate_boxes(bad, OM.CUTOFF)
    # a short box beside the open molecule is still named, by its own index
    bad = boxes.clone()
    bad[2, 1, 1] = 5.9
    with pytest.raises(RuntimeError, match=r"molecule 2: Invalid box vectors: box_vectors\[1\]\[1\] < 2\*cutoff"):
        kernels.validate_boxes(bad, OM.CUTOFF)


def test_a_lone_zero_box_is_still_refused():
    with pytest.raises(RuntimeError, match=r"molecule 0: Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"):
        kernels.validate_boxes(torch.zeros(1, 3, 3, dtype=torch.float64), OM.CUTOFF)
    with pytest.raises(RuntimeError, match=r"Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff"):
        kernels.validate_box(torch.zeros(3, 3, dtype=torch.float64), OM.CUTOFF)


# ----------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_fixture_has_what_the_gpu_tests_rely_on(dt):
    c = OM.get(dt)
    OM.check_fixture(c)
    assert OM.margin_ok(c) and OM.margin_ok(OM.get(dt, True))
    assert c.sizes == (70, 9, 33, 1) and len(c.pos) == 113
    # the shuffled batch is the same molecules: the same number of pairs
    assert OM.ref(dt, True)[0].shape == OM.ref(dt)[0].shape
    # the open molecule's rows are the non-periodic list's: deltas are plain differences
    p, d, _ = OM.ref(dt, False, False, True)
    rows = c.batch[p[1]] == OM.OPEN
    assert rows.any()
    pos = np.asarray(c.pos, dtype=np.float64)
    assert np.array_equal(d[rows], pos[p[0][rows]] - pos[p[1][rows]])


# ----------------------------------------------------------------------------- prior constructors
def test_periodic_is_opt_in_and_reported_only_when_set():
    zbl = ZBL(3.0, 40, atomic_number=NUMBERS, **SCALES)
    d2 = D2(3.0, 64, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
    for p in (zbl, d2):
        assert p.periodic is False and p.neighbor_strategy == "brute" and p.cell_bound is None
        assert "periodic" not in p.get_init_args() and "neighbor_strategy" not in p.get_init_args()
    zp = ZBL(3.0, 40, atomic_number=NUMBERS, periodic=True, **SCALES)
    assert zp.periodic is True and zp.get_init_args()["periodic"] is True
    assert "neighbor_strategy" not in zp.get_init_args()
    dp = D2(3.0, 64, atomic_number=NUMBERS, periodic=True, neighbor_strategy="cell", **SCALES)
    args = dp.get_init_args()
    assert args["periodic"] is True and args["neighbor_strategy"] == "cell"
    again = D2(**args)
    assert again.periodic and again.neighbor_strategy == "cell" and again.get_init_args() == args
    assert set(zp.state_dict()) == set(zbl.state_dict())
    with pytest.raises(ValueError, match="neighbor_strategy"):
        ZBL(3.0, 40, atomic_number=NUMBERS, neighbor_strategy="tree", **SCALES)


def test_coulomb_refuses_periodic():
    with pytest.raises(ValueError, match="infinite cutoff"):
        Coulomb(0.3, 40, periodic=True, **SCALES)
    assert Coulomb(0.3, 40, periodic=False, **SCALES).periodic is False
    # the strategy of a periodic list means nothing to it either: refused, not stored and lost on reload
    with pytest.raises(ValueError, match="neighbor_strategy.*infinite cutoff"):
        Coulomb(0.3, 40, neighbor_strategy="cell", **SCALES)
    assert Coulomb(0.3, 40, neighbor_strategy="brute", **SCALES).neighbor_strategy == "brute"


def test_periodic_prior_from_a_yaml_entry():
    from torchmdnet.models.model import create_prior_models
    from conftest import yaml_args
    args = yaml_args("equivariant-transformer")
    args["prior_model"] = [{"ZBL": dict(cutoff_distance=3.0, max_num_neighbors=40, atomic_number=NUMBERS,
                                        periodic=True, **SCALES)}]
    prior, = create_prior_models(args)
    assert isinstance(prior, ZBL) and prior.periodic


# ----------------------------------------------------------------------------- the restatement
def _golden_inputs():
    d = golden("priors_ref.npz")
    return d, torch.tensor(d["z"]), torch.tensor(d["pos"]), torch.tensor(d["batch"])


def _energy(kind, z, batch, n_mol, boxes, zbl=PR.zbl_energy, cutoff=None):
    if kind == "zbl":
        return lambda p: zbl(p, z, batch, n_mol, cutoff or 5.0, NUMBERS, boxes=boxes, **SCALES)
    t = D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
    return lambda p: PR.d2_energy(p, z, batch, n_mol, cutoff or 10.0, NUMBERS, c6=t.C_6, r_r=t.R_r, boxes=boxes,
                                  **SCALES)


def _far_boxes(pos, batch, n_mol):
    """Per-molecule boxes (the first skewed, the last open) far larger than the molecules: the imaged pairs are the
    molecules' own."""
    L = 50.0 * float(pos.abs().max())
    boxes = torch.eye(3, dtype=torch.float64).repeat(n_mol, 1, 1) * L
    boxes[0, 1, 0], boxes[0, 2, 0], boxes[0, 2, 1] = 0.3 * L, -0.2 * L, 0.25 * L
    boxes[n_mol - 1] = 0.0
    return boxes


@pytest.mark.parametrize("kind", ["zbl", "d2"])
def test_restatement_in_a_large_box_reproduces_the_reference_run(kind):
    """The reference's own float64 outputs, to 1e-12 of the largest entry, from the periodic restatement in boxes far
    larger than the molecules -- one box for all, and per-molecule boxes with a skewed and an open one.  ZBL is
    compared with the screening length rounded as the reference rounds it (float32; the package and
    pair_prior_ref.zbl_energy keep float64 there, 2e-8 away: tests/test_pair_priors_cpu.py), and that form is tied
    to ``zbl_energy`` by the non-periodic comparison below."""
    d, z, pos, batch = _golden_inputs()
    n_mol = int(batch.max()) + 1
    one = torch.eye(3, dtype=torch.float64) * 50.0 * float(pos.abs().max())
    zbl = PR.zbl_energy_reference_rounding
    for boxes in (one, _far_boxes(pos, batch, n_mol)):
        y, f, h = R.energy_forces_second(_energy(kind, z, batch, n_mol, boxes, zbl=zbl), pos)
        for name, got, ref in (("y", y.reshape(-1), d[kind + "/y"].reshape(-1)), ("forces", f, d[kind + "/forces"]),
                               ("dF2", h, d[kind + "/dF2"])):
            ref = torch.tensor(ref)
            err = float((got - ref).abs().max() / ref.abs().max())
            print(f"{kind} {name}: max|d|/max|ref| = {err:.3e}")
            assert err <= 1e-12, (kind, name, err)


@pytest.mark.parametrize("kind", ["zbl", "d2"])
def test_restatement_in_a_large_box_is_the_non_periodic_one(kind):
    """Same formulas, same pairs: the periodic restatement in large boxes against pair_prior_ref's own functions,
    with atoms of the boxed molecules moved into other images (the shift is exact in none of them, so the bound is
    rounding of the deltas at 50 times the coordinates: 1e-12)."""
    d, z, pos, batch = _golden_inputs()
    n_mol = int(batch.max()) + 1
    boxes = _far_boxes(pos, batch, n_mol)
    moved = pos.clone()
    k = (torch.arange(len(pos)) % 3 == 0) & (batch < n_mol - 1)
    moved[k] += torch.einsum("j,njk->nk", torch.tensor([1.0, -1.0, 3.0], dtype=torch.float64), boxes[batch[k]])
    plain = {"zbl": lambda p: R.zbl_energy(p, z, batch, n_mol, 5.0, NUMBERS, **SCALES)}
    if kind == "d2":
        t = D2(10.0, 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
        plain["d2"] = lambda p: R.d2_energy(p, z, batch, n_mol, 10.0, NUMBERS, c6=t.C_6, r_r=t.R_r, **SCALES)
    ref = R.energy_forces_second(plain[kind], pos)
    got = R.energy_forces_second(_energy(kind, z, batch, n_mol, boxes), moved)
    for name, a, b in zip(("y", "forces", "dF2"), got, ref):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{kind} {name}: max|d|/max|ref| = {err:.3e}")
        assert err <= 1e-12, (kind, name, err)
    # and the reference-rounded ZBL differs from it by the float32 rounding of the screening length only
    if kind == "zbl":
        y32 = PR.zbl_energy_reference_rounding(pos, z, batch, n_mol, 5.0, NUMBERS, boxes=boxes, **SCALES)
        assert 0 < float((y32 - ref[0]).abs().max() / ref[0].abs().max()) < 1e-6


def test_restatement_images_pairs_and_its_virial_is_the_strain_derivative():
    """On the open-molecule batch: the periodic energy differs from the non-periodic one for the boxed molecules
    and equals it for the open one and the single atom; the virial of ``PR.virial`` is a central difference of the
    energy under pos -> pos (I + eps)^T, box -> box (I + eps)^T (h = 1e-5, 1e-8 of the largest entry:
    tests/test_virial_cpu.py), and the open molecule's is sum F (x) pos."""
    c = OM.get("f64")
    pos, batch, z = torch.tensor(c.pos), torch.tensor(c.batch), torch.tensor(c.z)
    boxes = torch.tensor(c.boxes)
    e = lambda p, bx, eps=None: PR.zbl_energy(p, z, batch, 4, 3.0, NUMBERS, boxes=bx, eps=eps, **SCALES)
    y_box, y_open = e(pos, boxes), e(pos, None)
    assert y_box[1] == y_open[1] and y_box[3] == 0 and y_open[3] == 0
    assert y_box[0] != y_open[0] and y_box[2] != y_open[2]
    p = pos.clone().requires_grad_(True)
    W = PR.virial(lambda q, eps: e(q, boxes, eps), p).detach()
    f, = torch.autograd.grad(-e(p, boxes).sum(), p)
    idx = batch == OM.OPEN
    assert torch.allclose(W[OM.OPEN], f[idx].T @ pos[idx], rtol=1e-12, atol=1e-12 * float(W.abs().max()))
    assert float(W[3].abs().max()) == 0
    h = 1e-5
    m = 2  # the triclinic molecule.  Only the strains that keep the box in the reduced (lower-triangular) form the
    # image is defined for: eps_ab with a <= b (the virial of a pair potential is symmetric)
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        ys = []
        for sgn in (1.0, -1.0):
            s = torch.eye(3, dtype=torch.float64)
            s[a, b] += sgn * h
            ys.append(e(pos @ s.T, boxes @ s.T)[m])
        fd = float(ys[0] - ys[1]) / (2 * h)
        assert abs(fd + float(W[m, a, b])) <= 1e-8 * float(W[m].abs().max()), (a, b)
