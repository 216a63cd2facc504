"""CPU checks of the per-molecule-box yardstick (tests/batch_box_ref.py) and of the pieces of the feature that
need no GPU: the yardstick against ``neighbor_cases.reference`` where they must agree, the input condition the
GPU tests rely on, the batched box validation and ``stress_from_virial``."""
import numpy as np
import pytest
import torch

import batch_box_ref as BB
import neighbor_cases as NC


@pytest.mark.parametrize("dt", list(NC.DTYPES))
def test_equal_boxes_are_the_single_box_reference(dt):
    """A batch whose boxes are all the same box: the per-molecule yardstick is ``neighbor_cases.reference`` with
    that one box (which already keeps pairs inside a molecule), list for list."""
    c = BB.get("main", dt)
    for box in (BB.BOXES[2], BB.BOXES[0]):
        boxes = np.repeat(box[None], len(c.sizes), axis=0)
        for loop, tr in ((True, True), (False, True), (True, False), (False, False)):
            got = BB.reference(c.pos, c.batch, boxes, 0.0, c.cutoff, loop, tr)
            p, d, r = NC.reference(c.pos, c.batch, box, 0.0, c.cutoff, loop, tr)
            ref = NC.sort_edges(p, d, r)
            assert got[0].shape[1] > 300
            assert np.array_equal(got[0], ref[0])
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("dt", list(NC.DTYPES))
@pytest.mark.parametrize("name", ["main", "interleaved"])
def test_inputs_keep_the_margin_and_probe_the_images(name, dt):
    """The input condition of the GPU tests: no pair distance within MARGIN * cutoff of the cutoff (fp64
    reference on the values the GPU sees); the boxes are valid reduced forms, the triclinic one with all three
    skew entries; a third of the atoms sit in other images; every box wraps some pair, the list differs from a
    one-box list, and molecule 0's 70 candidates reach into a second 64-lane iteration that finds pairs."""
    c = BB.get(name, dt)
    assert BB.margin_ok(c)
    for b in c.boxes:
        assert b[0, 1] == b[0, 2] == b[1, 2] == 0
        assert min(b[0, 0], b[1, 1], b[2, 2]) >= 2 * c.cutoff
        assert b[0, 0] >= 2 * abs(b[1, 0]) and b[0, 0] >= 2 * abs(b[2, 0]) and b[1, 1] >= 2 * abs(b[2, 1])
    assert all(BB.BOXES[2][i, j] != 0 for i, j in ((1, 0), (2, 0), (2, 1)))
    pairs, deltas, _ = BB.ref(name, dt)
    raw = c.pos[pairs[0]].astype(np.float64) - c.pos[pairs[1]]
    moved = np.abs(deltas - raw).max(axis=1) > 1.0
    for m in range(len(c.sizes)):
        if c.sizes[m] > 1:
            assert moved[c.batch[pairs[1]] == m].any(), m
    frac = np.stack([np.linalg.solve(c.boxes[m].T, p) for p, m in zip(c.pos.astype(np.float64), c.batch)])
    outside = ((frac < 0.45) | (frac > 1.55)).any(axis=1)  # the unmoved atoms lie in [0.5, 1.5]
    assert 0.2 * len(c.pos) < outside.sum() < 0.45 * len(c.pos)
    one = NC.sort_edges(*NC.reference(c.pos, c.batch, c.boxes[0], 0.0, c.cutoff))[0]
    assert one.shape != pairs.shape or not np.array_equal(one, pairs)
    if name == "main":
        assert c.sizes == (70, 33, 1, 65) and c.cutoff == 3.0
        assert np.array_equal(c.batch, np.repeat(np.arange(4), c.sizes))
        # molecule 0's candidates span two 64-lane iterations, and its second iteration finds pairs
        assert ((pairs[1] < 70) & (pairs[0] >= 64)).any()
    else:
        assert (np.diff(c.batch) < 0).sum() >= 30


def test_validate_boxes_names_the_first_offender():
    from torchmdnet import kernels
    boxes = torch.tensor(BB.BOXES)
    kernels.validate_boxes(boxes, BB.CUTOFF)
    kernels.validate_boxes(boxes, BB.CUTOFF, torch.tensor([0, 0, 1, 3]))
    bad = boxes.clone()
    bad[2, 0, 0] = 5.0
    bad[3, 0, 1] = 0.1
    with pytest.raises(RuntimeError, match=r"^molecule 2: Invalid box vectors: box_vectors\[0\]\[0\] < 2\*cutoff$"):
        kernels.validate_boxes(bad, BB.CUTOFF)
    for m in range(4):  # the message is validate_box's for that box
        bad = boxes.clone()
        bad[m, 2, 1] = 0.75 * float(bad[m, 1, 1])
        with pytest.raises(RuntimeError) as one:
            kernels.validate_box(bad[m], BB.CUTOFF)
        with pytest.raises(RuntimeError) as many:
            kernels.validate_boxes(bad, BB.CUTOFF)
        assert str(many.value) == f"molecule {m}: " + str(one.value)
    with pytest.raises(RuntimeError, match="4 boxes.*molecule 4"):
        kernels.validate_boxes(boxes, BB.CUTOFF, torch.tensor([0, 4, 1]))
    with pytest.raises(RuntimeError, match="shape"):
        kernels.validate_boxes(boxes[0], BB.CUTOFF)
    with pytest.raises(RuntimeError, match=r"shape \(3, 3\)"):  # the (3, 3) form is as it was
        kernels.validate_box(boxes, BB.CUTOFF)


@pytest.mark.parametrize("model", ["equivariant-transformer", "tensornet"])
def test_scripted_forward_refuses_a_box(model):
    """The models still script with the new argument; a scripted forward given a box raises RuntimeError inside the
    interpreter (it reaches Python as torch.jit.Error naming it) before anything else runs."""
    from conftest import yaml_args
    from torchmdnet import _native
    from torchmdnet.models.model import create_model
    _native.load_torch_ops()
    m = create_model(yaml_args(model, embedding_dimension=32, num_layers=1, derivative=True))
    s = torch.jit.script(m)
    z, pos, batch = torch.tensor([8, 1, 1]), torch.randn(3, 3), torch.zeros(3, dtype=torch.long)
    with pytest.raises((RuntimeError, torch.jit.Error), match="RuntimeError: .*per-call box runs eagerly"):
        s(z, pos, batch, box=torch.tensor(BB.BOXES[:1]))


def test_stress_from_virial():
    from torchmdnet.utils import stress_from_virial
    g = torch.Generator().manual_seed(0)
    w = torch.randn(4, 3, 3, generator=g, dtype=torch.float64)
    boxes = torch.tensor(BB.BOXES)
    s = stress_from_virial(w, boxes)
    for m in range(4):
        assert torch.allclose(s[m], -w[m] / torch.linalg.det(boxes[m]), rtol=1e-14, atol=0)
    assert torch.allclose(stress_from_virial(w, boxes[2]), -w / torch.linalg.det(boxes[2]), rtol=1e-14, atol=0)
    assert torch.allclose(-s * torch.linalg.det(boxes).reshape(4, 1, 1), w, rtol=1e-14, atol=0)
