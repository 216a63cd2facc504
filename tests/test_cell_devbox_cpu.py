"""The parts of the device-box cell build that need no GPU: the Python refusals of a 3-d box with the cell strategy
(raised before the native library is loaded), the box that ``validate_boxes`` brings back in its one read, and the
``cell_margin`` -> ``cell_bound`` arithmetic of ``GraphedEnergyForces``."""
import pytest
import torch

import neighbor_cases_tric as TC

CUT = 4.0


@pytest.fixture
def no_native(monkeypatch):
    """Any touch of the native library fails the test."""
    from torchmdnet import _native as nat

    def refuse(*a, **k):
        raise AssertionError("the native library was touched")

    monkeypatch.setattr(nat, "load", refuse)
    monkeypatch.setattr(nat, "require_gpu", refuse)


def _inputs():
    # positions "on a device" without one: the checks compare devices and shapes, they read no value
    pos = torch.empty(12, 3, device="meta")
    batch = torch.zeros(12, dtype=torch.long, device="meta")
    return pos, batch, torch.tensor(TC.box_of("t31"))


def test_refusals_touch_no_native_code(no_native):
    from torchmdnet import kernels
    pos, batch, box = _inputs()
    on_dev = box.reshape(1, 3, 3).to("meta")
    graph = lambda **kw: kernels.build_graph(pos, batch, 0.0, CUT, 512, strategy="cell", **kw)  # noqa: E731
    raw = lambda bx, **kw: kernels.neighbor_pairs_raw("cell", pos, batch, bx, True, 0.0, CUT, 512, True, True, **kw)  # noqa: E731
    # one box, but on the host
    with pytest.raises(RuntimeError, match="on the device"):
        graph(box=box.reshape(1, 3, 3))
    with pytest.raises(RuntimeError, match="on the device"):
        raw(box.reshape(1, 3, 3), cell_bound=box)
    # several boxes: as before
    two = on_dev.expand(2, 3, 3)
    with pytest.raises(RuntimeError, match="brute and shared"):
        graph(box=two)
    with pytest.raises(RuntimeError, match="brute and shared"):
        graph(box=two, static_capacity=512, cell_bound=box)
    with pytest.raises(RuntimeError, match="brute and shared"):
        raw(two, cell_bound=box)
    # static capacity: nothing may be read back, so the bound is required
    with pytest.raises(RuntimeError, match='needs "cell_bound"'):
        graph(box=on_dev, static_capacity=512)
    with pytest.raises(RuntimeError, match=r'"cell_bound" to have shape \(3, 3\)'):
        graph(box=on_dev, static_capacity=512, cell_bound=box.reshape(1, 3, 3))


def test_validate_boxes_reads_the_box_back():
    from torchmdnet import kernels
    box = torch.tensor(TC.box_of("t31")) * 1.0371
    assert kernels.validate_boxes(box.reshape(1, 3, 3), CUT) is None
    back = kernels.validate_boxes(box.reshape(1, 3, 3), CUT, read_back=True)
    assert back.dtype == torch.float64 and back.device.type == "cpu" and torch.equal(back, box)
    back = kernels.validate_boxes(box.float().reshape(1, 3, 3), CUT, torch.tensor([0, 0]), read_back=True)
    assert torch.equal(back, box.float().double())
    short = box.clone()
    short[2, 2] = 7.5
    with pytest.raises(RuntimeError, match=r"^molecule 0: Invalid box vectors: box_vectors\[2\]\[2\] < 2\*cutoff$"):
        kernels.validate_boxes(short.reshape(1, 3, 3), CUT, read_back=True)
    with pytest.raises(RuntimeError, match="1 boxes.*molecule 1"):
        kernels.validate_boxes(box.reshape(1, 3, 3), CUT, torch.tensor([0, 1]), read_back=True)


def test_cell_margin_scales_every_lattice_vector():
    from torchmdnet.graphs import GraphedEnergyForces, cell_bound_of
    from torchmdnet.models.utils import OptimizedDistance
    box = torch.tensor(TC.box_of("t31"))
    for form in (box, box.reshape(1, 3, 3), box.float()):
        b = cell_bound_of(form, 1.25)
        assert b.shape == (3, 3) and b.dtype == torch.float64 and b.device.type == "cpu"
        assert torch.equal(b, box * 1.25)
    # the bound's grid has room for the cell scaled by anything up to the margin
    assert all(g >= h for g, h in zip(TC.grid(cell_bound_of(box, 1.25).numpy(), CUT),
                                      TC.grid(TC.box_of("t31") * 1.2, CUT)))
    assert torch.equal(cell_bound_of(box, 1.0), box)
    import inspect
    assert inspect.signature(GraphedEnergyForces.__init__).parameters["cell_margin"].default == 1.25
    d = OptimizedDistance(0.0, CUT, max_num_pairs=64, strategy="cell", box=box)
    assert d.cell_bound is None

    # release() on a stub: the bound goes with the static capacity
    class Stub:
        pass
    gm, dist = Stub(), Stub()
    dist.static_capacity, dist.cell_bound = 512, cell_bound_of(box, 1.25)
    gm.dists, gm.cell_dists, gm.priors = [dist], [dist], []
    GraphedEnergyForces.release(gm)
    assert dist.cell_bound is None and dist.static_capacity is None
