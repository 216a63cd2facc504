"""The device pair-row count of a static-capacity graph (``EdgeGraph.num_pair_rows_dev``) and the captured ET
evaluation that stops its dk/dv projection there (et_stack: ``proj_act(..., rows=)``).

The count: written by the neighbour build's row scan (``tmdnet_nl_build``'s ``num_pair_rows``) or by the pair numbering's
scan (``tmdnet_pair_index``'s); both must leave the number of pairs numbered over the KEPT list -- the number
of distinct ``pair_row`` values of the live edges, every one of them below it -- clamped to the slot count, with
head room in the capacity and with a capacity that truncates the list.

The model: a captured step whose projection skips the padding rows must give what the eager model gives (the
tolerance test_gpu_capture.py uses for captured against eager), and the same BITS whatever the capacity is: the
live rows do not depend on it.
"""
import numpy as np
import pytest
import torch

import neighbor_cases as NC
from conftest import yaml_args

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- the count
def _build(c, loop, cap, pairs):
    from torchmdnet import kernels
    pos = torch.from_numpy(np.array(c.pos)).to(DEV)
    batch = torch.from_numpy(np.array(c.batch)).to(DEV)
    box = None if c.box is None else torch.from_numpy(c.box)
    return kernels.build_graph(pos, batch, c.lower, c.cutoff, 1 << 20, loop=loop, strategy="brute", box=box,
                               static_capacity=cap, pairs=pairs)


@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
@pytest.mark.parametrize("name", ["rows_segments", "rows_descent_last", "scan_1025"])
def test_pair_row_count(name, loop):
    from torchmdnet import kernels
    c = NC.get(name, "f32")
    n = c.pos.shape[0]
    E = int(_build(c, loop, None, False).num_pairs)
    assert E > n
    for cap in (int(np.ceil(1.25 * E / 256) * 256), (3 * E) // 5):  # head room; a truncated list
        fused = _build(c, loop, cap, True)
        lazy = _build(c, loop, cap, False)
        assert lazy.num_pair_rows_dev is None
        pr_l, pe_l = kernels.pair_index(lazy)  # the closed-form passes over sorted rows
        n_sorted = int(lazy.num_pair_rows_dev.item())
        lazy._pairs, lazy.sorted_rows = None, False
        kernels.pair_index(lazy)  # the wave-per-row passes
        n_rows = int(lazy.num_pair_rows_dev.item())
        n_fused = int(fused.num_pair_rows_dev.item())
        pr_f, pe_f = fused._pairs
        slots = pe_f.shape[0]
        live = min(int(fused.num_pairs_dev.item()), cap)
        assert (live < E) == (cap < E) and slots == (cap + n) // 2
        distinct = int(torch.unique(pr_f[:live]).numel())
        print(f"{name} loop={loop} cap={cap} E={E} live={live} slots={slots} rows: build {n_fused} "
              f"pair_index {n_sorted} / {n_rows} distinct {distinct}")
        assert torch.equal(pr_f, pr_l) and torch.equal(pe_f, pe_l)
        assert n_fused == n_sorted == n_rows
        assert n_fused == distinct and n_fused <= slots
        assert int(pr_f[:live].max()) < n_fused and not bool(pr_f[live:].any())


def test_pair_row_count_of_a_cut_row_and_the_slot_clamp():
    """40 atoms all within the cutoff (row t holds every source, the canonical ones are s >= t): a capacity that
    cuts row 0, and one that keeps more canonical edges than it has (cap + n) // 2 slots."""
    from torchmdnet import kernels
    n = 40
    pos = torch.zeros(n, 3, device=DEV)
    pos[:, 0] = torch.arange(n, device=DEV) * 0.01  # every pair inside the cutoff: row 0 is all canonical
    batch = torch.zeros(n, dtype=torch.long, device=DEV)
    cap = 30  # row 0 alone (40 canonical edges) overflows it: 30 kept canonical edges, (30 + 40) // 2 = 35 slots
    for pairs in (True, False):
        g = kernels.build_graph(pos, batch, 0.0, 5.0, 1 << 20, loop=True, strategy="brute",
                                static_capacity=cap, pairs=pairs)
        kernels.pair_index(g)
        assert int(g.num_pair_rows_dev.item()) == 30
    cap = 100  # rows 0, 1 and half of row 2: 40 + 39 + 18 canonical edges kept, (100 + 40) // 2 = 70 slots
    for pairs in (True, False):
        g = kernels.build_graph(pos, batch, 0.0, 5.0, 1 << 20, loop=True, strategy="brute",
                                static_capacity=cap, pairs=pairs)
        pr, pe = kernels.pair_index(g)
        assert int(g.num_pair_rows_dev.item()) == 70 == pe.shape[0] and int(pr.max()) < 70


# ----------------------------------------------------------------------------- the captured model
SIZES = (5, 9, 12)


def _tiny_et():
    from torchmdnet.models.model import create_model
    torch.manual_seed(77)
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=32, num_heads=4,
                     derivative=True, output_model="Scalar", precision=32)
    return create_model(args).to(DEV)


def _molecules():
    """3 molecules of 5, 9 and 12 atoms as jittered chains of spacing 1.5 along x (cutoff 5: an atom sees three
    neighbours either side, 4.5 +- 0.2 against 6.0 +- 0.2, nothing near the cutoff), and two moves of one atom of
    the last chain across the cutoff: its first atom away from everything (3 pairs lost), and its last atom to
    beside the first (3 pairs lost, 4 gained: the farthest at 4.66 +- 0.1)."""
    g = torch.Generator().manual_seed(5)
    pos, z, batch = [], [], []
    for i, m in enumerate(SIZES):
        p = torch.zeros(m, 3)
        p[:, 0] = 1.5 * torch.arange(m)
        p = p + 0.1 * torch.rand(m, 3, generator=g)
        p[:, 1] += 20.0 * i
        pos.append(p)
        z.append(torch.randint(1, 9, (m,), generator=g))
        batch.append(torch.full((m,), i, dtype=torch.long))
    pos, z, batch = torch.cat(pos), torch.cat(z), torch.cat(batch)
    first = sum(SIZES[:2])
    lost = pos.clone()
    lost[first] += torch.tensor([-30.0, 0.0, 0.0])  # no neighbour left but itself
    gained = pos.clone()
    gained[-1] = pos[first] + torch.tensor([0.0, 1.2, 0.0])
    return z.to(DEV), batch.to(DEV), [p.to(DEV) for p in (pos, lost, gained)]


def _pairs_of(model, z, pos, batch):
    g = model.representation_model.distance.graph(pos, batch)
    return int(g.num_pairs)


def test_captured_et_stops_at_the_live_pair_rows(monkeypatch):
    from torchmdnet import kernels
    from torchmdnet.graphs import GraphedEnergyForces
    model = _tiny_et()
    z, batch, (pos, lost, gained) = _molecules()
    counts = [_pairs_of(model, z, p, batch) for p in (pos, lost, gained)]
    assert counts[1] < counts[0] < counts[2], counts
    eager = []
    for p in (pos, lost, gained):
        y, f = model(z, p.clone(), batch)
        eager.append((y.detach().clone(), f.detach().clone()))
    seen = []
    real = kernels.proj_act

    def spy(*a, **kw):
        seen.append((a[0].shape[0], kw.get("rows")))
        return real(*a, **kw)

    monkeypatch.setattr(kernels, "proj_act", spy)
    results = []
    for cap in (None, 4 * counts[0]):  # the default margin; four times the live pairs
        del seen[:]
        gm = GraphedEnergyForces(model, z, pos, batch, edge_capacity=cap)
        assert gm.edge_capacity >= counts[2]
        # the captured projection ran over every pair slot of the capacity, with the device count
        assert seen and seen[-1][0] == (gm.edge_capacity + z.shape[0]) // 2 and seen[-1][1] is not None
        out = []
        for p in (pos, lost, gained, pos):
            y, f = gm(p)
            out.append((y.clone(), f.clone()))
        gm.check_capacity()
        gm.release()
        results.append(out)
    for out in results:
        for (y, f), (ye, fe) in zip(out, eager + eager[:1]):
            print("captured vs eager: max |dy|", float((y - ye).detach().abs().max()),
                  "max |df|", float((f - fe).detach().abs().max()))
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(f).all())
            assert torch.allclose(y, ye, rtol=1e-5, atol=1e-5) and torch.allclose(f, fe, rtol=1e-5, atol=1e-5)
    for (ya, fa), (yb, fb) in zip(*results):  # live rows do not depend on the capacity
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
        assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))
