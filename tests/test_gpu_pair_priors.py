"""Pair priors (ZBL, D2, Coulomb) on the GPU: csrc/pair_prior.hip through ``kernels.pair_prior`` and the prior
classes against the dense float64 restatement of tests/pair_prior_ref.py (itself pinned to the reference's
recorded outputs by tests/test_pair_priors_cpu.py).

Gates: float64 rtol 1e-9 / atol 1e-9 (the project's f64 convention, test_gpu_edge_cases.py); float32
max|d| / max|ref| <= 1e-4 (the project's parity gate)."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import golden, state_dict_from, yaml_args
import pair_prior_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALES = dict(distance_scale=1e-10, energy_scale=4.35974e-18)
NUMBERS = list(range(100))
KINDS = ["zbl", "d2", "coulomb"]
CUTOFF = {"zbl": 5.0, "d2": 10.0}


def _prior(kind, cutoff=None, max_nbr=None):
    from torchmdnet.priors import D2, ZBL, Coulomb
    if kind == "zbl":
        p = ZBL(cutoff or 5.0, max_nbr or 40, atomic_number=NUMBERS, **SCALES)
    elif kind == "d2":
        p = D2(cutoff or 10.0, max_nbr or 128, atomic_number=NUMBERS, dtype=torch.float64, **SCALES)
    else:
        p = Coulomb(0.3, max_nbr or 40, **SCALES)
    return p.to(DEV)


def _ref_fn(kind, z, batch, q, n_mol, cutoff=None):
    """The restatement's energy as a function of float64 positions on the GPU."""
    if kind == "zbl":
        return lambda p: R.zbl_energy(p, z, batch, n_mol, cutoff or 5.0, NUMBERS, **SCALES)
    if kind == "d2":
        t = _prior("d2")
        return lambda p: R.d2_energy(p, z, batch, n_mol, cutoff or 10.0, NUMBERS, c6=t.C_6, r_r=t.R_r, **SCALES)
    return lambda p: R.coulomb_energy(p, q, batch, n_mol, 0.3, **SCALES)


def _all_orders(energy, pos, w):
    """(y, F, d(sum F^2)/dpos, d/dw of |d(sum_b w_b y_b)/dpos|^2) of ``energy(pos) -> (n_mol,)``."""
    p = pos.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = energy(p).reshape(-1)
    f, = torch.autograd.grad(-y.sum(), p, create_graph=True)
    h, = torch.autograd.grad((f ** 2).sum(), p, retain_graph=True)
    gp, = torch.autograd.grad((w * y).sum(), p, create_graph=True)
    gw, = torch.autograd.grad((gp ** 2).sum(), w)
    return [t.detach().double().cpu() for t in (y, f, h, gw)]


def _prior_energy(prior, z, batch, q, n_mol):
    def energy(p):
        y0 = torch.zeros(n_mol, 1, dtype=p.dtype, device=p.device)
        return prior.post_reduce(y0, z, p, batch, None if q is None else {"partial_charges": q.to(p.dtype)})
    return energy


def _weights(n_mol):
    return torch.linspace(0.5, 1.7, n_mol, dtype=torch.float64, device=DEV)


def _check(got, ref, dtype, what):
    for name, a, b in zip(("y", "forces", "dF2", "dgy"), got, ref):
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{what} {name}: max|d| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    for name, a, b in zip(("y", "forces", "dF2", "dgy"), got, ref):
        if dtype == torch.float64:
            assert torch.allclose(a, b, rtol=1e-9, atol=1e-9), (what, name)
        else:
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), (what, name)


def _fixture():
    d = golden("priors_ref.npz")
    return (torch.tensor(d["z"], device=DEV), torch.tensor(d["pos"], device=DEV),
            torch.tensor(d["batch"], device=DEV), torch.tensor(d["partial_charges"], device=DEV))


@functools.lru_cache(maxsize=None)
def _fixture_ref(kind):
    """The restatement on the fixture input, computed once per kind and shared (read-only); on the CPU, where
    its own sums have a fixed order."""
    z, pos, batch, q = (t.cpu() for t in _fixture())
    return tuple(_all_orders(_ref_fn(kind, z, batch, q, 3), pos, _weights(3).cpu()))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_restatement(kind, dtype):
    z, pos, batch, q = _fixture()
    got = _all_orders(_prior_energy(_prior(kind), z, batch, q, 3), pos.to(dtype), _weights(3).to(dtype))
    _check(got, _fixture_ref(kind), dtype, f"{kind} {dtype}")


def _compare_case(kind, z, pos, batch, q, n_mol, cutoff=None, max_nbr=None):
    prior = _prior(kind, cutoff, max_nbr)
    w = _weights(n_mol)
    got = _all_orders(_prior_energy(prior, z, batch, q, n_mol), pos, w)
    ref = _all_orders(_ref_fn(kind, z, batch, q, n_mol, cutoff), pos, w)
    _check(got, ref, torch.float64, kind)
    return prior, got


def test_rows_longer_than_a_wave():
    """One molecule of 100 atoms in a 4 A blob, D2 cutoff 10: every row has 99 edges (more than a 16-lane group
    and more than a wave64, so the row loop runs 7 times)."""
    g = torch.Generator().manual_seed(3)
    grid = torch.stack(torch.meshgrid(torch.arange(5.0), torch.arange(5.0), torch.arange(4.0), indexing="ij"), -1)
    pos = grid.reshape(-1, 3).double() + (torch.rand(100, 3, generator=g, dtype=torch.float64) - 0.5) * 0.3
    z = torch.tensor([1, 6, 7, 8])[torch.randint(0, 4, (100,), generator=g)]
    batch = torch.zeros(100, dtype=torch.long)
    prior, _ = _compare_case("d2", z.to(DEV), pos.to(DEV), batch.to(DEV), None, 1)
    assert int(prior.last_num_pairs) == 100 * 99


@pytest.mark.parametrize("kind", KINDS)
def test_single_atom_molecules_have_zero_energy(kind):
    """Single-atom molecules first, in the middle and last: empty CSR rows, molecules without pairs get 0."""
    g = torch.Generator().manual_seed(4)
    batch = torch.tensor([0, 1, 1, 1, 1, 2, 3, 3, 3, 4])
    pos = torch.randn(10, 3, generator=g, dtype=torch.float64) * 1.2
    z = torch.tensor([8, 6, 1, 1, 7, 9, 6, 8, 1, 1])
    q = torch.randn(10, generator=g, dtype=torch.float64) * 0.4
    _, got = _compare_case(kind, z.to(DEV), pos.to(DEV), batch.to(DEV), q.to(DEV), 5)
    assert got[0][[0, 2, 4]].tolist() == [0.0, 0.0, 0.0]
    assert (got[0][[1, 3]] != 0).all()
    assert (got[1][[0, 5, 9]] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_third_order_through_the_composite(kind):
    """d/dpos of |d(sum F^2)/dpos|^2: the backward of the second-order Function differentiates the torch
    restatement of the kernel.  Both sides are float64 evaluations of the same formulas in another order of
    operations, so the bound is rounding: 1e-9 of the largest entry."""
    g = torch.Generator().manual_seed(6)
    batch = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1]).to(DEV)
    pos = (torch.randn(9, 3, generator=g, dtype=torch.float64) * 1.3).to(DEV)
    z = torch.tensor([8, 6, 1, 1, 7, 6, 8, 1, 1]).to(DEV)
    q = (torch.randn(9, generator=g, dtype=torch.float64) * 0.4).to(DEV)

    def third(energy):
        p = pos.clone().requires_grad_(True)
        f, = torch.autograd.grad(-energy(p).sum(), p, create_graph=True)
        h, = torch.autograd.grad((f ** 2).sum(), p, create_graph=True)
        t, = torch.autograd.grad((h ** 2).sum(), p)
        return t

    got = third(_prior_energy(_prior(kind), z, batch, q, 2))
    ref = third(_ref_fn(kind, z, batch, q, 2))
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{kind} third order: max|d| = {err:.3e}, max|ref| = {scale:.3e}")
    assert scale > 0 and err <= 1e-9 * scale


@pytest.mark.parametrize("kind", KINDS)
def test_two_atoms(kind):
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.7, -0.6, 0.9]], dtype=torch.float64, device=DEV)
    z = torch.tensor([8, 1], device=DEV)
    q = torch.tensor([-0.4, 0.3], dtype=torch.float64, device=DEV)
    _compare_case(kind, z, pos, torch.zeros(2, dtype=torch.long, device=DEV), q, 1)


def test_two_atoms_beyond_the_cutoff():
    """No pair at all (an empty list, n_slots = 0): zero energy, zero forces, no fault."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.0, 6.0, 0.0]], dtype=torch.float64, device=DEV)
    z = torch.tensor([8, 1], device=DEV)
    prior = _prior("zbl")
    p = pos.clone().requires_grad_(True)
    y = prior.post_reduce(torch.zeros(1, 1, dtype=torch.float64, device=DEV), z, p,
                          torch.zeros(2, dtype=torch.long, device=DEV), None)
    f, = torch.autograd.grad(y.sum(), p)
    assert int(prior.last_num_pairs) == 0 and float(y.detach().abs().max()) == 0 and float(f.abs().max()) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_interleaved_batch_equals_sorted(kind):
    z, pos, batch, q = _fixture()
    perm = torch.argsort(torch.arange(len(z), device=DEV) % 7, stable=True)  # interleaves the three molecules
    assert bool((batch[perm][1:] < batch[perm][:-1]).any())
    prior, w = _prior(kind), _weights(3)
    a = _all_orders(_prior_energy(prior, z, batch, q, 3), pos, w)
    b = _all_orders(_prior_energy(prior, z[perm], batch[perm], q[perm], 3), pos[perm], w)
    p = perm.cpu()
    # the same pairs in another summation order: float64 rounding of sums of < 100 terms, relative to the largest
    for x, y in ((a[0], b[0]), (a[1][p], b[1]), (a[2][p], b[2]), (a[3], b[3])):
        assert float((x - y).abs().max()) <= 1e-12 * float(y.abs().max())
    _check(b[:1] + [b[1][torch.argsort(p)], b[2][torch.argsort(p)], b[3]], _fixture_ref(kind), torch.float64,
           f"{kind} interleaved")


@pytest.mark.parametrize("kind", ["zbl", "d2"])
def test_pair_at_the_cutoff_is_excluded(kind):
    """Atoms 0 and 1 are exactly ``cutoff`` apart (r < cutoff is strict), atoms 1 and 2 further: only the pair
    (0, 2) interacts."""
    cut = 4.0
    pos = torch.tensor([[0.0, 0.0, 0.0], [cut, 0.0, 0.0], [-1.5, 0.0, 0.0]], dtype=torch.float64, device=DEV)
    z = torch.tensor([6, 8, 1], device=DEV)
    prior, got = _compare_case(kind, z, pos, torch.zeros(3, dtype=torch.long, device=DEV), None, 1, cutoff=cut)
    assert int(prior.last_num_pairs) == 2
    assert float(got[1][1].abs().max()) == 0.0 and float(got[1][0].abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_static_capacity_equals_dynamic(kind):
    z, pos, batch, q = _fixture()
    prior, w = _prior(kind), _weights(3)
    dyn = _all_orders(_prior_energy(prior, z, batch, q, 3), pos, w)
    n_pairs = int(prior.last_num_pairs)
    prior.static_capacity = 2 * n_pairs
    sta = _all_orders(_prior_energy(prior, z, batch, q, 3), pos, w)
    assert not prior.last_overflow.item() and int(prior.last_num_pairs.item()) == n_pairs
    for a, b in zip(sta, dyn):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
def test_padding_slots_get_exact_zeros(kind):
    """The per-slot gradients of a static-capacity list: the slots no row references hold exactly 0, first order
    (g_r) and second order (d_r), whatever the unwritten buffers held before."""
    from torchmdnet import kernels
    z, pos, batch, q = _fixture()
    prior = _prior(kind)
    cutoff = CUTOFF.get(kind, math.inf)
    n_pairs = kernels.build_graph(pos, batch, 0.0, cutoff, 128 * len(z), loop=False).num_pairs
    junk = torch.full((4 * n_pairs,), float("nan"), dtype=torch.float64, device=DEV)  # poison the allocator's blocks
    del junk
    p = pos.clone().requires_grad_(True)
    g = kernels.build_graph(p, batch, 0.0, cutoff, 128 * len(z), loop=False, static_capacity=2 * n_pairs)
    if kind == "zbl":
        Z = prior.atomic_number[z].double()
        a, b, kname = Z, Z.pow(0.23), "zbl"
    elif kind == "d2":
        Zm = prior.Z_map[z]
        a, b, kname = prior.C_6[Zm].sqrt(), prior.R_r[Zm], "d2"
    else:
        a, b, kname = q, None, "coulomb"
    y = kernels.pair_prior(kname, g, a, b, prior.constants(), batch, 3)
    g_r, = torch.autograd.grad(y.sum(), g.distances, create_graph=True)
    assert g_r.shape[0] == 2 * n_pairs
    assert bool((g_r[n_pairs:] == 0).all()) and bool((g_r[:n_pairs] != 0).any())
    d_r, = torch.autograd.grad((g_r ** 2).sum(), g.distances)
    assert bool((d_r[n_pairs:] == 0).all()) and bool(torch.isfinite(d_r).all())


def test_too_small_capacity_sets_the_flag():
    z, pos, batch, q = _fixture()
    prior = _prior("zbl")
    prior.static_capacity = 64
    p = pos.clone().requires_grad_(True)
    y = prior.post_reduce(torch.zeros(3, 1, dtype=torch.float64, device=DEV), z, p, batch, None)
    f, = torch.autograd.grad(y.sum(), p)
    torch.cuda.synchronize()
    assert prior.last_overflow.item() is True
    assert y.shape == (3, 1) and f.shape == p.shape
    prior.static_capacity = None
    with pytest.raises(RuntimeError, match="max_num_pairs"):  # the dynamic build's total-pairs check
        _prior("zbl", max_nbr=1).post_reduce(torch.zeros(3, 1, dtype=torch.float64, device=DEV), z, pos, batch, None)


# ----------------------------------------------------------------------------- whole model
ZBL_ARGS = dict(cutoff_distance=5.0, max_num_neighbors=40, atomic_number=NUMBERS, **SCALES)


def _et_tiny(with_zbl, precision=64):
    """The ``_model_from_fixture`` configuration of test_gpu_edge_cases.py with the weights of et_tiny_f64 and
    seeded Atomref offsets; with or without ZBL in front of Atomref."""
    from torchmdnet.models.model import create_model
    d = golden("et_tiny_f64.npz")
    args = yaml_args("equivariant-transformer", embedding_dimension=32, num_layers=2, num_rbf=16, num_heads=4,
                     max_num_neighbors=32, derivative=True, output_model="Scalar", precision=precision)
    args["prior_model"] = ([{"ZBL": dict(ZBL_ARGS)}] if with_zbl else []) + [{"Atomref": {"max_z": 100}}]
    m = create_model(args)
    sd = {k: torch.tensor(v).to(m.mean.dtype) if v.dtype.kind == "f" else torch.tensor(v)
          for k, v in state_dict_from(d).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("prior_model.") for k in missing)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        w = m.prior_model[-1].atomref.weight
        w.copy_(torch.randn(w.shape, generator=g, dtype=torch.float64).to(w.dtype))
    return m.to(DEV)


def test_model_with_zbl_equals_model_plus_restatement():
    from torchmdnet.priors import ZBL, Atomref
    z, pos, batch, _ = _fixture()
    mz, mb = _et_tiny(True), _et_tiny(False)
    assert [type(p) for p in mz.prior_model] == [ZBL, Atomref]
    ref = _ref_fn("zbl", z, batch, None, 3)

    def grads(model, extra_energy):
        p = pos.clone()
        y, f = model(z, p, batch)  # (p requires grad from here on)
        if extra_energy:
            e = ref(p).reshape(y.shape)
            fe, = torch.autograd.grad(-e.sum(), p, create_graph=True)
            y, f = y + e, f + fe
        loss = (y ** 2).sum() + (f ** 2).sum()
        params = [q for q in model.parameters() if q.requires_grad]
        return y.detach(), f.detach(), torch.autograd.grad(loss, params, allow_unused=True)

    y1, f1, g1 = grads(mz, False)
    y2, f2, g2 = grads(mb, True)
    assert torch.allclose(y1, y2, rtol=1e-9, atol=1e-9) and torch.allclose(f1, f2, rtol=1e-9, atol=1e-9)
    assert float((y1 - grads(mb, False)[0]).abs().min()) > 1.0  # ZBL is not a rounding error on this input
    names = [n for n, q in mz.named_parameters() if q.requires_grad]
    assert len(g1) == len(g2) and any(g is not None for g in g1)
    for n, a, b in zip(names, g1, g2):
        assert (a is None) == (b is None), n
        if a is not None:
            assert bool(torch.isfinite(a).all()), n
            assert torch.allclose(a, b, rtol=1e-7, atol=1e-7), (n, float((a - b).abs().max()))


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def test_graphed_energy_forces_with_zbl():
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.training import GraphedTrainStep, LNNPStep
    z, pos, batch, _ = _fixture()
    pos = pos.float()
    m = _et_tiny(True, precision=32)
    gm = GraphedEnergyForces(m, z, pos, batch)
    assert len(gm.priors) == 1 and gm.priors[0].static_capacity % 256 == 0
    g = torch.Generator().manual_seed(5)
    pos2 = pos + (torch.randn(pos.shape, generator=g) * 0.02).to(DEV)
    y1, f1 = gm(pos2)
    y1, f1 = y1.clone(), f1.clone()
    gm.check_capacity()
    gm.release()
    assert gm.priors[0].static_capacity is None
    y0, f0 = m(z, pos2.clone(), batch)
    assert _rel(y1, y0) < 1e-5 and _rel(f1, f0) < 1e-5
    # a prior capacity below its pair count: the replay must not fault, and the check must name the prior
    gs = GraphedEnergyForces(m, z, pos, batch, prior_capacity=256)
    gs(pos)
    with pytest.raises(RuntimeError, match="ZBL prior"):
        gs.check_capacity()
    gs.release()
    del gm, gs, y0, f0, y1, f1

    yl = torch.zeros(3, 1, device=DEV)
    fl = torch.zeros(len(z), 3, device=DEV)
    with pytest.raises(ValueError, match="LNNPStep"):
        GraphedTrainStep(m, z, pos, batch, yl, fl)
    before = [p.detach().clone() for p in m.parameters()]
    loss = LNNPStep(m, lr=1e-3).step(z, pos, batch, yl, fl)
    assert math.isfinite(float(loss))
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_padded_trainer_refuses_pair_priors():
    from torchmdnet.training import PaddedBatches, PaddedGraphedTrainer
    with pytest.raises(ValueError, match="pair priors"):
        PaddedGraphedTrainer(_et_tiny(True, precision=32), PaddedBatches([64], 4, 5.0))


def test_scripted_model_with_zbl_compiles_and_raises_when_called():
    from torchmdnet import _native
    _native.load_torch_ops()
    z, pos, batch, _ = _fixture()
    s = torch.jit.script(_et_tiny(True, precision=32))
    with pytest.raises(Exception, match="annotated to be ignored"):
        s(z, pos.float(), batch)
