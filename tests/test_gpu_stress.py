"""The differentiable virial on the GPU: tmdnet_nl_backward2 with the virial's cotangent (k_nl_backward2_virial),
``TorchMD_Net.energy_forces_virial(create_graph=True)`` and the stress term of ``training.LNNPStep``.

Kernel level: against ``kernels.nl_backward2_virial_composite`` evaluated in float64 on upcasts of the same device
tensors, on the 48 atoms of tests/test_gpu_virial.py (rows of a full 16-lane stride plus a remainder, short rows, an
empty row).  Model level: parameter and position gradients of a loss on the virial against the fp64 oracle with the
strained edge geometry (tests/stress_ref.py), labels random with a fixed seed.

Bars are tests/test_gpu_virial._close's (float64 rtol = atol = 1e-9; float32 max|d| <= 1e-4 max|ref|); float32
parameter gradients are compared per tensor, norm-relative with tests/test_gpu_train_parity._compare's floor, at FP32_BAR.
"""
import pytest
import torch
import torch.nn.functional as F

import gn_ref
import stress_ref as SR
import virial_ref as VR
from oracle import model_oracle as O
from test_gpu_gn import _outside_input, _small_args
from test_gpu_virial import CUTOFF, _atoms, _build, _close, _fixture_model, _same_call, _zbl_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
# float32 parameter gradients of a loss on the virial: worst parameter tensor, norm-relative against the fp64 oracle.
# Nobody had measured this quantity, so the bar follows a rule fixed beforehand: a fixture whose measured worst is
# <= 5e-5 is gated at the project's 1e-4 (tests/test_gpu_train_parity.TOL, 2x headroom); otherwise at twice the
# measured worst rounded up to one significant figure, never above 1e-3.  Measured on MI355X (stress-only loss):
#   et_tiny_periodic_f64         9.1e-7   -> 1e-4
#   tn_tiny_periodic_dyn_f64     1.1e-6   -> 1e-4
#   tn_tiny_periodic_static_f64  1.24e-4  -> 3e-4   (static_shapes: the padding copies of atom 0's self loop amplify
#                                                    float32 rounding; tests/test_gpu_virial.py
#                                                    leaves this fixture out in float32 for the first order already)
#   et_tiny_periodic_f64, E + F + stress 1 / 1 / 1 (test_combined_loss_step)  1.0e-6 -> 1e-4
FP32_BAR = {"et_tiny_periodic_f64": 1e-4, "tn_tiny_periodic_dyn_f64": 1e-4, "tn_tiny_periodic_static_f64": 3e-4}


# ----------------------------------------------------------------------------- kernel level
def _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol):
    """tmdnet_nl_backward2 with every output asked for: (d_pos, d_gd, d_gr)."""
    from torchmdnet import _native as nat
    lib = nat.load()
    cap = graph.n_edges
    nan = float("nan")
    d_pos = torch.full_like(pos, nan)
    d_gd = torch.full((cap, 3), nan, dtype=pos.dtype, device=pos.device)
    d_gr = torch.full((cap,), nan, dtype=pos.dtype, device=pos.device)
    rc = lib.tmdnet_nl_backward2(nat.dtype_code(pos.dtype), pos.shape[0], nat.ptr(graph.row_ptr), nat.ptr(graph.src),
                                 nat.ptr(graph.transpose), cap, nat.ptr(gd), nat.ptr(gr), nat.ptr(dl), nat.ptr(dist),
                                 nat.ptr(G), nat.ptr(batch), int(n_mol), nat.ptr(B), nat.ptr(d_pos), nat.ptr(d_gd),
                                 nat.ptr(d_gr), nat.stream(pos.device))
    nat.check(rc, "tmdnet_nl_backward2")
    torch.cuda.synchronize()
    return d_pos, d_gd, d_gr


def _operands(which, cot, E, rows, n, n_mol, dtype):
    """Random gd / gr for the E live edges (NaN in the rows beyond them: static padding) and cotangents G [n, 3] /
    B [n_mol, 3, 3] (B non-symmetric, different per molecule), each present or None."""
    g = torch.Generator().manual_seed(5)
    out = {}
    for name, shape in (("gd", (E, 3)), ("gr", (E,))):
        v = torch.randn(shape, generator=g, dtype=torch.float64)
        full = torch.full((rows,) + shape[1:], float("nan"), dtype=torch.float64)
        full[:E] = v
        out[name] = full.to(dtype).to(DEV) if name in which else None
    G = torch.randn(n, 3, generator=g, dtype=torch.float64)
    B = torch.randn(n_mol, 3, 3, generator=g, dtype=torch.float64)
    out["G"] = G.to(dtype).to(DEV) if "G" in cot else None
    out["B"] = B.to(dtype).to(DEV) if "B" in cot else None
    return out["gd"], out["gr"], out["G"], out["B"]


def _reference(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol):
    from torchmdnet import kernels
    up = lambda t: None if t is None else t.double()
    return kernels.nl_backward2_virial_composite(up(pos), up(G), up(B), up(gd), up(gr), up(dl), up(dist), graph.src,
                                                 graph.dst, batch, n_mol)


def _check(got, ref, dtype, what, E=None):
    for name, a, b in zip(("d_pos", "d_gd", "d_gr"), got, ref):
        _close(a, b, dtype, f"{what} {name}")
        if E is not None and name != "d_pos":
            assert float(a[E:].abs().max()) == 0, f"{what}: padding rows of {name}"


def _case(loop, which, cot, dtype, static=False, box=None, pos64=None, batch=None):
    if pos64 is None:
        pos64, batch = _atoms()
    pos = pos64.to(dtype).to(DEV)
    batch = batch.to(DEV)
    n_mol = int(batch.max()) + 1
    graph, dl, dist, E = _build(pos, batch, loop, static, box=None if box is None else box.to(dtype))
    gd, gr, G, B = _operands(which, cot, E, dl.shape[0], pos.shape[0], n_mol, dtype)
    return pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cot", [("B",), ("G",), ("B", "G")], ids=["B", "G", "B+G"])
@pytest.mark.parametrize("which", [("gd",), ("gr",), ("gd", "gr")], ids=["gd", "gr", "gd+gr"])
@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
def test_kernel_against_composite(loop, which, cot, dtype):
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(loop, which, cot, dtype)
    counts = (graph.row_ptr[1:] - graph.row_ptr[:-1]).cpu()
    assert int(counts[0]) == (30 if loop else 29) and int(counts[-1]) == (1 if loop else 0)
    got = _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)
    ref = _reference(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)
    _check(got, ref, dtype, f"loop={loop} {which} {cot}")
    assert float(ref[1].abs().max()) > 0 and float(ref[2].abs().max()) > 0
    if "gr" in which or "B" in cot:
        assert float(ref[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_periodic_image_shifts(dtype):
    """The atoms wrapped into a triclinic box (the box of tests/test_gpu_virial.py): edges across the cell faces carry
    an image shift, and B_m multiplies the minimum-image deltas, not pos[s] - pos[t]."""
    pos, batch = _atoms()
    L = 2.2 * CUTOFF
    box = torch.tensor([[L, 0, 0], [0.2 * L, L, 0], [0.1 * L, -0.15 * L, L]], dtype=torch.float64)
    pos = pos.clone()
    pos[30:] -= torch.tensor([20.0, 0.0, 0.0]) - 0.5 * box.sum(0)
    s = pos @ torch.linalg.inv(box)
    pos = (s - torch.floor(s)) @ box
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(False, ("gd", "gr"), ("B", "G"), dtype, box=box,
                                                                pos64=pos, batch=batch)
    raw = pos[graph.src[:E].long()] - pos[graph.dst[:E].long()]
    assert float((dl[:E] - raw).abs().max()) > 1.0, "no edge crosses a periodic image"
    got = _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)
    _check(got, _reference(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol), dtype, "triclinic")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_static_capacity_padding(dtype):
    """A static-capacity list with NaN in gd and gr at the padding slots: finite outputs, the padding rows of d_gd and
    d_gr exactly zero, the live rows those of the dynamic list."""
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(True, ("gd", "gr"), ("B", "G"), dtype, static=True)
    assert dl.shape[0] > E and bool(torch.isnan(gd[E:]).all()) and bool(torch.isnan(gr[E:]).all())
    got = _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)
    _check(got, _reference(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol), dtype, "static", E=E)
    dyn = _case(True, ("gd", "gr"), ("B", "G"), dtype)
    got_dyn = _raw(dyn[0], G, B, dyn[7], dyn[8], dyn[4], dyn[5], dyn[3], batch, n_mol)
    assert torch.equal(got[0], got_dyn[0]) and torch.equal(got[1][:E], got_dyn[1]) and torch.equal(got[2][:E], got_dyn[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_kernel_skips_molecules_outside_the_range(dtype):
    """batch values outside [0, n_mol) for the 12-atom molecule (one above, the rest negative): its rows behave as
    B = 0, bit for bit, and match the composite given the same batch."""
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(False, ("gd", "gr"), ("B", "G"), dtype)
    odd = batch.clone()
    odd[batch == 1] = -3
    odd[30] = n_mol
    got = _raw(pos, G, B, gd, gr, dl, dist, graph, odd, n_mol)
    B0 = B.clone()
    B0[1] = 0
    zeroed = _raw(pos, G, B0, gd, gr, dl, dist, graph, batch, n_mol)
    for a, b in zip(got, zeroed):
        assert torch.equal(a, b)
    _check(got, _reference(pos, G, B, gd, gr, dl, dist, graph, odd, n_mol), dtype, "outside")
    full = _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)
    assert not torch.equal(full[0][30:42], got[0][30:42]) and torch.equal(full[0][:30], got[0][:30])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("loop", [True, False], ids=["loop", "noloop"])
def test_zero_virial_cotangent_is_the_plain_second_order(loop, dtype):
    """g_virial all zeros (k_nl_backward2_virial) and NULL (k_nl_backward2, the launch of every step so far): equal
    bits on d_pos, d_gd and d_gr."""
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(loop, ("gd", "gr"), ("B", "G"), dtype)
    plain = _raw(pos, G, None, gd, gr, dl, dist, graph, batch, n_mol)
    zeros = _raw(pos, G, torch.zeros_like(B), gd, gr, dl, dist, graph, batch, n_mol)
    for name, a, b in zip(("d_pos", "d_gd", "d_gr"), zeros, plain):
        assert torch.equal(a, b), name
    assert float(plain[0].abs().max()) > 0
    from torchmdnet import kernels
    d_pos, d_gd, d_gr = kernels._NeighborGeomBwd2.apply(pos, G, gd, gr, dl, dist, graph)  # today's Function
    assert torch.equal(d_pos, plain[0]) and torch.equal(d_gd, plain[1]) and torch.equal(d_gr, plain[2])


def test_function_third_order_against_composite():
    """_NeighborGeomBwd2Virial's outputs equal the raw launch's, and differentiating them once more (w.r.t. G, B and
    the operands) equals autograd through the composite (float64)."""
    from torchmdnet import kernels
    dtype = torch.float64
    pos, batch, n_mol, graph, dl, dist, E, gd, gr, G, B = _case(False, ("gd", "gr"), ("B", "G"), dtype)
    g = torch.Generator().manual_seed(9)
    cots = [torch.randn(t.shape, generator=g, dtype=dtype).to(DEV) for t in (pos, gd, gr)]
    leaves = lambda: [t.clone().requires_grad_(True) for t in (G, B, gd, gr, pos)]
    G1, B1, gd1, gr1, p1 = leaves()
    outs = kernels._NeighborGeomBwd2Virial.apply(p1, G1, B1, gd1, gr1, dl, dist, graph, batch, n_mol)
    for a, b in zip(outs, _raw(pos, G, B, gd, gr, dl, dist, graph, batch, n_mol)):
        assert torch.equal(a.detach(), b)
    got = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), (G1, B1, gd1, gr1, p1))
    G2, B2, gd2, gr2, p2 = leaves()
    ref_outs = kernels.nl_backward2_virial_composite(p2, G2, B2, gd2, gr2, dl, dist, graph.src, graph.dst, batch, n_mol)
    ref = torch.autograd.grad(sum((o * c).sum() for o, c in zip(ref_outs, cots)), (G2, B2, gd2, gr2, p2))
    for name, a, b in zip(("G", "B", "gd", "gr", "pos"), got, ref):
        _close(a, b, dtype, f"third order d/d{name}")
        assert float(b.abs().max()) > 0, name


# ----------------------------------------------------------------------------- model level: the oracle, once per case
_ORACLE = {}


def _label(n_mol, seed=5):
    return torch.randn(n_mol, 3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _fixture_oracle(name, combined=False):
    """Oracle gradients of the stress-only loss (or E + F + stress, 1 / 1 / 1) on a periodic fixture at its float64
    weights, computed once per session and shared, read-only: (loss, parameter gradients, d loss / d pos, labels)."""
    key = (name, combined)
    if key not in _ORACLE:
        from torchmdnet.models.model import create_model
        sd, cfg, z, pos, batch, static = VR.fixture_case(name)
        m = create_model(VR.fixture_args(name, 64))
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        g = torch.Generator().manual_seed(17)
        labels = (torch.randn(1, 1, generator=g, dtype=torch.float64),
                  torch.randn(z.shape[0], 3, generator=g, dtype=torch.float64), _label(1))
        w = 1.0 if combined else 0.0
        loss, grads, gpos, _ = SR.oracle_stress_grads(m, cfg, z, pos, batch, labels[2], y=labels[0], neg_dy=labels[1],
                                                      w_y=w, w_f=w, static_shapes=static)
        _ORACLE[key] = (loss, grads, gpos, labels)
    return _ORACLE[key]


def _worst_relative(model, ref, what):
    """tests/test_gpu_train_parity._compare's figure -- per parameter tensor ||g - g_ref|| / max(||g_ref||, floor),
    floor = 1e-6 of the largest reference norm -- printed before the caller asserts on it."""
    floor = 1e-6 * max(float(g.norm()) for g in ref.values())
    worst = (0.0, None)
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        got = torch.zeros_like(p) if p.grad is None else p.grad
        d = float((got.detach().cpu().double() - ref[n]).norm()) / max(float(ref[n].norm()), floor)
        worst = max(worst, (d, n))
    print(f"{what}: worst parameter-gradient norm-relative error {worst[0]:.3g} ({worst[1]})")
    return worst


def _close_params(model, ref, what):
    seen = 0
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        got = torch.zeros_like(p) if p.grad is None else p.grad
        _close(got, ref[n], torch.float64, f"{what} {n}")
        seen += float(ref[n].abs().max()) > 0
    assert seen > 0


def test_default_is_unchanged_and_create_graph_attaches():
    """create_graph=False: detached, as before.  create_graph=True: the same forward and force pass, the virial
    attached and ``torch.equal`` to the default's.  On the float32 model: the per-molecule sum pass adds the per-atom
    values in double with LDS atomics whose order is not fixed (as the energy reduction, tests/test_gpu_virial.py
    ``_same_call``); float32 addends of like magnitude add exactly in double, so every order rounds to the same
    float32, while two float64 calls may differ in the last bit."""
    m, z, pos, batch, dtype = _fixture_model("et_tiny_periodic_f64", 32, "brute")
    y0, f0, w0 = m.energy_forces_virial(z, pos.clone(), batch)
    assert not w0.requires_grad and w0.grad_fn is None
    y, f, w = m.energy_forces_virial(z, pos.clone(), batch, create_graph=True)
    assert w.requires_grad and w.grad_fn is not None
    assert torch.equal(w.detach(), w0)
    _same_call(y, f, y0, f0)
    y1, f1, w1 = m.energy_forces_virial(z, pos.clone(), batch)  # and the next default call is detached again
    assert not w1.requires_grad and torch.equal(w1, w0)


@pytest.mark.parametrize("name", VR.PERIODIC_FIXTURES)
def test_stress_only_parameter_gradients_f64(name):
    """energy_forces_virial(create_graph=True), MSE(virial) and loss.backward() on the float64 model: every parameter
    gradient at the float64 bar against the oracle's.

    The oracle is evaluated with pairwise edge sums (tests/stress_ref.py).  With the oracle's one-after-the-other
    ``index_add`` the static_shapes fixture read 2.85e-8 at max|ref| = 5.3e2 on
    tensor_embedding.linears_tensor.0.weight (1.2e-8 on distance_proj1, 9.9e-9 on emb2.weight): the oracle's own
    summation error over the padding copies of atom 0's self loop.  Summed pairwise, the same tensors are 1.5e-10,
    6.7e-11 and 5.7e-11 from the GPU's (measured on MI355X)."""
    loss_ref, ref, _, (_, _, L) = _fixture_oracle(name)
    m, z, pos, batch, dtype = _fixture_model(name, 64, "brute")
    _, _, w = m.energy_forces_virial(z, pos.clone(), batch, create_graph=True)
    loss = F.mse_loss(w, L.to(DEV))
    loss.backward()
    assert abs(float(loss) - loss_ref) <= 1e-9 * abs(loss_ref)
    _close_params(m, ref, name)


@pytest.mark.parametrize("name", VR.PERIODIC_FIXTURES)
def test_stress_only_parameter_gradients_f32(name):
    """LNNPStep(y_weight = neg_dy_weight = 0, virial_weight = 1) on the float32 model -- only the virial term
    differentiates the force pass -- against the fp64 oracle, worst parameter tensor at the fixture's FP32_BAR (the
    measured values are listed there)."""
    from torchmdnet.training import LNNPStep
    loss_ref, ref, _, (y, f, L) = _fixture_oracle(name)
    m, z, pos, batch, dtype = _fixture_model(name, 32, "brute")
    tr = LNNPStep(m, lr=0.0, y_weight=0.0, neg_dy_weight=0.0, virial_weight=1.0)
    tr.opt.zero_grad(set_to_none=False)
    lt = tr.loss(z, pos.clone(), batch, y.float().to(DEV), f.float().to(DEV), virial=L.float().to(DEV))
    tr.backward(lt)
    assert abs(float(lt.detach()) - loss_ref) <= 1e-4 * abs(loss_ref)
    worst = _worst_relative(m, ref, f"{name} f32 stress only")
    assert worst[0] <= FP32_BAR[name], worst


def test_stress_only_position_gradient():
    """d loss / d pos of the stress-only loss on the ET periodic fixture (float64): d_pos of the second order, the
    B_m^T g term included, through the whole model."""
    name = "et_tiny_periodic_f64"
    _, _, gpos_ref, (_, _, L) = _fixture_oracle(name)
    m, z, pos, batch, dtype = _fixture_model(name, 64, "brute")
    p = pos.clone().requires_grad_(True)
    _, _, w = m.energy_forces_virial(z, p, batch, create_graph=True)
    gpos, = torch.autograd.grad(F.mse_loss(w, L.to(DEV)), p)
    assert float(gpos_ref.abs().max()) > 0
    _close(gpos, gpos_ref, torch.float64, "d loss / d pos")


def test_combined_loss_step():
    """LNNPStep(lr=0, y_weight=1, neg_dy_weight=1, virial_weight=1) .loss and .backward on the ET periodic fixture in
    float32: the loss within 1e-4 relative of the oracle's, the gradients at FP32_BAR."""
    from torchmdnet.training import LNNPStep
    name = "et_tiny_periodic_f64"
    loss_ref, ref, _, (y, f, L) = _fixture_oracle(name, combined=True)
    m, z, pos, batch, dtype = _fixture_model(name, 32, "brute")
    tr = LNNPStep(m, lr=0.0, y_weight=1.0, neg_dy_weight=1.0, virial_weight=1.0)
    tr.opt.zero_grad(set_to_none=False)
    lt = tr.loss(z, pos.clone(), batch, y.float().to(DEV), f.float().to(DEV), virial=L.float().to(DEV))
    tr.backward(lt)
    assert abs(float(lt.detach()) - loss_ref) <= 1e-4 * abs(loss_ref)
    worst = _worst_relative(m, ref, "ET f32 E + F + stress")
    assert worst[0] <= FP32_BAR[name], worst


def test_graph_network_stress_gradients():
    """Isolated molecules (float64): the restatement's virial is sum_{i in m} F_i (x) pos_i; stress-only parameter
    gradients against its autograd."""
    from torchmdnet.models.model import create_model
    torch.manual_seed(11)
    args = _small_args("add")
    model = create_model(args)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
    sd.update(leaves)
    z, pos, batch = _outside_input()
    L = _label(4)
    p = pos.clone().requires_grad_(True)
    y_ref = gn_ref.energy(sd, args, z, p, batch)
    f_ref, = torch.autograd.grad(-y_ref.sum(), p, create_graph=True)
    w_ref = torch.zeros(4, 3, 3, dtype=torch.float64).index_add(0, batch, f_ref.unsqueeze(2) * p.unsqueeze(1))
    g = torch.autograd.grad(F.mse_loss(w_ref, L), [leaves[n] for n in names], allow_unused=True)
    ref = {n: (torch.zeros_like(leaves[n]) if gi is None else gi) for n, gi in zip(names, g)}
    model = model.to(DEV)
    _, _, w = model.energy_forces_virial(z.to(DEV), pos.to(DEV), batch.to(DEV), create_graph=True)
    _close(w, w_ref, torch.float64, "gn virial")
    F.mse_loss(w, L.to(DEV)).backward()
    _close_params(model, ref, "gn")


def test_et_with_zbl_prior_stress_gradients():
    """The parameter-free ZBL prior adds a constant W_zbl to the virial (its own graph, a second share in the sink):
    the gradients with label L equal the oracle's (which has no prior) with label L - W_zbl.  Float64, isolated
    molecules."""
    from torchmdnet.models.model import create_model
    args = _zbl_args()
    torch.manual_seed(4)
    m = create_model(args).to(DEV)
    z, pos, batch = O.qm9_like(3)
    zd, pd, bd = z.to(DEV), pos.to(DEV), batch.to(DEV)
    _, _, w_all = m.energy_forces_virial(zd, pd.clone(), bd)
    prior, m.prior_model = m.prior_model, None
    _, _, w_net = m.energy_forces_virial(zd, pd.clone(), bd)
    m.prior_model = prior
    w_zbl = (w_all - w_net).detach()
    assert float(w_zbl.abs().max()) > 1e-6 * float(w_all.abs().max())
    L = _label(3)
    cfg = dict(args)
    cfg["prior_model"] = None
    _, ref, _, w_oracle = SR.oracle_stress_grads(m, cfg, z, pos, batch, L - w_zbl.cpu())
    _close(w_net, w_oracle, torch.float64, "et virial without the prior")
    _, _, w = m.energy_forces_virial(zd, pd.clone(), bd, create_graph=True)
    _close(w, w_all, torch.float64, "both shares, attached")
    F.mse_loss(w, L.to(DEV)).backward()
    _close_params(m, ref, "et+zbl")


# ----------------------------------------------------------------------------- refusals (raised before any launch)
def test_captured_trainers_refuse_a_virial_weight():
    from torchmdnet.training import GraphedTrainStep, PaddedGraphedTrainer
    m, z, pos, batch, dtype = _fixture_model("et_tiny_periodic_f64", 32, "brute")
    y, f = torch.zeros(1, 1, device=DEV), torch.zeros_like(pos)
    with pytest.raises(ValueError, match="virial_weight"):
        GraphedTrainStep(m, z, pos, batch, y, f, lr=0.0, virial_weight=1.0)
    with pytest.raises(ValueError, match="virial_weight"):
        PaddedGraphedTrainer(m, None, virial_weight=1.0)


def test_create_graph_is_refused_under_stream_capture(monkeypatch):
    """The check runs on the host before anything is enqueued, so it is exercised with the capture query answering
    yes -- no capture is opened for a call that is meant to fail."""
    from torchmdnet.models import utils
    m, z, pos, batch, dtype = _fixture_model("et_tiny_periodic_f64", 32, "brute")
    monkeypatch.setattr(utils, "check_stream_capturing", lambda: True)
    with pytest.raises(ValueError, match="stream capture"):
        m.energy_forces_virial(z, pos.clone(), batch, create_graph=True)
