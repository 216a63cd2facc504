"""The fused EquivariantScalar head (csrc/eq_head.hip, csrc/eq_head_x3.hip) across widths, atom tiles, the split
and unsplit transposed products, the ends of its envelope and zero norms, against ``kernels.eq_head_composite``
in float64 on the CPU (tests/eq_head_ref.py), evaluated at the float32-rounded inputs and weights when the
kernel is fp32: outputs, first order (g_x, g_vec through the Jacobian + k_scale and through the weight-gradient
factors, the 12 weight gradients, seed g_y) and second order (cotangents on (g_x, g_vec): d_x, d_vec, d_gy, the
12 weight terms through tmdnet_eq_head_hvp).  Every case keeps a zero-vector atom whose g_vec / d_vec rows must
be exactly 0.

Measure, per tensor: float64 allclose(rtol 1e-9, atol 1e-9); float32 max|d| <= 1e-4 max|ref|; a tensor whose
reference is identically zero is exactly zero or None.  Every figure is printed (``pytest -s``).  Worst float32
ratio max|d| / max|ref| measured on an MI355X, next to that 1e-4 bar:

    first order (per-atom kernels, all cases)    2.1e-6   g of block 2's vec1_proj.weight, H = 264, N = 3
    first order, four atoms per workgroup        7.6e-7   g of block 2's update_net[0].weight, H = 20
    second order (HVP kernel, all cases)         5.1e-5   d_x at H = 8, N = 2049 (3.7e-5 d_vec there; every
                                                          other case at most 1.6e-5)
    x3 head (fp32, H = 128)                      8.1e-7   g_vec, N = 16

The second order at H = 8 is the largest error among 2049 atoms (max|ref| 9.8 there against 0.74 at N = 5, where
the same width gives 1.3e-6); it keeps a factor 2 of room under the bar.

Which form runs is decided by LDS arithmetic over the two layouts of eq_head.hip, in values of T per atom:

    P  = align4(29.5 H + 8)     k_eq_head      (Layout)
    P2 = align4(61 H + 8)       k_eq_head_hvp  (Layout2)
    nt atoms fit if nt * P * sizeof(T) <= 65536; SPLIT if nt * (P + 1536) * sizeof(T) <= 65536

(``_form`` below restates it; the library's own answer at the four ends is pinned by the refusal tests).  nt = 1
below 2048 atoms, 2 from there where two fit (first order: else 1; TMDNET_HEAD_NT=4: 4, stepping down).  VEC
(16-byte loads) = H % 8 == 0.  Largest H per form:

    kernel       dtype  nt   split up to   unsplit up to
    first order  fp32   1    500           552
    first order  fp64   1    224           276
    first order  fp32   2    224           276
    first order  fp64   2     84           136
    first order  fp32   4     84           136
    first order  fp64   4     16            68
    HVP          fp32   1    240           268
    HVP          fp64   1    108           132
    HVP          fp32   2    108           132
    HVP          fp64   2     40            64

Every compiled instantiation and a case that runs it (H at N; N = 2049 runs nt = 2, N = 37 under
TMDNET_HEAD_NT=4 in tests/eq_head_nt_worker.py runs nt = 4); ``test_every_compiled_form_has_a_case`` derives the
same table from the case lists and fails if a form is left without one:

    k_eq_head<float, 1, VEC, SPLIT>     H = 8      k_eq_head<double, 1, VEC, SPLIT>     H = 8
    k_eq_head<float, 1, VEC, -->        H = 504    k_eq_head<double, 1, VEC, -->        H = 256
    k_eq_head<float, 1, --, SPLIT>      H = 4      k_eq_head<double, 1, --, SPLIT>      H = 4
    k_eq_head<float, 1, --, -->         H = 508    k_eq_head<double, 1, --, -->         H = 228
    k_eq_head<float, 2, VEC, SPLIT>     H = 8      k_eq_head<double, 2, VEC, SPLIT>     H = 8
    k_eq_head<float, 2, VEC, -->        H = 256    k_eq_head<double, 2, VEC, -->        H = 128
    k_eq_head<float, 2, --, SPLIT>      H = 20     k_eq_head<double, 2, --, SPLIT>      H = 20
    k_eq_head<float, 2, --, -->         H = 228    k_eq_head<double, 2, --, -->         H = 100
    k_eq_head<float, 4, VEC, SPLIT>     H = 64     k_eq_head<double, 4, VEC, SPLIT>     H = 8
    k_eq_head<float, 4, VEC, -->        H = 136    k_eq_head<double, 4, VEC, -->        H = 64
    k_eq_head<float, 4, --, SPLIT>      H = 20     k_eq_head<double, 4, --, SPLIT>      H = 12
    k_eq_head<float, 4, --, -->         H = 100    k_eq_head<double, 4, --, -->         H = 20
    k_eq_head_hvp<float, 1, VEC, SPLIT> H = 8      k_eq_head_hvp<double, 1, VEC, SPLIT> H = 8
    k_eq_head_hvp<float, 1, VEC, -->    H = 264    k_eq_head_hvp<double, 1, VEC, -->    H = 112
    k_eq_head_hvp<float, 1, --, SPLIT>  H = 4      k_eq_head_hvp<double, 1, --, SPLIT>  H = 4
    k_eq_head_hvp<float, 1, --, -->     H = 244    k_eq_head_hvp<double, 1, --, -->     H = 132
    k_eq_head_hvp<float, 2, VEC, SPLIT> H = 8      k_eq_head_hvp<double, 2, VEC, SPLIT> H = 8
    k_eq_head_hvp<float, 2, VEC, -->    H = 128    k_eq_head_hvp<double, 2, VEC, -->    H = 64
    k_eq_head_hvp<float, 2, --, SPLIT>  H = 20     k_eq_head_hvp<double, 2, --, SPLIT>  H = 20
    k_eq_head_hvp<float, 2, --, -->     H = 132    k_eq_head_hvp<double, 2, --, -->     H = 60
    k_scale<float>, k_scale<double>     every first-order case (the Jacobian path)
    k_head_x3                           test_x3_head_tile_edges

Beyond the envelope nothing is launched (TMDNET_UNSUPPORTED, outputs untouched) and the model takes the other
path: ``eq_head_fusable`` is false above fp32 552 / fp64 276 (the module blocks), and the head's second order
above fp32 268 / fp64 132 is the composite's.
"""
import ctypes
import functools
import os
import subprocess
import sys
import types

import pytest
import torch

import eq_head_ref as R
from test_eq_head import _head
from torchmdnet import _native as nat
from torchmdnet import kernels
from torchmdnet.models.output_modules import EquivariantScalar

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
WORST = {"first": [0.0], "second": [0.0], "x3": [0.0]}
FWD_MAX = {F32: 552, F64: 276}
HVP_MAX = {F32: 268, F64: 132}

# (H, dtype, N, orders): "1" first order, "2" second order
WIDTHS = [(H, dt, 5, "12") for H in (4, 12, 20, 100, 8, 24, 136, 256) for dt in (F32, F64)]
TILES = [(H, dt, 2049, "12") for H, dt in ((8, F32), (8, F64), (20, F32), (20, F64), (128, F64), (256, F32),
                                           (228, F32), (100, F64), (128, F32), (132, F32), (64, F64), (60, F64))]
SPLIT_EDGES = [(500, F32, 3, "1"), (504, F32, 3, "1"), (508, F32, 3, "1"), (224, F64, 3, "1"), (228, F64, 3, "1"),
               (240, F32, 3, "12"), (244, F32, 3, "12"), (108, F64, 3, "12"), (112, F64, 3, "12")]
ENDS = [(552, F32, 3, "1"), (276, F64, 3, "1"), (268, F32, 3, "12"), (264, F32, 3, "12"), (132, F64, 3, "12")]
BEYOND_HVP = [(272, F32, 3, "2"), (136, F64, 3, "2")]  # (fp64 136 and 256 at N = 5 are in WIDTHS as well)
CASES = WIDTHS + TILES + SPLIT_EDGES + ENDS + BEYOND_HVP
NT4 = [(20, F32), (64, F32), (100, F32), (136, F32), (8, F64), (12, F64), (20, F64), (64, F64)]  # the worker's


def _id(c):
    return f"H{c[0]}-{str(c[1])[6:]}-N{c[2]}"


def _select(order):
    cs = [c[:3] for c in CASES if order in c[3]]
    return pytest.mark.parametrize("H,dtype,N", cs, ids=[_id(c) for c in cs])


def _form(kernel, dtype, H, N, env_nt=0):
    """(nt, VEC, SPLIT) of the launch, or None outside the envelope: head_tile / launch_head_hvp restated."""
    es = 8 if dtype == F64 else 4
    per = ((59 * H // 2 + 8 if kernel == "first" else 61 * H + 8) + 3) & ~3
    cap = env_nt or (2 if N >= 2048 else 1)
    nts = [nt for nt in (4, 2, 1) if nt <= cap and nt * per * es <= 65536]
    if not nts:
        return None
    nt = nts[0]
    return nt, H % 8 == 0, nt * (per + 1536) * es <= 65536


@pytest.fixture(autouse=True)
def _per_atom_hand(monkeypatch):
    """The per-atom kernels and the hand-written second order, whatever the environment says."""
    monkeypatch.setattr(kernels, "HEAD_X3", False)
    monkeypatch.setattr(kernels, "HEAD_SECOND_ORDER", "hand")


@functools.lru_cache(maxsize=None)
def _case(H, dtype, N, zero=2, dead_channels=False, second=True):
    """One head, its inputs and the float64 reference, computed once and shared (never modified)."""
    head = _head(H, dtype)
    if dead_channels:
        R.zero_channels(head)
    ps = kernels.eq_head_params(head.output_network)
    x, vec, gy, cx, cv = R.inputs(N, H, dtype, zero=min(zero, N - 1) if zero >= 0 else N - 1)
    # a dead channel: autograd's double differentiation of the composite is NaN there, as the reference's
    # torch.norm (kernels.masked_norm restates that reference and stays as it is); the oracle is the
    # double-where norm, proven equal to the composite elsewhere by tests/test_eq_head_ref.py
    y, first, sec = R.reference(ps, x, vec, gy, cx if second else None, cv,
                                composite=R.composite_dw if dead_channels else None)
    if dead_channels:  # first order against the composite itself, which is finite there
        y, first, _ = R.reference(ps, x, vec, gy)
    dev = lambda t: t.to(DEV)  # noqa: E731
    return types.SimpleNamespace(H=H, dtype=dtype, N=N, zero=min(zero, N - 1) if zero >= 0 else N - 1,
                                 head=head.to(DEV), x=dev(x), vec=dev(vec), gy=dev(gy), cx=dev(cx), cv=dev(cv),
                                 y=y, first=first, second=sec, what=f"H={H} {str(dtype)[6:]} N={N}")


def _check_first(c, worst, forward=None):
    """y, the Jacobian path (tmdnet_eq_head_fwd + k_scale) and the weights path (tmdnet_eq_head_bwd_weights + the
    factor GEMMs) against the reference."""
    forward = forward or (lambda x, v: kernels.eq_scalar_head(x, v, c.head.output_network))
    ps = kernels.eq_head_params(c.head.output_network)
    xs, vs = c.x.clone().requires_grad_(True), c.vec.clone().requires_grad_(True)
    y = forward(xs, vs)
    R.close(y, c.y, c.dtype, f"{c.what} y", worst)
    jac = torch.autograd.grad(y, (xs, vs), c.gy, retain_graph=True)
    for name, a, b in zip(R.FIRST, jac, c.first):
        R.close(a, b, c.dtype, f"{c.what} jacobian {name}", worst)
    got = torch.autograd.grad(y, [xs, vs] + ps, c.gy)
    for name, a, b in zip(R.FIRST, got, c.first):
        R.close(a, b, c.dtype, f"{c.what} {name}", worst)
    assert not bool(jac[1][c.zero].any()) and not bool(got[1][c.zero].any())  # exactly 0, not merely small


def _check_second(c, worst, forward=None):
    """The force pass (g_x, g_vec with a graph, no weight gradients) differentiated again.  Returns whether
    tmdnet_eq_head_hvp refused (nothing launched) and the composite ran instead."""
    forward = forward or (lambda x, v: kernels.eq_scalar_head(x, v, c.head.output_network))
    ps = kernels.eq_head_params(c.head.output_network)
    xs, vs = c.x.clone().requires_grad_(True), c.vec.clone().requires_grad_(True)
    g = c.gy.clone().requires_grad_(True)
    refused = []
    orig = kernels.eq_head_hvp

    def spy(*a, **kw):
        res = orig(*a, **kw)
        refused.append(res is None)
        return res

    kernels.eq_head_hvp = spy
    try:
        y = forward(xs, vs)
        gx, gv = torch.autograd.grad(y, (xs, vs), g, create_graph=True)
        l2 = (gx * c.cx).sum() + (gv * c.cv).sum()
        got = torch.autograd.grad(l2, [xs, vs, g] + ps, allow_unused=True)
    finally:
        kernels.eq_head_hvp = orig
    for name, a, b in zip(R.SECOND, got, c.second):
        R.close(a, b, c.dtype, f"{c.what} {name}", worst)
    assert not bool(got[1][c.zero].any())
    assert kernels.head_pending_left() == 0
    return refused


# ----------------------------------------------------------------------------- the per-atom kernels
@_select("1")
def test_first_order(H, dtype, N):
    assert _form("first", dtype, H, N) is not None
    assert kernels.eq_head_fusable(_case(H, dtype, N).head.output_network)
    _check_first(_case(H, dtype, N), WORST["first"])


@_select("2")
def test_second_order(H, dtype, N):
    beyond = H > HVP_MAX[dtype]
    refused = _check_second(_case(H, dtype, N), [0.0] if beyond else WORST["second"])
    # inside its envelope the HVP kernel ran; beyond it nothing was launched and the composite answered
    assert refused == [beyond]
    assert (_form("hvp", dtype, H, N) is None) == (H > HVP_MAX[dtype])


def test_every_compiled_form_has_a_case():
    """k_eq_head x {float, double} x NT {1, 2, 4} x VEC x SPLIT and k_eq_head_hvp x ... x NT {1, 2}: each is the
    form of at least one case above (NT = 4: of the child process's cases)."""
    have = {("first", c[1], *_form("first", c[1], c[0], c[2])) for c in CASES if "1" in c[3]}
    have |= {("hvp", c[1], *f) for c in CASES if "2" in c[3] and (f := _form("hvp", c[1], c[0], c[2]))}
    have |= {("first", dt, *_form("first", dt, H, 37, env_nt=4)) for H, dt in NT4}
    want = {(k, dt, nt, v, s) for k, nts in (("first", (1, 2, 4)), ("hvp", (1, 2))) for dt in (F32, F64)
            for nt in nts for v in (True, False) for s in (True, False)}
    assert want <= have, sorted(map(str, want - have))
    assert _form("first", F32, 256, 37, env_nt=4)[0] == 2  # the worker's step-down case


def test_four_atoms_per_workgroup():
    """TMDNET_HEAD_NT=4, read once per process: one child process (tests/eq_head_nt_worker.py)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eq_head_nt_worker.py")
    res = subprocess.run([sys.executable, worker], env={**os.environ, "TMDNET_HEAD_NT": "4"}, timeout=300,
                         capture_output=True, text=True)
    print(res.stdout)
    print(res.stderr[-4000:])
    assert res.returncode == 0, res.returncode


# ----------------------------------------------------------------------------- the envelope's ends
SENT = -7.0


def _filled(*shape, dtype):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def _abi(entry, H, dtype, N=3):
    """One direct C-ABI call with every output pre-filled with SENT.  Returns (rc, outputs)."""
    lib = nat.load()
    ps =[p.detach() for p in kernels.eq_head_params(_head(H, dtype).to(DEV).output_network)]
    ws = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in ps])
    x, vec = torch.randn(N, H, dtype=dtype, device=DEV), torch.randn(N, 3, H, dtype=dtype, device=DEV)
    gy = torch.randn(N, 1, dtype=dtype, device=DEV)
    O = Q = H // 2
    code, st = nat.dtype_code(dtype), nat.stream(x.device)
    f = functools.partial(_filled, dtype=dtype)
    if entry == "fwd":
        outs = [f(N, 1), f(N, H), f(N, 3, H)]
        rc = lib.tmdnet_eq_head_fwd(code, N, H, nat.ptr(x), nat.ptr(vec), ws, *map(nat.ptr, outs), st)
    else:
        n = N if entry == "bwd_weights" else 2 * N
        saves = [f(n, 3, H + O), f(n, H), f(n, 2 * H + 1), f(n, 2 * O), f(n, H + 1), f(n, 3, Q + 1), f(n, 3, O),
                 f(n, Q), f(n, 2 * Q + 1), f(n, 2), f(n, Q + 1)]
        if entry == "bwd_weights":
            outs = [f(N, H), f(N, 3, H)]
            sv = (ctypes.c_void_p * 11)(*[t.data_ptr() for t in saves])
            rc = lib.tmdnet_eq_head_bwd_weights(code, N, H, nat.ptr(x), nat.ptr(vec), ws, nat.ptr(gy),
                                                *map(nat.ptr, outs), sv, st)
        else:
            saves.append(f(n, 3, H))
            outs = [f(N, H), f(N, 3, H), f(N, 1)]
            sv = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in saves])
            rc = lib.tmdnet_eq_head_hvp(code, N, H, nat.ptr(x), nat.ptr(vec), ws, nat.ptr(gy), nat.ptr(x),
                                        nat.ptr(vec), *map(nat.ptr, outs), sv, st)
        outs += saves
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("entry,limits", [("fwd", FWD_MAX), ("bwd_weights", FWD_MAX), ("hvp", HVP_MAX)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_refusal_launches_nothing(entry, limits, dtype):
    """The next legal width above each end: TMDNET_UNSUPPORTED and every output keeps its sentinel; the end
    itself is taken and writes them all.  This ties kernels.HEAD_MAX_HIDDEN to the library's answer."""
    assert limits is not FWD_MAX or kernels.HEAD_MAX_HIDDEN[dtype] == limits[dtype]
    rc, outs = _abi(entry, limits[dtype] + 4, dtype)
    assert rc == nat.UNSUPPORTED
    assert all(bool((t == SENT).all()) for t in outs)
    rc, outs = _abi(entry, limits[dtype], dtype)
    assert rc == 0
    assert not any(bool((t == SENT).all()) for t in outs)


@pytest.mark.parametrize("H,dtype", [(556, F32), (280, F64)], ids=["H556-float32", "H280-float64"])
def test_wider_than_the_forward_kernel_runs_the_blocks(H, dtype):
    """Above the first-order envelope the head is not routed to the fused kernel: EquivariantScalar.pre_reduce
    runs module by module, right in both orders."""
    c = _case(H, dtype, 3)
    assert not kernels.eq_head_fusable(c.head.output_network)
    assert kernels.eq_head_fusable(_case(FWD_MAX[dtype], dtype, 3, second=False).head.output_network)
    calls = []
    orig = kernels.eq_scalar_head
    kernels.eq_scalar_head = lambda *a: calls.append(1) or orig(*a)
    try:
        forward = lambda x, v: c.head.pre_reduce(x, v, None, None, None)  # noqa: E731
        _check_first(c, [0.0], forward)
        assert _check_second(c, [0.0], forward) == []
    finally:
        kernels.eq_scalar_head = orig
    assert not calls


def test_force_loss_step_beyond_the_hvp_envelope():
    """An fp64 ET at H = 256, the ET-QM9 width (one layer, six QM9-like molecules), takes one backward of an
    E + F loss: the head's forward and first backward are the fused kernels, its second order falls back to the
    composite, no factor rows stay handed off, and the parameter gradients equal the HEAD_SECOND_ORDER =
    "composite" run.  (Not H = 136, the first width beyond the HVP's fp64 end: the ET message kernels take
    only multiples of 32, so 256 is the narrowest ET there is beyond it; the head alone is checked at 136 by
    test_second_order.)"""
    from conftest import yaml_args
    from oracle import model_oracle as O
    from torchmdnet.models.model import create_model
    args = yaml_args("equivariant-transformer", embedding_dimension=256, num_layers=1, num_rbf=16, num_heads=8,
                     derivative=True, output_model="Scalar", precision=64)
    torch.manual_seed(3)
    m = create_model(args).to(DEV)
    z, pos, batch = (t.to(DEV) for t in O.qm9_like(6))
    refused = []
    orig = kernels.eq_head_hvp

    def spy(*a, **kw):
        res = orig(*a, **kw)
        refused.append(res is None)
        return res

    def grads(mode):
        kernels.HEAD_SECOND_ORDER = mode  # (restored by the autouse fixture's monkeypatch)
        m.zero_grad(set_to_none=True)
        y, f = m(z, pos, batch)
        ((y ** 2).mean() + (f ** 2).mean()).backward()
        assert kernels.head_pending_left() == 0
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    kernels.eq_head_hvp = spy
    try:
        hand = grads("hand")
    finally:
        kernels.eq_head_hvp = orig
    assert refused == [True]
    comp = grads("composite")
    assert hand.keys() == comp.keys() and any("output_model" in n for n in hand)
    for n in comp:
        R.close(hand[n], comp[n], F64, f"ET H=256 fp64 {n}")


@pytest.mark.parametrize("H,dtype", [(8, F32), (136, F64)], ids=["H8-float32", "H136-float64"])
def test_factor_rows_left_by_the_forward_node_are_summed(H, dtype):
    """The hand-off in its other order (the head's forward node has already left its weight-gradient factor
    rows when the second order runs): the second order returns both passes' weight gradients, through the
    HVP kernel's GEMMs inside its envelope and on top of the composite's terms beyond it."""
    c = _case(H, dtype, 5)
    ps = kernels.eq_head_params(c.head.output_network)
    xs, vs = c.x.clone().requires_grad_(True), c.vec.clone().requires_grad_(True)
    y = kernels.eq_scalar_head(xs, vs, c.head.output_network)
    gx, gv = torch.autograd.grad(y, (xs, vs), c.gy, create_graph=True)
    link = y.grad_fn.link
    with torch.no_grad():
        left = kernels._eq_head_weight_grads(nat.load(), c.x, c.vec, [p.detach() for p in ps], c.gy,
                                             torch.empty_like(c.x), torch.empty_like(c.vec), stash=link)
    assert left is None and link.pending is not None
    got = torch.autograd.grad((gx * c.cx).sum() + (gv * c.cv).sum(), ps, allow_unused=True)
    assert link.pending is None and kernels.head_pending_left() == 0
    for i, a in enumerate(got):
        first, second = c.first[2 + i], c.second[3 + i]
        R.close(a, first if second is None else first + second, dtype, f"{c.what} g_p{i} + d_p{i}")


# ----------------------------------------------------------------------------- zero norms, per channel
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
@pytest.mark.parametrize("H", [20, 24])
def test_one_dead_channel_among_live_ones(H, dtype):
    """Row 1 of block 1's vec1_proj.weight and row 0 of block 2's are zero: those channels' norms vanish on
    every atom while the others live.  First order against the composite (finite there), second order against
    the double-where reference (tests/eq_head_ref.py): the kernels' guards are per channel."""
    c = _case(H, dtype, 5, dead_channels=True)
    _check_first(c, WORST["first"])
    assert _check_second(c, WORST["second"]) == [False]


# ----------------------------------------------------------------------------- the 16-atom-tile MFMA head
@pytest.mark.parametrize("N", [1, 15, 16, 17, 33])
def test_x3_head_tile_edges(N, monkeypatch):
    """tmdnet_eq_head_x3_f32 at one atom, one short of a tile, a full tile, one and two tiles plus one atom; the
    zero-vector atom is the last one (the last live row of a partial tile).  Energies and the Jacobian-seeded
    g_x, g_vec against float64 and against the per-atom kernel; the energy-only call (NULL Jacobians)."""
    c = _case(128, F32, N, zero=-1, second=False)
    assert c.zero == N - 1
    monkeypatch.setattr(kernels, "HEAD_X3_MIN_ATOMS", 0)
    used = []
    orig = kernels._eq_head_x3

    def spy(*a):
        used.append(orig(*a))
        return used[-1]

    monkeypatch.setattr(kernels, "_eq_head_x3", spy)

    def run(x3):
        monkeypatch.setattr(kernels, "HEAD_X3", x3)
        xs, vs = c.x.clone().requires_grad_(True), c.vec.clone().requires_grad_(True)
        y = kernels.eq_scalar_head(xs, vs, c.head.output_network)
        return (y.detach(),) + torch.autograd.grad(y, (xs, vs), c.gy)

    mfma, valu = run(True), run(False)
    assert used == [True, False]
    ref = (c.y, c.first[0], c.first[1])
    for name, a, b, r in zip(("y", "g_x", "g_vec"), mfma, valu, ref):
        R.close(a, r, F32, f"x3 N={N} {name}", WORST["x3"])
        R.close(b, r, F32, f"per-atom N={N} {name}", WORST["first"])
        R.close(a, b, F32, f"x3 against per-atom N={N} {name}")
    assert not bool(mfma[2][N - 1].any())
    monkeypatch.setattr(kernels, "HEAD_X3", True)
    with torch.no_grad():
        y = kernels.eq_scalar_head(c.x, c.vec, c.head.output_network)
    assert used == [True, False, True]
    R.close(y, c.y, F32, f"x3 N={N} y, energy only", WORST["x3"])


def test_worst_ratios_are_reported():
    """Last in the file: the worst float32 ratio of each group over the cases that ran."""
    for k, v in WORST.items():
        print(f"worst fp32 max|d| / max|ref|, {k}: {v[0]:.2e} (bar 1e-4)")
        assert v[0] <= 1e-4
