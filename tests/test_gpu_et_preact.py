"""Pre-activated dk/dv rows (TMDNET_ET_PREACT): the projection GEMM with the activation in its epilogue
(tmdnet_proj_act_f32), the ET edge kernels reading S = act(pre) and D = act'(pre) * d pre / d r instead of
evaluating the activation per edge, and the stack / model wiring (et_stack.PREACT).

Bars as in test_gpu_et_widths: fp64 kernels 1e-12 forward, 1e-11 first order (max abs error over max abs value,
per tensor); fp32 kernels, per output tensor,

    e_k <= 2 * e_c + 4 * 2**-24 * scale

with e_k the error of the code under test against fp64, e_c the error of the RAW-ROW path (kernels.proj + the
activation in fp32, the fp32 composite, the model with PREACT off) against the same fp64, scale the max abs of
the fp64 result.  Every element is compared, every figure printed (``pytest -s``) before anything is asserted.

The "same bits" check of the epilogue: S against ``kernels.proj`` followed by the activation in fp32, at most
1 ulp apart, bit-equality reported.  The fp32 activation is the one the edge kernels evaluate in registers
(common.h Silu / ActF: hardware exp and reciprocal, each within 1 ulp, so e.g. their sigmoid is 2-5 ulp from
torch's division form -- measured -- and torch is no 1-ulp reference for it): ``_edge_kernel_act`` has k_fwd
itself evaluate it elementwise, on isolated atoms (self-loop rows, u = 0) with v = vec = 1, where
vec_out[t][0][c] = 1 * (1 * act(pv_1[t][c])) + (...) * 0 exactly.  1 ulp is the fp32 spacing at the reference
value -- for ShiftedSoftplus at softplus(x), the rounded quantity the constant log 2 is subtracted from (the
difference itself can be arbitrarily small).

Measured on an MI355X: S bit-equal to the edge kernels' evaluation for all four codes at K = 32 and 64; worst
fp32 share of the bar 0.54 (D at K = 32, SiLU, M = 1, N = 64; e_k / e_c 2.19), edge kernels 0.45 (g_r at H = 32),
model 0.50 (a dk_proj bias gradient of the double backward); worst fp64 relative error 1.2e-15.  The model's y is
NOT bit-equal between PREACT on and off (max |dy| 7.5e-9; forces 3.3e-7 of their max): the two k_fwd
instantiations contract their common arithmetic into FMAs differently.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as Fn

import test_gpu_et_widths as W
from conftest import yaml_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -24
LOG2 = 0.693147182464599609375


def _act(code, x):
    """(act(x), act'(x)) in x's dtype, the reference act_class_mapping codes."""
    sg = torch.sigmoid(x)
    if code == 0:
        return x * sg, sg * (1 + x * (1 - sg))
    if code == 1:
        return Fn.softplus(x) - LOG2, sg
    if code == 2:
        t = torch.tanh(x)
        return t, 1 - t * t
    return sg, sg * (1 - sg)


def _bar(rep, name, got, ref, comp):
    rep.check(name, got, ref, comp, 1e-12)


# ----------------------------------------------------------------------------- 1. projection epilogue
MS = (1, 31, 32, 33, 127, 128, 129)
NS = (16, 64, 80, 1024)


def _spacing(x):
    """fp32 spacing at |x| (x fp64; below the normal range: the smallest normal's)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64, device=x.device), e - 23)


EVAL_H = 16
EVAL_N = max(MS) * max(NS) // EVAL_H


@functools.lru_cache(maxsize=None)
def _iso_graph():
    """EVAL_N isolated atoms 10 apart: row t is the self loop t <- t, edge t."""
    j = torch.arange(EVAL_N)
    g = W._build(10.0 * torch.stack([j % 20, (j // 20) % 20, j // 400], 1).to(F64), EVAL_N)
    idx = torch.arange(EVAL_N, device=DEV)
    assert g.n_edges == EVAL_N and torch.equal(g.src.long(), idx) and torch.equal(g.dst.long(), idx)
    return g


def _edge_kernel_act(code, pre):
    """act(pre) elementwise as k_fwd evaluates the dk / dv activation ``code`` on raw rows (see the module
    docstring): pre's values as the v1 block of planar pv rows of EVAL_H channels."""
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    H, n = EVAL_H, EVAL_N
    flat = torch.zeros(n * H, dtype=F32, device=DEV)
    flat[:pre.numel()] = pre.reshape(-1)
    pv = torch.zeros(n, 3 * H, dtype=F32, device=DEV)
    pv[:, H:2 * H] = flat.view(n, H)
    one, zero = (lambda *s: torch.ones(*s, dtype=F32, device=DEV)), (lambda *s: torch.zeros(*s, dtype=F32, device=DEV))
    xo, vo = W._nan(n, H, dtype=F32), W._nan(n, 3, H, dtype=F32)
    kernels.et_message_fwd_launch(zero(n, H), zero(n, H), one(n, 3 * H), one(n, 3, H), None, pv, one(n), zero(n, 3),
                                  _iso_graph(), 2, xo, vo, flags=nat.ET_V_PLANAR | kernels.et_act_flags(code, 0))
    return vo[:, 0, :].reshape(-1)[:pre.numel()].view(pre.shape)


@pytest.mark.parametrize("code", [0, 1, 2, 3], ids=["silu", "ssp", "tanh", "sigmoid"])
@pytest.mark.parametrize("K", [32, 64])
def test_projection_epilogue_matches_fp64_and_raw_rows(K, code):
    """S and D of tmdnet_proj_act_f32 for every M x N, with and without dA / D, against fp64 formed from the fp32
    operands; S against kernels.proj + the fp32 activation within 1 ulp; NaN-filled outputs with a guard row and
    guard columns."""
    from torchmdnet import kernels
    rep = W._Report("proj-act")
    g = torch.Generator().manual_seed(100 + K + code)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F32).to(DEV)  # noqa: E731
    worst, biteq = 0.0, True
    for N in NS:
        Wt, b = rn(N, K) / K ** 0.5, rn(N)
        wp = kernels.proj_split(Wt)
        assert wp is not None
        for M in MS:
            A, dA = rn(M, K), rn(M, K)
            pre64 = A.double() @ Wt.double().t() + b.double()
            s64, ds64 = _act(code, pre64)
            d64 = ds64 * (dA.double() @ Wt.double().t())
            pre32 = kernels.proj(A, Wt, b, wp=wp)
            dpre32 = kernels.proj(dA, Wt, None, wp=wp)
            s32, ds32 = _act(code, pre32)
            d32 = ds32 * dpre32
            s_same = _edge_kernel_act(code, pre32)  # the edge kernels' own fp32 activation of the raw rows
            for der in (False, True):
                tag = f"K{K} act{code} M{M} N{N} {'S+D' if der else 'S'}"
                bufS, bufD = W._nan(M + 1, N + 8, dtype=F32), W._nan(M + 1, N + 8, dtype=F32)
                out = kernels.proj_act(A, dA if der else None, Wt, b, code, wp=wp,
                                       out=(bufS[:M, :N], bufD[:M, :N] if der else None))
                assert out is not None, tag
                S, D = out
                clean = W._untouched(bufS[M:], bufS[:, N:], bufD[M:], bufD[:, N:]) and \
                    (der or W._untouched(bufD))
                rep.require(clean, f"{tag}: a store into a guard row or column")
                _bar(rep, f"{tag} S", S, s64, s32)
                if der:
                    _bar(rep, f"{tag} D", D, d64, d32)
                at = Fn.softplus(pre32.double()) if code == 1 else s_same.double()
                ulps = float(((S.double() - s_same.double()).abs() / _spacing(at)).max())
                worst, biteq = max(worst, ulps), biteq and torch.equal(S, s_same)
                rep.require(ulps <= 1.0, f"{tag}: S {ulps:.3g} ulp from proj + activation")
    print(f"ETP|proj-act|K{K} act{code}|worst ulp distance {worst:.3g}|bit-equal {biteq}")
    rep.done()


def test_projection_epilogue_row_slice_of_a_stacked_weight_and_refusals():
    """row0: rows [row0, row0 + N) of a stacked weight's split give the rows of the slice's own launch, bit for
    bit; D without dA is refused (bad argument) with nothing written; outside the envelope: None."""
    from torchmdnet import kernels
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F32).to(DEV)  # noqa: E731
    K, M = 64, 129
    Wall, ball = rn(3 * 80, K) / 8, rn(3 * 80)
    wp = kernels.proj_split(Wall)
    A, dA = rn(M, K), rn(M, K)
    S1, D1 = kernels.proj_act(A, dA, Wall[80:160], ball[80:160], 0, wp=wp, row0=80)
    S2, D2 = kernels.proj_act(A, dA, Wall[80:160].contiguous(), ball[80:160].contiguous(), 0)
    Sa, Da = kernels.proj_act(A, dA, Wall, ball, 0, wp=wp)
    assert torch.equal(S1, S2) and torch.equal(D1, D2)
    assert torch.equal(S1, Sa[:, 80:160]) and torch.equal(D1, Da[:, 80:160])
    assert torch.equal(kernels.proj_act(A, None, Wall, ball, 0, wp=wp)[0], Sa)
    S, D = W._nan(M, 240, dtype=F32), W._nan(M, 240, dtype=F32)
    with pytest.raises(RuntimeError, match="tmdnet_proj_act_f32 failed: bad argument"):
        kernels.proj_act(A, None, Wall, ball, 0, wp=wp, out=(S, D))
    torch.cuda.synchronize()
    assert W._untouched(S, D)
    assert kernels.proj_act(A.double(), None, Wall.double(), ball.double(), 0) is None  # fp64: the raw rows
    assert kernels.proj_act(rn(M, 48), None, rn(32, 48), rn(32), 0) is None            # K = 48
    assert kernels.proj_act(A.cpu(), None, Wall.cpu(), ball.cpu(), 0) is None


# ----------------------------------------------------------------------------- 2. edge kernels
def _pre_ops(A, code=0):
    """The launch operands with pk / pv replaced by S and dpk / dpv by D, formed in fp64 from the same
    pre-activations the reference uses and rounded to the kernels' dtype."""
    B = dict(A)
    for k, dk in (("pk", "dpk"), ("pv", "dpv")):
        if A[k] is None:
            continue
        s, ds = _act(code, A[k].double())
        B[k], B[dk] = s.to(A[k].dtype), (ds * A[dk].double()).to(A[k].dtype)
    return B


def _bwd_pre(graph, heads, A, I, flags, edge_prefill=None, g_r=True, gp=False):
    """tmdnet_et_message_bwd in dr mode into NaN-filled guarded buffers (or, ``edge_prefill``, g_C / g_u / g_r
    pre-filled for TMDNET_ACC_EDGE).  Returns (grads in NAMES order, g_r, guards untouched, all buffers)."""
    from torchmdnet import kernels
    N, H = A["q"].shape
    E, dtype = graph.n_edges, A["q"].dtype
    bufs = [W._guarded(N, w, dtype=dtype) for w in (H, H, 3 * H)] + [W._guarded(N, 3, H, dtype=dtype)] + \
        [W._guarded(E, dtype=dtype), W._guarded(E, 3, dtype=dtype), W._guarded(E, dtype=dtype)]
    (gq, gk, gv, gw, gC, gu, gr), guards = [b[0] for b in bufs], [b[1] for b in bufs]
    gpk = W._nan(E, H, dtype=dtype) if gp else None
    if edge_prefill is not None:
        for buf, p in zip((gC, gu, gr), edge_prefill):
            buf.copy_(p)
    kernels.et_message_bwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph, heads,
                                  I["gx"], I["gvec"], gq, gk, gv, gw, gpk, None, gC, gu, accumulate=flags,
                                  pk_rows=A["rows"], dpk=A["dpk"], dpv=A["dpv"], g_r=gr if g_r else None)
    return [gq, gk, gv, gw, None, None, gC, gu], gr, W._untouched(*guards), [gq, gk, gv, gw, gC, gu, gr, gpk]


WIDTHS = [(32, 4), (64, 8), (128, 8), (256, 8)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H,heads", WIDTHS, ids=[f"H{h}x{n}" for h, n in WIDTHS])
def test_preact_edge_kernels_match_composite(H, heads, dtype):
    """k_fwd / k_bwd_both / k_bwd_dst + k_bwd_src with PRE at V = 1, 2, 4, 8 on rows of 1 to 130 edges: forward,
    backward in the one-grid and the two-launch form; pair rows, per-edge rows and the planar layout; g_r per pair,
    gq / gk / gv / gvec_in, g_C and g_u against the composite on the raw pre-activations."""
    from torchmdnet import _native as nat
    rep = W._Report("preact")
    graph, I, R = W._case_data("reduced", H, heads, dtype, 41)
    for lay_name, planar, pairs in (("pairs", False, True), ("planar+pairs", True, True), ("edges", False, False)):
        A = _pre_ops(W._operands(graph, heads, I, planar=planar, pairs=pairs))
        flags = nat.ET_PREACT | (nat.ET_V_PLANAR if planar else 0)
        tag = f"H{H}x{heads} {lay_name}"
        outs, clean = W._fwd(graph, heads, A, flags)
        rep.require(clean, f"{tag} fwd: a store past the last node row")
        W._check_outputs(rep, tag, outs, R)
        for form, both_max in (("both", None), ("dst+src", 0)):
            with W._tuning(both_max=both_max):
                grads, g_r, clean, _ = _bwd_pre(graph, heads, A, I, flags)
            rep.require(clean, f"{tag} {form}: a store into a guard row")
            W._check_grads(rep, f"{tag} {form}", graph, grads, g_r, R, A["lay"])
    rep.done()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("absent", ["pk", "pv"])
def test_preact_with_an_absent_projection(absent, dtype):
    """pk (pv) NULL under PREACT: the absent projection is the constant 1 and contributes nothing to g_r."""
    from torchmdnet import _native as nat
    rep = W._Report("preact-absent")
    H, heads = 64, 8
    graph = W._graph("reduced")
    I = dict(W._inputs(graph, H, dtype, 42))
    for k in (absent, "d" + absent, absent + "P", "d" + absent + "P"):
        I[k] = None
    fn = W._composite(graph, heads)
    names = [n for n in W.NAMES if n != absent]

    def run(cast):
        def f(*xs):
            d = dict(zip(names, xs))
            return fn(*[d.get(n) for n in W.NAMES])
        out, gr = W._first_order(f, [cast(I[n]) for n in names], (cast(I["gx"]), cast(I["gvec"])))
        grads = dict(zip(names, gr))
        other = "pv" if absent == "pk" else "pk"
        return out, [grads.get(n) for n in W.NAMES], (grads[other] * cast(I["d" + other])).sum(1)

    R = {}
    R["out"], R["grads"], R["g_r"] = run(lambda t: t.double())
    if dtype == F32:
        R["out32"], R["grads32"], R["g_r32"] = run(lambda t: t)
    A = _pre_ops(W._operands(graph, heads, {k: v for k, v in I.items()}, pairs=True))
    outs, clean = W._fwd(graph, heads, A, nat.ET_PREACT)
    rep.require(clean, "fwd: a store past the last node row")
    W._check_outputs(rep, f"no {absent}", outs, R)
    grads, g_r, clean, _ = _bwd_pre(graph, heads, A, I, nat.ET_PREACT)
    rep.require(clean, "bwd: a store into a guard row")
    W._check_grads(rep, f"no {absent}", graph, grads, g_r, R, A["lay"])
    rep.done()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_preact_acc_edge_and_static_capacity(dtype):
    """TMDNET_ACC_EDGE under PREACT: overwriting (NaN-filled buffers) and accumulating onto a pre-fill of g_C /
    g_u / g_r; and a static-capacity list: the valid rows equal the dynamic graph's bit for bit, the rows past
    row_ptr[N] are zero, the guard row past the capacity stays NaN."""
    from torchmdnet import _native as nat
    rep = W._Report("preact-acc")
    H, heads = 128, 8
    dyn, I, R = W._case_data("reduced", H, heads, dtype, 43)
    E = dyn.n_edges
    A = _pre_ops(W._operands(dyn, heads, I, pairs=True))
    grads, g_r, clean, _ = _bwd_pre(dyn, heads, A, I, nat.ET_PREACT)
    rep.require(clean, "overwrite: a store into a guard row")
    W._check_grads(rep, "overwrite", dyn, grads, g_r, R, A["lay"])
    g = torch.Generator().manual_seed(44)
    fill = [torch.randn(*s, generator=g, dtype=F64).to(dtype).to(DEV) for s in ((E,), (E, 3), (E,))]
    gacc, gr_acc, clean, _ = _bwd_pre(dyn, heads, A, I, nat.ET_PREACT | nat.ACC_EDGE, edge_prefill=fill)
    rep.require(clean, "accumulate: a store into a guard row")
    S = W._syms(dyn)
    for nm, got, ref, c, p, sym in (("gC", gacc[6], R["grads"][6], R.get("grads32", [None] * 8)[6], fill[0], S["C"]),
                                    ("gu", gacc[7], R["grads"][7], R.get("grads32", [None] * 8)[7], fill[1], S["u"]),
                                    ("g_r", gr_acc, R["g_r"], R.get("g_r32"), fill[2], S["g_r"])):
        rep.check(f"accumulate {nm}", sym(got), sym(ref + p.double()), None if c is None else sym(c + p), 1e-11)
    for i in range(4):
        rep.require(torch.equal(gacc[i], grads[i]), f"accumulate: node gradient {i} differs from the overwriting run")
    # static capacity (per-edge rows, capacity rows of finite junk)
    cap = E + 37
    st = W._build(W._positions(W.REDUCED)[0], cap, static=True)
    assert int(st.num_pairs_dev.item()) == E and st.n_edges == cap and torch.equal(st.row_ptr, dyn.row_ptr)
    Ae = _pre_ops(W._operands(dyn, heads, I))
    Ast = dict(Ae)
    for k in ("pk", "pv", "dpk", "dpv", "C", "u"):
        junk = torch.randn(cap - E, *Ae[k].shape[1:], generator=g, dtype=F64).to(dtype).to(DEV)
        Ast[k] = torch.cat([Ae[k], junk])
    res = {}
    for name, graph, ops in (("dyn", dyn, Ae), ("static", st, Ast)):
        outs, c0 = W._fwd(graph, heads, ops, nat.ET_PREACT)
        gs, gr, c1, _ = _bwd_pre(graph, heads, ops, I, nat.ET_PREACT)
        rep.require(c0 and c1, f"{name}: a store into a guard row")
        res[name] = outs + gs[:4] + [gs[6], gs[7], gr]
    for i, (a, b) in enumerate(zip(res["dyn"], res["static"])):
        valid = b[:E] if i >= 6 else b
        rep.require(torch.equal(valid, a), f"tensor {i}: the static-capacity graph differs from the dynamic one")
        if i >= 6:
            rep.require(bool((b[E:] == 0).all()), f"tensor {i}: padding rows not zeroed")
    W._check_outputs(rep, "static", res["static"][:2], R)
    sg = res["static"]
    W._check_grads(rep, "static", dyn, sg[2:6] + [None, None, sg[6], sg[7]], sg[8], R, Ae["lay"], n_edges=E)
    rep.done()


def test_preact_backward_refusals_write_nothing():
    """PREACT with gpk != NULL, and PREACT without gdist: TMDNET_BAD_ARGUMENT, no output touched."""
    from torchmdnet import _native as nat
    H, heads = 64, 8
    graph, I, _ = W._case_data("reduced", H, heads, F32, 45)
    A = _pre_ops(W._operands(graph, heads, I, pairs=True))
    for kw in (dict(gp=True), dict(g_r=False)):
        with pytest.raises(RuntimeError, match="tmdnet_et_message_bwd failed: bad argument"):
            _bwd_pre(graph, heads, A, I, nat.ET_PREACT, **kw)
    # (the buffers of a refused call are local to _bwd_pre: run the refusals again on buffers kept here)
    from torchmdnet import kernels
    N, E = graph.n_nodes, graph.n_edges
    outs = [W._nan(*s, dtype=F32) for s in ((N, H), (N, H), (N, 3 * H), (N, 3, H), (E, H), (E,), (E, 3), (E,))]
    gq, gk, gv, gw, gpk, gC, gu, gr = outs
    for gp, g_r in ((gpk, gr), (None, None)):
        with pytest.raises(RuntimeError, match="bad argument"):
            kernels.et_message_bwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph,
                                          heads, I["gx"], I["gvec"], gq, gk, gv, gw, gp, None, gC, gu,
                                          accumulate=nat.ET_PREACT, pk_rows=A["rows"], dpk=A["dpk"], dpv=A["dpv"],
                                          g_r=g_r)
    torch.cuda.synchronize()
    assert W._untouched(*outs)


# ----------------------------------------------------------------------------- 3. stack and model
def _molecules():
    """Four molecules of 1, 2, 9 and 30 atoms (the first has only its self-loop row), 50 apart."""
    g = torch.Generator().manual_seed(5)
    pos, batch = [], []
    for i, n in enumerate((1, 2, 9, 30)):
        k = int(round(n ** (1 / 3) + 0.5))
        grid = torch.cartesian_prod(*[torch.arange(k)] * 3).double()[:n] * 1.3
        pos.append(grid + 0.2 * torch.rand(n, 3, generator=g, dtype=F64) + torch.tensor([50.0 * i, 0, 0]))
        batch += [i] * n
    pos = torch.cat(pos)
    z = torch.randint(1, 10, (pos.shape[0],), generator=g)
    return z.to(DEV), pos.to(DEV), torch.tensor(batch, dtype=torch.long, device=DEV)


def _model(**kw):
    from torchmdnet.models.model import create_model
    torch.manual_seed(0)
    return create_model(yaml_args("equivariant-transformer", embedding_dimension=128, num_heads=8, num_layers=2,
                                  num_rbf=64, derivative=True, **kw)).to(DEV)


def _spy(monkeypatch):
    from torchmdnet import kernels
    calls, orig = [], kernels.proj_act

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(None if out is None else out[1] is not None)
        return out

    monkeypatch.setattr(kernels, "proj_act", spy)
    return calls


def _check_model(rep, name, on, off, ref):
    rep.check(name, on.detach(), ref.detach().double(), off.detach(), 1e-11)


def test_model_preact_on_against_off_and_fp64(monkeypatch):
    """Energy, forces and a double backward through the forces (no second-order expectation set) with PREACT on
    against the package's fp64 model on the same weights, e_c the error of the PREACT-off path."""
    from torchmdnet import et_stack
    rep = W._Report("preact-model")
    m = _model()
    m64 = copy.deepcopy(m).double()
    z, pos, batch = _molecules()
    calls = _spy(monkeypatch)
    names = [n for n, p in m.named_parameters() if p.requires_grad]

    def run(model, p, on):
        monkeypatch.setattr(et_stack, "PREACT", on)
        model.zero_grad(set_to_none=True)
        y, f = model(z, p, batch)
        ((f ** 2).sum() + y.sum()).backward()
        return y.detach(), f.detach(), [q.grad for _, q in model.named_parameters() if q.requires_grad]

    y1, f1, g1 = run(m, pos.float(), True)
    assert calls == [True], calls  # one launch, S and D
    y0, f0, g0 = run(m, pos.float(), False)
    assert calls == [True], calls
    yr, fr, gr = run(m64, pos, True)  # fp64: outside the envelope, the raw rows
    assert calls == [True], calls
    _check_model(rep, "y", y1, y0, yr)
    _check_model(rep, "forces", f1, f0, fr)
    print(f"ETP|preact-model|y bit-equal on/off {torch.equal(y1, y0)}|"
          f"forces max |on - off| / max |f| {float((f1 - f0).abs().max() / f0.abs().max()):.3g}")
    for n, a, b, c in zip(names, g1, g0, gr):
        if c is None:
            assert a is None and b is None, n
            continue
        _check_model(rep, f"double backward {n}", a, b, c)
    with torch.no_grad():  # no backward to follow: S only
        monkeypatch.setattr(et_stack, "PREACT", True)
        m.derivative = False
        y_ng = m(z, pos.float(), batch)[0]
        m.derivative = True
    assert calls == [True, False], calls
    _check_model(rep, "y (no grad)", y_ng, y0, yr)
    rep.done()


def test_training_step_never_calls_proj_act(monkeypatch):
    """Inside second_order_expected() (a force-matching training step) the stack keeps the raw rows."""
    from torchmdnet import et_stack
    m = _model()
    z, pos, batch = _molecules()
    calls = _spy(monkeypatch)
    with et_stack.second_order_expected():
        y, f = m(z, pos.float(), batch)
        ((f ** 2).sum() + (y ** 2).sum()).backward()
    assert calls == [], calls
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_graphed_energy_forces_replays_equal_eager(monkeypatch):
    """GraphedEnergyForces (static-capacity list) with PREACT: two replays at different positions equal eager
    (the relative bound of test_gpu_capture, 1e-5; bit-equality printed)."""
    from torchmdnet.graphs import GraphedEnergyForces
    m = _model()
    z, pos, batch = _molecules()
    calls = _spy(monkeypatch)
    gm = GraphedEnergyForces(m, z, pos.float(), batch)
    try:
        assert calls and all(c is True for c in calls), calls
        g = torch.Generator().manual_seed(9)
        for i in range(2):
            p = (pos + 0.05 * torch.randn(pos.shape, generator=g, dtype=F64).to(DEV)).float()
            y, f = gm(p)
            y, f = y.clone(), f.clone()
            gm.check_capacity()
            gm.release()
            ye, fe = m(z, p.clone(), batch)
            for d in gm.dists:
                d.static_capacity = gm.edge_capacity
            ry = float((y - ye).abs().max() / ye.abs().max())
            rf = float((f - fe).abs().max() / fe.abs().max())
            print(f"ETP|preact-graph|replay {i}|y rel {ry:.3g}|f rel {rf:.3g}|bit-equal {torch.equal(f, fe.detach())}")
            assert ry < 1e-5 and rf < 1e-5
    finally:
        gm.release()


def test_fused_projection_graphs_do_not_take_preact(monkeypatch):
    """fep_supported shapes with FEP_MIN_EDGES forced to 0 still run the fused-projection kernels."""
    from torchmdnet import et_stack, kernels
    assert kernels.fep_supported(128, 8, 64, F32)
    fused = []
    f0, b0 = kernels.et_fused_fwd_launch, kernels.et_fused_bwd_launch
    monkeypatch.setattr(kernels, "et_fused_fwd_launch", lambda *a, **k: (fused.append("f"), f0(*a, **k))[1])
    monkeypatch.setattr(kernels, "et_fused_bwd_launch", lambda *a, **k: (fused.append("b"), b0(*a, **k))[1])
    monkeypatch.setattr(et_stack, "FEP_MIN_EDGES", 0)
    calls = _spy(monkeypatch)
    m = _model()
    z, pos, batch = _molecules()
    y, f = m(z, pos.float(), batch)
    assert fused.count("f") == 2 and fused.count("b") == 2, fused  # one fused launch per layer and direction
    assert calls == [], calls
    assert torch.isfinite(y).all() and torch.isfinite(f).all()
