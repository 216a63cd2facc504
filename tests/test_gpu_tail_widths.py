"""The small kernels at the end of every forward and training step -- LayerNorm (csrc/layernorm.hip), the
per-molecule sums (csrc/reduce.hip) and the two-term MSE loss (csrc/loss.hip) -- at their edges, against the float64
restatements of tests/tail_ref.py evaluated on the kernel's own inputs.

LayerNorm (fp32).  Every TMD_LN_CPL form (2, 4, 6, 8, 16 values per lane) at both of its ends with a ragged last
lane group; rows around the 4-rows-per-block guard; weight-gradient rows around a chunk (16) and past 4096, where
the chunk grows to 17 (4097 rows are 241 whole chunks of 17; 4100 leave a final chunk of 3); zero rows; leading
dimensions larger than C; accumulate = 1; the second order with every cotangent and every output absent in turn;
ill-conditioned and constant rows; the envelope's ends.  Measure: row outputs, the worst row of (max |d| in the row
/ max |ref| in the row); gw and gb per column against the column's sum of |gy xhat| and of |gy|; mean against the
row's max |x|, rstd against itself.  Tolerance: the same measure of ATen's fp32 LayerNorm (native_layer_norm, its
backward and autograd's second order) on the same inputs on the GPU, err_hip <= MARGIN err_aten + 4 u (u = 2^-24).
The backward kernels and ATen's take the float32-rounded reference mean / rstd, so all three see one input.

    MARGIN = 16: the smallest power of two at least twice the largest err_hip / err_aten measured on an
    MI355X.  Worst ratios of that run, per group (``pytest -s`` prints every case):

        first order, widths (7 rows)        3.44   rstd at C = 192 (1.0e-7 against 3.0e-8, both within 2 u)
        first order, rows at C = 200        2.07   y at 3 rows
        weight gradient, chunks (C = 64)    4.89   gb at 4096 rows (2.1e-8 against 4.3e-9 of the column's sum of
                                                   |gy|: the kernel adds 16 rows and then 256 partials in sequence,
                                                   ATen in a tree; up to 17 rows the two are the same bits, ratio 1)
        second order                        2.05   d_x at C = 256 without Wb (3.0e-7 against 1.4e-7)
        rows of 1000 + randn                1.00   (y 2.7e-5 both at C = 513; 2.3e-5 against 1.4e-4 at C = 100)
        leading dimension 164, the wrapper  1.00

    Twice 4.89 is 9.8, so 16.  Every error outside the ill-conditioned rows is below 4e-7, and no ratio is above 8
    (test_layer_norm_ratios_are_reported fails on one: that is a finding in the kernel, not a margin to raise).

Molecule sums (fp32, fp64) and loss (fp32, fp64): nothing is measured.  The exact family (halves and small
integers: every partial sum is a float32 value) must equal the float64 answer bit for bit -- one atom dropped,
doubled or sent to another molecule changes it -- and the random family is held to the summation bounds derived
in tests/tail_ref.py (``sum_bound``, ``mse2_bound``); elementwise gradients to their product chain.
"""
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
from torchmdnet import _native as nat
from torchmdnet import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
EPS = 1e-5
SENT = -7.0
U32 = R.U[F32]
BAD_ARGUMENT = 1
MARGIN = 16.0
RATIOS = {}  # group -> (worst err_hip / err_aten, where)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _sent(*shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENT).all()) for t in ts)


def _st():
    return nat.stream(torch.device(DEV))


# ----------------------------------------------------------------------------- LayerNorm: raw entry points
def _ln_fwd(x, w, b, y=None):
    rows, C = x.shape
    y = torch.empty(rows, C, dtype=F32, device=DEV) if y is None else y
    mean, rstd = _sent(rows), _sent(rows)
    rc = nat.load().tmdnet_layernorm_fwd_f32(rows, C, nat.ptr(x), x.stride(0), nat.ptr(w), nat.ptr(b), EPS,
                                             nat.ptr(y), y.stride(0), nat.ptr(mean), nat.ptr(rstd), _st())
    assert rc == 0
    return y, mean, rstd


def _ln_bwd(x, w, mean, rstd, gy, gx=None, accumulate=0):
    rows, C = x.shape
    gx = _sent(rows, C) if gx is None else gx
    assert gx.is_contiguous() and gx.shape == (rows, C) and mean.shape == rstd.shape == (rows,)
    rc = nat.load().tmdnet_layernorm_bwd_f32(rows, C, nat.ptr(x), x.stride(0), nat.ptr(w), nat.ptr(mean),
                                             nat.ptr(rstd), nat.ptr(gy), gy.stride(0), nat.ptr(gx), accumulate, _st())
    assert rc == 0
    return gx


def _ln_wgrad(x, mean, rstd, gy):
    """(gw, gb); the workspace is exactly what the library asks for, followed by a guard that must survive."""
    rows, C = x.shape
    lib = nat.load()
    wsb = int(lib.tmdnet_layernorm_wgrad_workspace_bytes(rows, C))
    chunk = R.wgrad_chunk(rows)
    assert wsb == (R.ceil_div(rows, chunk) * 2 * C * 4 if rows else 0)
    ws = torch.full((wsb // 4 + 64,), float("nan"), device=DEV)  # (an integer sum may equal any finite sentinel)
    gw, gb = _sent(C), _sent(C)
    rc = lib.tmdnet_layernorm_wgrad_f32(rows, C, nat.ptr(x), x.stride(0), nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy),
                                        gy.stride(0), nat.ptr(gw), nat.ptr(gb), nat.ptr(ws), wsb, _st())
    assert rc == 0
    assert bool(torch.isnan(ws[wsb // 4:]).all()) and not bool(torch.isnan(ws[:wsb // 4]).any())  # all, no more
    return gw, gb


def _ln_bwd2(x, w, mean, rstd, gy, X, Wb, Bb, want=(True, True, True)):
    rows, C = x.shape
    outs = [_sent(rows, C) for _ in range(3)]  # d_gy, d_x, T
    ps = [nat.ptr(o) if on else None for o, on in zip(outs, want)]
    rc = nat.load().tmdnet_layernorm_bwd2_f32(rows, C, nat.ptr(x), x.stride(0), nat.ptr(w), nat.ptr(mean),
                                              nat.ptr(rstd), nat.ptr(gy), gy.stride(0), nat.ptr(X), nat.ptr(Wb),
                                              nat.ptr(Bb), *ps, _st())
    assert rc == 0
    return outs


def _judge(group, what, measure, hip, aten, ref, *scale):
    """err_hip <= MARGIN err_aten + 4 u in one measure (R.row_err / R.col_err), both printed and the ratio kept."""
    eh, ea = measure(hip, ref, *scale), measure(aten, ref, *scale)
    ratio = eh / ea if ea > 0 else float("nan")
    print(f"{what}: hip {eh:.3e}  aten {ea:.3e}  ratio {ratio:.2f}")
    if ratio > RATIOS.get(group, (0.0, ""))[0]:
        RATIOS[group] = (ratio, what)
    assert eh < float("inf"), f"{what}: not zero where the reference is identically zero"
    assert eh <= MARGIN * ea + 4 * U32, (what, eh, ea)


def _stats32(x, w, b):
    """The reference (y, mean, rstd) and the float32-rounded statistics every backward is given."""
    yr, mr, rr = R.ln_fwd(x, w, b, EPS)
    return yr, mr, rr, mr.float().to(DEV), rr.float().to(DEV)


def _check_forward(group, what, x, w, b, y=None):
    rows, C = x.shape
    yr, mr, rr, _, _ = _stats32(x, w, b)
    y, mean, rstd = _ln_fwd(x, w, b, y)
    ya, ma, ra = torch.native_layer_norm(x.contiguous(), [C], w, b, EPS)
    _judge(group, f"{what} y", R.row_err, y, ya, yr)
    _judge(group, f"{what} mean", R.col_err, mean, ma.reshape(-1), mr, x.abs().amax(1))
    _judge(group, f"{what} rstd", R.col_err, rstd, ra.reshape(-1), rr, rr)
    return y, mean, rstd


def _check_input_backward(group, what, x, w, b, gy):
    rows, C = x.shape
    _, _, _, m32, r32 = _stats32(x, w, b)
    gxr, _, _ = R.ln_bwd(x, w, m32, r32, gy)
    gx = _ln_bwd(x, w, m32, r32, gy)
    gxa = torch.ops.aten.native_layer_norm_backward(gy.contiguous(), x.contiguous(), [C], m32.view(rows, 1),
                                                    r32.view(rows, 1), w, b, [True, False, False])[0]
    _judge(group, f"{what} gx", R.row_err, gx, gxa, gxr)


def _check_weight_gradient(group, what, x, w, b, gy):
    rows, C = x.shape
    _, _, _, m32, r32 = _stats32(x, w, b)
    _, gwr, gbr = R.ln_bwd(x, w, m32, r32, gy)
    gw, gb = _ln_wgrad(x, m32, r32, gy)
    _, gwa, gba = torch.ops.aten.native_layer_norm_backward(gy.contiguous(), x.contiguous(), [C], m32.view(rows, 1),
                                                            r32.view(rows, 1), w, b, [False, True, True])
    xhat = (x.double() - m32.double()[:, None]) * r32.double()[:, None]
    _judge(group, f"{what} gw", R.col_err, gw, gwa, gwr, (gy.double() * xhat).abs().sum(0))
    _judge(group, f"{what} gb", R.col_err, gb, gba, gbr, gy.double().abs().sum(0))


def _first_order(group, rows, C):
    x, w, b, gy = _dev(*R.ln_inputs(rows, C)[:4])
    what = f"{rows}x{C}"
    _check_forward(group, what, x, w, b)
    _check_input_backward(group, what, x, w, b, gy)
    _check_weight_gradient(group, what, x, w, b, gy)


LN_WIDTHS = (1, 63, 64, 65, 128, 129, 192, 256, 257, 384, 385, 512, 513, 1000, 1024)


@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layer_norm_widths(C):
    """Every CPL form at both ends (128 | 129, 256 | 257, 384 | 385, 512 | 513, 1024), a ragged last lane group in
    each, one column, and 7 rows: two blocks, the second one short of a row."""
    _first_order("first order, widths", 7, C)


def test_layer_norm_width_cases_reach_every_form():
    forms = {}
    for C in LN_WIDTHS:
        forms.setdefault(R.ln_cpl(C), []).append(C)
    for cpl, first, last in ((2, 1, 128), (4, 129, 256), (6, 257, 384), (8, 385, 512), (16, 513, 1024)):
        assert first in forms[cpl] and last in forms[cpl] and any(C % 64 for C in forms[cpl])


@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_layer_norm_rows_around_a_block(rows):
    _first_order("first order, rows", rows, 200)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4096, 4097, 4100])
def test_layer_norm_weight_gradient_chunks(rows):
    """One short chunk, one row short of a chunk, a whole one, one row into the second; 256 chunks of 16; chunk 17
    in 241 whole chunks (4097) and with a final chunk of 3 (4100).  The workspace size is checked in _ln_wgrad."""
    x, w, b, gy = _dev(*R.ln_inputs(rows, 64)[:4])
    _check_weight_gradient("weight gradient, chunks", f"{rows}x64", x, w, b, gy)


def test_layer_norm_zero_rows():
    C = 64
    _, w, b, _, _, _, _ = _dev(*R.ln_inputs(1, C))
    lib = nat.load()
    x, y, gy, gx = (_sent(4, C) for _ in range(4))
    mean, rstd = _sent(4), _sent(4)
    assert lib.tmdnet_layernorm_fwd_f32(0, C, nat.ptr(x), C, nat.ptr(w), nat.ptr(b), EPS, nat.ptr(y), C,
                                        nat.ptr(mean), nat.ptr(rstd), _st()) == 0
    assert lib.tmdnet_layernorm_bwd_f32(0, C, nat.ptr(x), C, nat.ptr(w), nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy), C,
                                        nat.ptr(gx), 0, _st()) == 0
    d = [_sent(4, C) for _ in range(3)]
    assert lib.tmdnet_layernorm_bwd2_f32(0, C, nat.ptr(x), C, nat.ptr(w), nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy),
                                         C, nat.ptr(gx), nat.ptr(w), nat.ptr(b), *map(nat.ptr, d), _st()) == 0
    assert _untouched(x, y, gy, gx, mean, rstd, *d)
    assert lib.tmdnet_layernorm_wgrad_workspace_bytes(0, C) == 0
    for which in ((True, True), (True, False), (False, True)):  # no workspace: the empty sums are zeros
        gw, gb = _sent(C + 3), _sent(C + 3)
        rc = lib.tmdnet_layernorm_wgrad_f32(0, C, nat.ptr(x), C, nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy), C,
                                            nat.ptr(gw) if which[0] else None, nat.ptr(gb) if which[1] else None,
                                            None, 0, _st())
        assert rc == 0
        for t, on in zip((gw, gb), which):
            assert _untouched(t[C:]) and (bool((t[:C] == 0).all()) if on else _untouched(t))


def _column_view(t, ld=164, left=20):
    """t as columns [left, left + C) of a sentinel-filled [rows, ld] buffer."""
    buf = _sent(t.shape[0], ld)
    view = buf[:, left:left + t.shape[1]]
    view.copy_(t)
    return buf, view


def _only_view_written(buf, left, C):
    return _untouched(buf[:, :left], buf[:, left + C:])


def test_layer_norm_leading_dimensions():
    """x, y and gy are columns 20..119 of 164-wide buffers (ldx = ldy = ldg = 164): same answers as the dense
    operands bit for bit, and every column outside y's view keeps its sentinel."""
    rows, C = 9, 100
    x, w, b, gy, X, Wb, Bb = _dev(*R.ln_inputs(rows, C))
    (_, xv), (_, gv), (ybuf, yv) = _column_view(x), _column_view(gy), _column_view(torch.zeros_like(x))
    assert xv.stride(0) == gv.stride(0) == yv.stride(0) == 164
    y, mean, rstd = _check_forward("strided", "9x100 ld 164", xv, w, b, y=yv)
    assert y is yv and _only_view_written(ybuf, 20, C)
    yd, md, rd = _ln_fwd(x, w, b)
    assert torch.equal(yd, yv) and torch.equal(md, mean) and torch.equal(rd, rstd)
    _check_input_backward("strided", "9x100 ld 164", xv, w, b, gv)
    _check_weight_gradient("strided", "9x100 ld 164", xv, w, b, gv)
    assert torch.equal(_ln_bwd(x, w, mean, rstd, gy), _ln_bwd(xv, w, mean, rstd, gv))
    for a, d in zip(_ln_wgrad(xv, mean, rstd, gv), _ln_wgrad(x, mean, rstd, gy)):
        assert torch.equal(a, d)
    for a, d in zip(_ln_bwd2(xv, w, mean, rstd, gv, X, Wb, Bb), _ln_bwd2(x, w, mean, rstd, gy, X, Wb, Bb)):
        assert torch.equal(a, d)


def _layer_norm_both_orders(fn, x, w, b, gy, X, Wb, Bb):
    """(y, gx, gw, gb, d_gy, d_x, d_w) of fn(x, w, b) through autograd."""
    xs, ws, bs, gs = (t.detach().requires_grad_(True) for t in (x, w, b, gy))
    y = fn(xs, ws, bs)
    first = torch.autograd.grad(y, (xs, ws, bs), gs, create_graph=True)
    l2 = sum((g * c).sum() for g, c in zip(first, (X, Wb, Bb)))
    second = torch.autograd.grad(l2, (gs, xs, ws))
    return [t.detach() for t in (y, *first, *second)]


def test_layer_norm_strided_through_the_wrapper(monkeypatch):
    """kernels.layer_norm with x a column view (stride(0) = 164): the HIP kernels run (the leading dimension is
    theirs to take), first and second order."""
    from torchmdnet import tn_node
    monkeypatch.setattr(tn_node, "SECOND_ORDER", "hip")
    rows, C = 9, 100
    x, w, b, gy, X, Wb, Bb = _dev(*R.ln_inputs(rows, C))
    _, xv = _column_view(x)
    calls = []
    lib = nat.load()
    for name in ("tmdnet_layernorm_fwd_f32", "tmdnet_layernorm_bwd_f32", "tmdnet_layernorm_bwd2_f32"):
        orig = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _o=orig, _n=name: calls.append((_n, a[3])) or _o(*a))
    got = _layer_norm_both_orders(lambda *a: kernels.layer_norm(*a, EPS), xv, w, b, gy, X, Wb, Bb)
    assert calls == [("tmdnet_layernorm_fwd_f32", 164), ("tmdnet_layernorm_bwd_f32", 164),
                     ("tmdnet_layernorm_bwd2_f32", 164)]
    aten = _layer_norm_both_orders(lambda *a: F.layer_norm(a[0], (C,), a[1], a[2], EPS), x, w, b, gy, X, Wb, Bb)
    yr, mr, rr = R.ln_fwd(x, w, b, EPS)
    ref = [yr, *R.ln_bwd(x, w, mr, rr, gy), *R.ln_bwd2(x, w, mr, rr, gy, X, Wb, Bb)[:3]]
    xhat = (x.double().cpu() - mr[:, None]) * rr[:, None]
    for name, a, t, r in zip(("y", "gx", "gw", "gb", "d_gy", "d_x", "d_w"), got, aten, ref):
        if name in ("gw", "gb", "d_w"):
            g = gy.double().cpu()
            scale = {"gw": (g * xhat).abs().sum(0), "gb": g.abs().sum(0),
                     "d_w": (g * R.ln_bwd2(x, w, mr, rr, gy, X, Wb, Bb)[3]).abs().sum(0)}[name]
            _judge("wrapper, strided", f"layer_norm strided {name}", R.col_err, a, t, r, scale)
        else:
            _judge("wrapper, strided", f"layer_norm strided {name}", R.row_err, a, t, r)


def test_layer_norm_backward_accumulates():
    """accumulate = 1: gx += the input gradient.  The pre-fill holds integers, so the one add rounds once: the
    result is fl(pre-fill + gx of accumulate = 0) bit for bit, and that gx is held to the reference elsewhere."""
    rows, C = 7, 200
    x, w, b, gy = _dev(*R.ln_inputs(rows, C)[:4])
    _, mean, rstd = _ln_fwd(x, w, b)
    plain = _ln_bwd(x, w, mean, rstd, gy)
    pre = torch.arange(rows * C, dtype=F32, device=DEV).reshape(rows, C) % 13 - 6
    acc = _ln_bwd(x, w, mean, rstd, gy, gx=pre.clone(), accumulate=1)
    assert torch.equal(acc, pre + plain)
    ref = pre.double().cpu() + R.ln_bwd(x, w, mean, rstd, gy)[0]
    assert R.row_err(acc, ref) <= 8 * U32  # two roundings of values up to 6 + |gx| against the row's largest


SECOND_VARIANTS = ("all", "no X", "no Wb", "no Bb", "no d_gy", "no d_x", "no T")


@pytest.mark.parametrize("C", [64, 100, 256, 512, 1024])
def test_layer_norm_second_order(C):
    """tmdnet_layernorm_bwd2_f32, 6 rows: each cotangent NULL in turn, each output NULL in turn (it keeps its
    sentinel; the others are the same bits as with it).  ATen's side is autograd's double differentiation of
    F.layer_norm in fp32, and for T the first backward's gx of (gy = X, w = 1), the same projection."""
    rows = 6
    x, w, b, gy, X, Wb, Bb = _dev(*R.ln_inputs(rows, C))
    _, mr, rr, m32, r32 = _stats32(x, w, b)
    full = None
    for variant in SECOND_VARIANTS:
        cot = [None if variant == f"no {n}" else t for n, t in zip(("X", "Wb", "Bb"), (X, Wb, Bb))]
        want = [variant != f"no {n}" for n in ("d_gy", "d_x", "T")]
        outs = _ln_bwd2(x, w, m32, r32, gy, *cot, want=want)
        for o, on in zip(outs, want):
            assert on or _untouched(o), variant
        if variant == "all":
            full = outs
        if not all(want):  # an absent output changes nothing in the others
            for o, f_, on in zip(outs, full, want):
                assert not on or torch.equal(o, f_), variant
            continue
        d_gy, d_x, _, T = R.ln_bwd2(x, w, m32, r32, gy, *cot)
        xs, gs = x.clone().requires_grad_(True), gy.clone().requires_grad_(True)
        ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ya = F.layer_norm(xs, (C,), ws, bs, EPS)
        g1 = torch.autograd.grad(ya, (xs, ws, bs), gs, create_graph=True)
        l2 = sum((g * c).sum() for g, c in zip(g1, cot) if c is not None)
        a_gy, a_x = torch.autograd.grad(l2, (gs, xs), allow_unused=True)
        a_x = torch.zeros_like(x) if a_x is None else a_x
        what = f"6x{C} {variant}"
        _judge("second order", f"{what} d_gy", R.row_err, outs[0], a_gy, d_gy)
        _judge("second order", f"{what} d_x", R.row_err, outs[1], a_x, d_x)
        if cot[0] is None:
            assert not bool(outs[2].any())
        else:
            ones = torch.ones_like(w)
            a_T = torch.ops.aten.native_layer_norm_backward(X, x, [C], m32.view(rows, 1), r32.view(rows, 1), ones,
                                                            ones, [True, False, False])[0]
            _judge("second order", f"{what} T", R.row_err, outs[2], a_T, T)


@pytest.mark.parametrize("C", [100, 513])
def test_layer_norm_row_conditioning(C):
    """Rows of 1000 + randn (a one-pass variance E[x^2] - E[x]^2 loses every digit of a unit variance beside 10^6
    in fp32) and a constant row of 0.5: x - mean is exactly 0 there, so y is b bit for bit and rstd is eps^-1/2."""
    x, w, b = _dev(*R.ln_inputs(6, C, offset=1000.0)[:3])
    x[4] = 0.5
    y, mean, rstd = _check_forward("conditioning", f"6x{C} + 1000", x, w, b)
    assert torch.equal(y[4], b)
    assert float(mean[4]) == 0.5
    assert abs(float(rstd[4]) / EPS ** -0.5 - 1) <= 1e-6
    yr, _, rr = R.ln_fwd(x, w, b, EPS)
    assert R.row_err(y, yr) <= 1e-3  # 1000 u against a unit spread, a few times over; a one-pass form is O(1) off
    assert R.col_err(rstd, rr, rr) <= 1e-3


def test_layer_norm_bias_gradient_of_integers_is_exact():
    rows, C = 4100, 65
    x, w, b, _ = _dev(*R.ln_inputs(rows, C)[:4])
    g = torch.Generator().manual_seed(3)
    gy = torch.randint(-8, 9, (rows, C), generator=g).float().to(DEV)
    _, mean, rstd = _ln_fwd(x, w, b)
    _, gb = _ln_wgrad(x, mean, rstd, gy)
    assert torch.equal(gb.cpu(), gy.double().sum(0).float().cpu())


def test_layer_norm_envelope():
    """C = 1025, a leading dimension below C and a NULL x: TMDNET_BAD_ARGUMENT, nothing written.  kernels.layer_norm
    does not ask for C = 1025: ATen's route, and it matches."""
    lib = nat.load()
    rows = 3
    for C, ld, null_x in ((1025, 1025, False), (100, 99, False), (100, 100, True)):
        x, y, gy, gx = (_sent(rows, 1025) for _ in range(4))
        w, b, mean, rstd = _sent(1025), _sent(1025), _sent(rows), _sent(rows)
        xp = None if null_x else nat.ptr(x)
        d = [_sent(rows, 1025) for _ in range(3)]
        assert lib.tmdnet_layernorm_fwd_f32(rows, C, xp, ld, nat.ptr(w), nat.ptr(b), EPS, nat.ptr(y), C, nat.ptr(mean),
                                            nat.ptr(rstd), _st()) == BAD_ARGUMENT
        assert lib.tmdnet_layernorm_bwd_f32(rows, C, xp, ld, nat.ptr(w), nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy), C,
                                            nat.ptr(gx), 0, _st()) == BAD_ARGUMENT
        assert lib.tmdnet_layernorm_bwd2_f32(rows, C, xp, ld, nat.ptr(w), nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy), C,
                                             nat.ptr(gx), nat.ptr(w), nat.ptr(b), *map(nat.ptr, d), _st()) \
            == BAD_ARGUMENT
        if C <= 1024:  # (the weight gradient strides its columns: it has no width limit)
            assert lib.tmdnet_layernorm_wgrad_f32(rows, C, xp, ld, nat.ptr(mean), nat.ptr(rstd), nat.ptr(gy), C,
                                                  nat.ptr(gx), nat.ptr(y), nat.ptr(d[0]), 1025 * 4 * 3, _st()) \
                == BAD_ARGUMENT
        assert _untouched(x, y, gy, gx, w, b, mean, rstd, *d)
    C = 1025
    x, w, b, gy, X, Wb, Bb = _dev(*R.ln_inputs(5, C))
    called = []
    orig = lib.tmdnet_layernorm_fwd_f32
    lib.tmdnet_layernorm_fwd_f32 = lambda *a: called.append(1) or orig(*a)
    try:
        got = _layer_norm_both_orders(lambda *a: kernels.layer_norm(*a, EPS), x, w, b, gy, X, Wb, Bb)
    finally:
        lib.tmdnet_layernorm_fwd_f32 = orig
    assert not called
    yr, mr, rr = R.ln_fwd(x, w, b, EPS)
    ref = [yr, *R.ln_bwd(x, w, mr, rr, gy), *R.ln_bwd2(x, w, mr, rr, gy, X, Wb, Bb)[:3]]
    for name, a, r in zip(("y", "gx", "gw", "gb", "d_gy", "d_x", "d_w"), got, ref):
        err = R.row_err(a, r)
        print(f"layer_norm C=1025 (ATen) {name}: {err:.2e}")
        assert err <= 1e-4  # the project's fp32 bar for a route that is not the kernel's


# ----------------------------------------------------------------------------- molecule sums
def _scalar(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


def _atom_sum(x, batch, n_mol, std, mean, dtype, expect=0):
    """tmdnet_atom_sum_fwd on CPU operands; x keeps one element when there are no atoms (a pointer to pass)."""
    n = x.shape[0]
    xd = torch.cat([x, x.new_zeros(1)]).to(DEV) if n == 0 else x.to(DEV)
    bd = torch.cat([batch, batch.new_zeros(1)]).to(DEV) if n == 0 else batch.to(DEV)
    y = _sent(n_mol + 3, dtype=dtype)
    sd, md = _scalar(std, dtype), _scalar(mean, dtype)  # (named: they must outlive the launch)
    rc = nat.load().tmdnet_atom_sum_fwd(nat.dtype_code(dtype), n, n_mol, nat.ptr(xd), nat.ptr(bd), nat.ptr(sd),
                                        nat.ptr(md), nat.ptr(y), _st())
    assert rc == expect
    assert _untouched(y[n_mol:] if rc == 0 else y)
    return y[:n_mol].cpu()


def _dot_sum(h, w, b0, batch, n_mol, std, mean, dtype, with_buf, pad=0):
    """tmdnet_dot_sum_fwd on CPU operands -> (y, atom_buf or None); ``pad`` sentinel columns after each row of h."""
    n, K = h.shape
    hb = _sent(max(n, 1), K + pad, dtype=dtype)
    hb[:n, :K] = h.to(DEV)
    bd = torch.cat([batch, batch.new_zeros(1)]).to(DEV)
    buf = _sent(n + 3, dtype=dtype) if with_buf else None
    y = _sent(n_mol + 3, dtype=dtype)
    wd, b0d, sd, md = w.to(DEV), _scalar(b0, dtype), _scalar(std, dtype), _scalar(mean, dtype)
    rc = nat.load().tmdnet_dot_sum_fwd(nat.dtype_code(dtype), n, K, nat.ptr(hb), K + pad, nat.ptr(wd), nat.ptr(b0d),
                                       n_mol, nat.ptr(bd), nat.ptr(sd), nat.ptr(md), nat.ptr(buf), nat.ptr(y), _st())
    assert rc == 0
    assert _untouched(y[n_mol:], hb[:, K:]) and (buf is None or _untouched(buf[n:]))
    return y[:n_mol].cpu(), None if buf is None else buf[:n].cpu()


def _hold_sum(what, family, y, ref, bound, dtype):
    y = y.reshape(-1)
    if family == "exact":
        assert torch.equal(y, ref.to(dtype)), (what, (y.double() - ref).abs().max())
    else:
        assert bool(torch.isfinite(y).all()) and bool(((y.double() - ref).abs() <= bound).all()), \
            (what, float(((y.double() - ref).abs() / bound.clamp(min=1e-300)).max()))


@pytest.mark.parametrize("n", R.ATOM_SUM_N)
@pytest.mark.parametrize("n_mol", [1, 37])
def test_atom_sum_forward(n, n_mol):
    """k_atom_sum up to 4096 atoms, k_atom_runs above: sorted, shuffled, with empty molecules, with ids outside
    [0, n_mol), both families, both types.  No atoms: ``mean`` everywhere."""
    for kind in R.kinds_for(n_mol):
        assert (n, n_mol, kind) in R.ATOM_SUM_CASES
        for dtype in (F32, F64):
            for family in ("exact", "random"):
                x, batch, std, mean = R.atom_case(family, n, n_mol, kind, dtype)
                y = _atom_sum(x, batch, n_mol, std, mean, dtype)
                ref = R.atom_sum(x, batch, n_mol, std, mean)
                _hold_sum(f"atom_sum n={n} n_mol={n_mol} {kind} {family} {dtype}", family, y, ref,
                          R.sum_bound(x, None, None, batch, n_mol, std, mean, dtype), dtype)
                if n == 0:
                    assert bool((y == mean.to(dtype)).all())


@DTYPES
@pytest.mark.parametrize("n", [1000, 4097])
def test_atom_sum_without_std_or_mean(n, dtype):
    for family in ("exact", "random"):
        x, batch, std, mean = R.atom_case(family, n, 37, "range", dtype)
        for s, m in ((None, mean), (std, None), (None, None)):
            y = _atom_sum(x, batch, 37, s, m, dtype)
            _hold_sum(f"atom_sum n={n} std {s} mean {m}", family, y, R.atom_sum(x, batch, 37, s, m),
                      R.sum_bound(x, None, None, batch, 37, s, m, dtype), dtype)


@DTYPES
def test_molecule_ceiling(dtype):
    """8192 molecules, every one non-empty (the fp64 bins are the whole 64 KiB of static LDS), in each of the three
    kernels that keep bins; 8193: TMDNET_BAD_ARGUMENT and y untouched."""
    n, n_mol, kind = R.CEILING_CASE
    assert n_mol == kernels.ATOM_SUM_MAX_MOLECULES == R.MAX_MOLECULES
    x, batch, std, mean = R.atom_case("exact", n, n_mol, kind, dtype)
    assert not R.has_empty(batch, n_mol)
    ref = R.atom_sum(x, batch, n_mol, std, mean)
    assert torch.equal(_atom_sum(x, batch, n_mol, std, mean, dtype), ref.to(dtype))  # k_atom_runs
    few = 4000  # k_atom_sum: at most 4096 atoms, spread over the whole range of bins
    xs, bs = x[:few], (torch.arange(few) * 8191 // (few - 1))
    assert int(bs.max()) == n_mol - 1
    assert torch.equal(_atom_sum(xs, bs, n_mol, std, mean, dtype), R.atom_sum(xs, bs, n_mol, std, mean).to(dtype))
    h, w, b0, _, _, _ = R.dot_case("exact", few, 5, n_mol, "sorted", dtype)
    y, _ = _dot_sum(h, w, b0, bs, n_mol, std, mean, dtype, with_buf=False)  # k_dot_sum
    assert torch.equal(y, R.dot_sum(h, w, b0, bs, n_mol, std, mean).to(dtype))
    _atom_sum(x, batch, n_mol + 1, std, mean, dtype, expect=BAD_ARGUMENT)
    hd, wd, bd, yd = *_dev(h, w, bs), _sent(n_mol + 1, dtype=dtype)
    rc = nat.load().tmdnet_dot_sum_fwd(nat.dtype_code(dtype), few, 5, nat.ptr(hd), 5, nat.ptr(wd), None, n_mol + 1,
                                       nat.ptr(bd), None, None, None, nat.ptr(yd), _st())
    assert rc == BAD_ARGUMENT and _untouched(yd)


@DTYPES
@pytest.mark.parametrize("n", R.SUM_BWD_N)
def test_sum_backwards(n, dtype):
    """gx[n] = std gy[batch[n]] and gh[n, k] = std gy[batch[n]] w[k]: one product chain each, so bit-equal to the
    same chain in the kernel's type; rows with an id outside [0, n_mol): exact zeros."""
    n_mol, K = 37, 5
    lib, code = nat.load(), nat.dtype_code(dtype)
    g = torch.Generator().manual_seed(n)
    gy = torch.randn(n_mol, generator=g, dtype=dtype)
    w = torch.randn(K, generator=g, dtype=dtype)
    std = torch.tensor([1.7], dtype=dtype)
    for kind in R.BATCH_KINDS:
        assert (n, n_mol, kind) in R.SUM_BWD_CASES
        batch = R.make_batch(kind, n, n_mol)
        on = (batch >= 0) & (batch < n_mol)
        a = torch.zeros(n, dtype=dtype)
        a[on] = std * gy[batch[on]]
        bd, gd, wd, sd = _dev(batch, gy, w, std)
        for s, scale in ((sd, a), (None, torch.where(on, gy[batch.clamp(0, n_mol - 1)], torch.zeros_like(a)))):
            gx, gh = _sent(n + 3, dtype=dtype), _sent(n * K + 3, dtype=dtype)
            assert lib.tmdnet_atom_sum_bwd(code, n, n_mol, nat.ptr(gd), nat.ptr(bd), nat.ptr(s), nat.ptr(gx),
                                           _st()) == 0
            assert lib.tmdnet_dot_sum_bwd(code, n, K, nat.ptr(gd), nat.ptr(bd), n_mol, nat.ptr(s), nat.ptr(wd),
                                          nat.ptr(gh), _st()) == 0
            assert _untouched(gx[n:], gh[n * K:])
            gx, gh = gx[:n].cpu(), gh[:n * K].cpu().reshape(n, K)
            assert torch.equal(gx, scale) and torch.equal(gh, scale[:, None] * w[None, :]), (kind, s is None)
            assert not bool(gx[~on].any()) and not bool(gh[~on].any())
            ref = R.dot_sum_bwd(gy, batch, n_mol, None if s is None else std, w)
            assert bool(((gh.double() - ref).abs() <= 2 * R.U[dtype] * ref.abs()).all())


@DTYPES
@pytest.mark.parametrize("K", R.DOT_K)
def test_dot_sum_forward(K, dtype):
    """k_dot_sum strides K by 64 lanes, k_row_dot by 16: K around both, 203 atoms in 9 molecules (some empty, or
    ids out of range).  With atom_buf (row products over the grid, then k_atom_runs) and without (one workgroup);
    rows of h padded by 4 sentinel columns; NULL b0; atom_buf holds h . w + b0."""
    (n, _, n_mol, kind), = [c for c in R.DOT_CASES if c[1] == K]
    for family in ("exact", "random"):
        h, w, b0, batch, std, mean = R.dot_case(family, n, K, n_mol, kind, dtype)
        for bias, pad in ((b0, 0), (b0, 4), (None, 4)):
            ref = R.dot_sum(h, w, bias, batch, n_mol, std, mean)
            bound = R.sum_bound(h, w, bias, batch, n_mol, std, mean, dtype)
            what = f"dot_sum K={K} {family} {dtype} pad {pad} b0 {bias is not None}"
            ys = []
            for with_buf in (False, True):
                y, buf = _dot_sum(h, w, bias, batch, n_mol, std, mean, dtype, with_buf, pad)
                _hold_sum(f"{what} atom_buf {with_buf}", family, y, ref, bound, dtype)
                ys.append(y)
                if buf is not None:
                    rows = R.dot_rows(h, w, bias)
                    if family == "exact":
                        assert torch.equal(buf, rows.to(dtype)), what
                    else:
                        mag = h.double().abs() @ w.double().abs() + (0 if bias is None else abs(float(bias)))
                        assert bool(((buf.double() - rows).abs() <= (K + 1) * R.U[dtype] * mag).all()), what
            assert family != "exact" or torch.equal(*ys)


@DTYPES
@pytest.mark.parametrize("n,K,n_mol,kind", R.DOT_ROUTE, ids=[f"n{c[0]}-{c[3]}" for c in R.DOT_ROUTE])
def test_dot_sum_route_switch(n, K, n_mol, kind, dtype, monkeypatch):
    """kernels.dot_sum hands the library an atom buffer above 4096 atoms and none up to there."""
    lib = nat.load()
    seen = []
    orig = lib.tmdnet_dot_sum_fwd
    monkeypatch.setattr(lib, "tmdnet_dot_sum_fwd", lambda *a: seen.append(a[11] is not None) or orig(*a))
    for family in ("exact", "random"):
        h, w, b0, batch, std, mean = R.dot_case(family, n, K, n_mol, kind, dtype)
        with torch.no_grad():
            y = kernels.dot_sum(*_dev(h, w, b0, batch), n_mol, *_dev(std, mean))
        assert y.shape == (n_mol, 1)
        _hold_sum(f"kernels.dot_sum n={n} {kind} {family} {dtype}", family, y.cpu(),
                  R.dot_sum(h, w, b0, batch, n_mol, std, mean),
                  R.sum_bound(h, w, b0, batch, n_mol, std, mean, dtype), dtype)
    assert seen == [n > 4096] * 2


@DTYPES
def test_sums_first_order_through_the_wrappers(dtype):
    """kernels.atom_sum and kernels.dot_sum at 4097 unsorted atoms: the outputs and the gradients of (x | h, w, b0)
    against float64 autograd of the restatement's arithmetic.  (Ids in range: the wrapper forms the weight
    gradient's per-atom seed with index_select, which takes no others.)"""
    n, n_mol, K = 4097, 37, 17
    h, w, b0, batch, std, mean = R.dot_case("random", n, K, n_mol, "shuffled", dtype)
    gy = torch.randn(n_mol, 1, generator=torch.Generator().manual_seed(2), dtype=dtype)
    on = ((batch >= 0) & (batch < n_mol)).double()
    safe = batch.clamp(0, n_mol - 1)

    def ref_sum(rows):  # the restatement with its graph kept
        return torch.zeros(n_mol, dtype=F64).index_add(0, safe, rows * on) * float(std) + float(mean)

    u = R.U[dtype]
    hs, ws, bs = (t.double().requires_grad_(True) for t in (h, w, b0))
    yr = ref_sum(hs @ ws + bs)
    assert torch.equal(yr.detach(), R.dot_sum(h, w, b0, batch, n_mol, std, mean))
    ref = torch.autograd.grad(yr, (hs, ws, bs), gy.double().reshape(-1))
    hd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (h, w, b0))
    y = kernels.dot_sum(hd, wd, bd, batch.to(DEV), n_mol, *_dev(std, mean))
    _hold_sum("kernels.dot_sum", "random", y.detach().cpu(), yr.detach(),
              R.sum_bound(h, w, b0, batch, n_mol, std, mean, dtype), dtype)
    gh, gw, gb = torch.autograd.grad(y, (hd, wd, bd), gy.to(DEV))
    assert bool(((gh.cpu().double() - ref[0]).abs() <= 2 * u * ref[0].abs()).all())  # a product chain
    # gw[k] = sum_n a_n h_nk and gb = sum_n a_n, a_n = std gy[batch[n]]: n-term sums of float32-rounded products
    a = (float(std) * gy.double().reshape(-1)[safe] * on).abs()
    assert bool(((gw.cpu().double() - ref[1]).abs() <= (n + 4) * u * (a @ h.double().abs())).all())
    assert abs(float(gb.cpu().double().reshape(-1)[0] - ref[2].reshape(-1)[0])) <= (n + 4) * u * float(a.sum())

    xs = h[:, 0].double().requires_grad_(True)
    yr = ref_sum(xs)
    gr, = torch.autograd.grad(yr, xs, gy.double().reshape(-1))
    xd = h[:, :1].contiguous().to(DEV).requires_grad_(True)
    y = kernels.atom_sum(xd, batch.to(DEV), n_mol, *_dev(std, mean))
    _hold_sum("kernels.atom_sum", "random", y.detach().cpu(), yr.detach(),
              R.sum_bound(h[:, 0], None, None, batch, n_mol, std, mean, dtype), dtype)
    gx, = torch.autograd.grad(y, xd, gy.to(DEV))
    assert bool(((gx.cpu().double().reshape(-1) - gr).abs() <= u * gr.abs()).all())
    assert not bool(gx.cpu().reshape(-1)[on == 0].any())


# ----------------------------------------------------------------------------- loss
W1, W2, GOUT = 0.75, 1.25, 3.0  # float32 values: the kernel's (T)w is the weight itself


def _mse2_fwd(a1, b1, a2, b2, dtype):
    ts = _dev(a1, b1, a2, b2)
    out = _sent(4, dtype=dtype)
    rc = nat.load().tmdnet_mse2_fwd(nat.dtype_code(dtype), a1.numel(), nat.ptr(ts[0]) if a1.numel() else None,
                                    nat.ptr(ts[1]) if a1.numel() else None, W1, a2.numel(),
                                    nat.ptr(ts[2]) if a2.numel() else None, nat.ptr(ts[3]) if a2.numel() else None,
                                    W2, nat.ptr(out), _st())
    assert rc == 0 and _untouched(out[1:])
    return float(out[0])


@DTYPES
@pytest.mark.parametrize("n1,n2", R.LOSS_PAIRS)
def test_mse2_forward(n1, n2, dtype):
    for family in ("exact", "random"):
        a1, b1, a2, b2 = R.loss_inputs(family, n1, n2, dtype)
        got = _mse2_fwd(a1, b1, a2, b2, dtype)
        ref, scale = R.mse2(a1, b1, W1, a2, b2, W2), R.mse2_scale(a1, b1, W1, a2, b2, W2)
        bound = R.mse2_bound(family, n1, n2, dtype)
        print(f"mse2 ({n1}, {n2}) {family}: {got!r} ref {ref!r} bound {bound * scale:.3e}")
        assert abs(got - ref) <= bound * scale
        if n1 == 0 and n2 == 0:
            assert got == 0.0


@DTYPES
@pytest.mark.parametrize("n1,n2", R.LOSS_PAIRS)
def test_mse2_backward(n1, n2, dtype):
    """d = g w 2 (a - b) / n with g = 3 read on the device: four operations, 4 u relative per element, over the
    full length of each side whichever is longer; d1 or d2 NULL leaves the other right; what lies beside them
    is not touched."""
    a1, b1, a2, b2 = R.loss_inputs("random", n1, n2, dtype)
    ts = _dev(a1, b1, a2, b2)
    ptrs = [nat.ptr(t) if t.numel() else None for t in ts]
    g = torch.tensor([GOUT], dtype=dtype, device=DEV)
    refs = R.mse2_bwd(a1, b1, W1, a2, b2, W2, GOUT)
    first = None
    for want in ((True, True), (False, True), (True, False)):
        d = [_sent(n1 + 3, dtype=dtype), _sent(n2 + 3, dtype=dtype)]
        rc = nat.load().tmdnet_mse2_bwd(nat.dtype_code(dtype), n1, ptrs[0], ptrs[1], W1, n2, ptrs[2], ptrs[3], W2,
                                        nat.ptr(g), nat.ptr(d[0]) if want[0] else None,
                                        nat.ptr(d[1]) if want[1] else None, _st())
        assert rc == 0
        for t, n, on, ref in zip(d, (n1, n2), want, refs):
            if not on:
                assert _untouched(t)
                continue
            assert _untouched(t[n:])
            err = (t[:n].cpu().double() - ref).abs()
            assert bool((err <= 4 * R.U[dtype] * ref.abs()).all()), (n1, n2, want)
        if first is None:
            first = d
        else:
            assert all(torch.equal(t, f) for t, f, on in zip(d, first, want) if on)


@DTYPES
def test_mse2_one_sided_through_the_wrapper(dtype):
    """kernels.mse2 with an empty side: the other side's loss and gradient (F.mse_loss of nothing is NaN)."""
    a, b, _, _ = R.loss_inputs("random", 7, 0, dtype)
    e = torch.zeros(0, dtype=dtype)
    for sides, ref, gref in (((a, b, e, e), W1 * R.mse(a, b), R.mse2_bwd(a, b, W1, e, e, W2, 1.0)[0]),
                             ((e, e, a, b), W2 * R.mse(a, b), R.mse2_bwd(e, e, W1, a, b, W2, 1.0)[1])):
        a1, b1, a2, b2 = _dev(*sides)
        a1.requires_grad_(True)
        a2.requires_grad_(True)
        loss = kernels.mse2(a1, b1, a2, b2, W1, W2)
        assert abs(float(loss.detach()) - ref) <= R.mse2_bound("random", 7, 0, dtype) * abs(ref)
        loss.backward()
        full, none = (a1, a2) if a1.numel() else (a2, a1)
        assert bool(((full.grad.cpu().double() - gref).abs() <= 4 * R.U[dtype] * gref.abs()).all())
        assert none.grad is None or none.grad.numel() == 0


def test_layer_norm_ratios_are_reported():
    """Last in the file: the worst err_hip / err_aten of each LayerNorm group over the cases that ran."""
    for group, (ratio, what) in sorted(RATIOS.items()):
        print(f"worst err_hip / err_aten, {group}: {ratio:.2f} at {what} (MARGIN {MARGIN:g})")
        assert ratio <= 8, (group, what)

