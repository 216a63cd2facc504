"""The scalar form of the ET message entry points (csrc/t_message.hip, TMDNET_ET_SCALAR: the invariant
Transformer's message) against ``kernels.t_message_composite`` in fp64 on the same inputs (the fp32 inputs upcast),
gradients by ``torch.autograd.grad``.

The kernels compile one code path per lane width V (first order H / 32 in {1, 2, 4, 8}, V = 1 below H = 32; second
order H / 64 from H = 64) and per activation form (SiLU / SiLU as constants, or the codes read at run time); the
head width in lanes lph = d / V and the lanes per edge L = H / V are run-time values.  One wave owns a destination
at every node count, so there is one launch form per entry point and no node-count switch.  The widths below hit
(V, lph) = (1, 4), (1, 32), (1, 4), (2, 4), (4, 4), (4, 2), (8, 4), (8, 32) in the first order and (1, 4), (1, 32),
(1, 4), (1, 8), (2, 8), (2, 4), (4, 8), (4, 64) in the second; the activation test runs the run-time form.

Graphs: test_gpu_et_widths' cliques of 1, 2, 3, 9, 17, 63, 64, 65 and 130 atoms, every atom with its self loop,
shuffled (rows of one slot, a partial step, exactly one chunk of 64, one chunk and one edge, two chunks and two
edges); and an explicit list with an empty row and a self loop, plain and with 5 static-capacity padding slots.

Bars are test_gpu_et_widths': fp64 1e-12 forward, 1e-11 first order, 1e-10 second order (max abs error over max
abs value, per tensor); fp32, per tensor, e_k <= 2 e_c + 4 * 2**-24 * scale with e_c the error of the composite
run in fp32 on the GPU.  Every figure is printed (``pytest -s``) before anything is asserted.

Per-edge inputs are pair-symmetric as in a model (pk, pv, C equal on an edge and its reverse); the upstream
gradient and every second-order cotangent are drawn per directed edge.
"""
import pytest
import torch

import test_gpu_et_widths as W
from torchmdnet import _native as nat
from torchmdnet import kernels
from torchmdnet._native import ET_SCALAR
from torchmdnet.kernels import EdgeGraph, et_act_flags, t_message, t_message_composite

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
WIDTHS = [(16, 4), (32, 1), (32, 8), (64, 8), (128, 8), (128, 16), (256, 8), (256, 1)]
LEAVES = ("q", "k", "v", "pk", "pv", "C")
BAD_ARGUMENT, UNSUPPORTED = 1, 2


def _report():
    return W._Report("t-message")


# ----------------------------------------------------------------------------- graphs, inputs, reference
def _explicit(pad):
    """8 atoms: the path 0-1-2-3 with the chord 1-3, self loops on 0 and 2 only, atom 4 with its self loop alone,
    the bond 5-6 without self loops, and atom 7 without any edge (an empty row).  ``pad``: static-capacity slots
    (-1) appended."""
    und = [(0, 1), (1, 2), (2, 3), (1, 3), (5, 6)]
    loops = [0, 2, 4]
    ei = torch.tensor([[a for a, b in und] + [b for a, b in und] + loops,
                       [b for a, b in und] + [a for a, b in und] + loops], device=DEV)
    g, _ = EdgeGraph.from_edge_index(ei, 8)
    assert g.symmetric and int(g.row_ptr[8] - g.row_ptr[7]) == 0
    if pad:
        fill = torch.full((pad,), -1, dtype=torch.int32, device=DEV)
        g = EdgeGraph(8, g.row_ptr, torch.cat([g.src, fill]), torch.cat([g.dst, fill]),
                      torch.cat([g.transpose, fill]), None, None, g.num_pairs, True, static=True)
    return g


def _live(graph):
    return int(graph.row_ptr[graph.n_nodes])


def _inputs(graph, H, dtype, seed, has=(True, True), strided=False, qscale=1.0):
    """Node rows, pair-symmetric per-edge rows (an edge and its reverse share a row; padding slots random), the
    upstream gradient gx.  ``strided``: pk | pv as column blocks of one [E, 2H] buffer.  ``qscale`` scales q."""
    N, E, n = graph.n_nodes, graph.n_edges, _live(graph)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    T = graph.transpose.long().cpu()
    rep = torch.arange(E)
    rep[:n] = torch.minimum(rep[:n], T[:n])  # the pair's representative edge
    I = dict(q=qscale * rn(N, H), k=rn(N, H), v=rn(N, H), gx=rn(N, H))
    pkv = rn(E, 2 * H)[rep]
    I["C"] = torch.rand(E, generator=g, dtype=F64)[rep]
    I = {k: t.to(dtype).to(DEV) for k, t in I.items()}
    pkv = pkv.to(dtype).to(DEV)
    if strided:
        I["pkv"] = pkv  # the leaf whose column blocks pk / pv are
        pk, pv = pkv[:, :H], pkv[:, H:]
    else:
        pk, pv = pkv[:, :H].contiguous(), pkv[:, H:].contiguous()
    I["pk"], I["pv"] = (pk if has[0] else None), (pv if has[1] else None)
    return I


def _cotangents(graph, H, I, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for nm in LEAVES:
        out.append(None if I[nm] is None else torch.randn(*I[nm].shape, generator=g, dtype=F64).to(DEV))
    return out


def _two_orders(fn, I, ggs, dtype):
    """(out, first-order gradients, second-order gradients w.r.t. gx + leaves) of ``fn`` in ``dtype``; absent
    operands give no entry.  With I["pkv"] the leaf is the [E, 2H] buffer and ``fn`` gets its column blocks."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    xs = {k: (None if I[k] is None else leaf(I[k])) for k in ("gx",) + LEAVES}
    H = I["q"].shape[1]
    both = I.get("pkv") is not None
    if both:
        pkv = leaf(I["pkv"])
        xs["pk"], xs["pv"] = pkv[:, :H], pkv[:, H:]
    out = fn(*(xs[k] for k in LEAVES))
    gg = dict(zip(LEAVES, ggs))
    if both:
        names = ["q", "k", "v", "pkv", "C"]
        xs["pkv"], gg["pkv"] = pkv, torch.cat([gg["pk"], gg["pv"]], 1)
    else:
        names = [k for k in LEAVES if xs[k] is not None]
    first = torch.autograd.grad(out, [xs[k] for k in names], xs["gx"], create_graph=True)
    wrt = ["gx"] + names
    second = torch.autograd.grad(first, [xs[k] for k in wrt], [gg[k].to(dtype) for k in names])
    f = dict(zip(names, (t.detach() for t in first)))
    s = dict(zip(wrt, second))
    for r in (f, s):
        if both:
            t = r.pop("pkv")
            r["pk"], r["pv"] = t[:, :H], t[:, H:]
    return out.detach(), f, s


def _against_composite(rep, tag, graph, heads, I, ggs, acts=0):
    src, dst, N = graph.src.long(), graph.dst.long(), graph.n_nodes
    comp = lambda *a: t_message_composite(*a, src, dst, N, heads, acts)  # noqa: E731
    hip = lambda *a: t_message(*a, graph, heads, acts)  # noqa: E731
    dtype = I["q"].dtype
    ref = _two_orders(comp, I, ggs, F64)
    c32 = _two_orders(comp, I, ggs, F32) if dtype == F32 else None
    got = _two_orders(hip, I, ggs, dtype)
    torch.cuda.synchronize()
    n = _live(graph)
    rep.check(f"{tag} out", got[0], ref[0], None if c32 is None else c32[0], 1e-12)
    for k in ref[1]:
        rep.check(f"{tag} order 1 g_{k}", got[1][k], ref[1][k], None if c32 is None else c32[1][k], 1e-11)
        if k in ("pk", "pv", "C"):
            rep.require(bool((got[1][k][n:] == 0).all()), f"{tag} g_{k}: padding rows not zero")
    for k in ref[2]:
        rep.check(f"{tag} order 2 d_{k}", got[2][k], ref[2][k], None if c32 is None else c32[2][k], 1e-10)
        if k in ("pk", "pv", "C"):
            rep.require(bool((got[2][k][n:] == 0).all()), f"{tag} d_{k}: padding rows not zero")


# ----------------------------------------------------------------------------- 1. widths
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H,heads", WIDTHS, ids=[f"H{h}x{n}" for h, n in WIDTHS])
def test_widths(H, heads, dtype):
    """Forward, first and second order at every lane width and head width, rows of 1 to 130 edges, pk | pv as
    column blocks of one [E, 2H] buffer."""
    graph = W._graph("reduced")
    I = _inputs(graph, H, dtype, 41, strided=True)
    rep = _report()
    _against_composite(rep, f"H{H}x{heads}", graph, heads, I, _cotangents(graph, H, I, 42))
    rep.done()


# ----------------------------------------------------------------------------- 2. operand combinations
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("has", [(True, False), (False, True), (False, False), (True, True)],
                         ids=["pk", "pv", "neither", "both-dense"])
def test_operand_combinations(has, dtype):
    graph = W._graph("reduced")
    I = _inputs(graph, 64, dtype, 43, has=has)
    rep = _report()
    _against_composite(rep, f"pk{int(has[0])}pv{int(has[1])}", graph, 8, I, _cotangents(graph, 64, I, 44))
    rep.done()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kv,at", [(0, 1), (1, 2), (2, 3), (3, 0)], ids=["silu-ssp", "ssp-tanh", "tanh-sigmoid",
                                                                         "sigmoid-silu"])
def test_activation_codes(kv, at, dtype):
    """All four codes in each role, H = 128: the kernels' run-time activation form.  q is scaled by 1/4, which
    keeps every attention pre-activation below 20: past it F.softplus is the identity with derivative exactly 1,
    while the kernels (common.h ActF, shared with the vector form) keep sigmoid(x) = 1 - 2e-9 -- a difference of
    definition above the fp64 bars, not an error of either side."""
    graph = W._graph("reduced")
    I = _inputs(graph, 128, dtype, 45, strided=True, qscale=0.25)
    rep = _report()
    _against_composite(rep, f"act{kv}{at}", graph, 8, I, _cotangents(graph, 128, I, 46), acts=et_act_flags(kv, at))
    rep.done()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("pad", [0, 5], ids=["plain", "padded"])
def test_explicit_list(pad, dtype):
    """An EdgeGraph.from_edge_index list with an empty row, atoms without a self loop and self-loop-only atoms;
    with 5 padding slots their per-edge gradient rows are exactly zero (checked in _against_composite)."""
    graph = _explicit(pad)
    I = _inputs(graph, 32, dtype, 47, strided=True)
    rep = _report()
    _against_composite(rep, f"explicit pad{pad}", graph, 4, I, _cotangents(graph, 32, I, 48))
    out = t_message(I["q"], I["k"], I["v"], I["pk"], I["pv"], I["C"], graph, 4)
    rep.require(bool((out[7] == 0).all()), "empty row not zero")
    rep.done()


def test_asymmetric_graph_raises():
    ei = torch.tensor([[0, 1, 2], [1, 0, 0]], device=DEV)  # 2 -> 0 has no reverse
    g, _ = EdgeGraph.from_edge_index(ei, 3)
    assert not g.symmetric
    q = torch.randn(3, 32, device=DEV, requires_grad=True)
    C = torch.rand(3, device=DEV)
    with pytest.raises(RuntimeError, match="symmetric"):
        t_message(q, q, q, None, None, C, g, 4)
    with torch.no_grad():  # the forward alone needs no reverse edges
        out = t_message(q, q, q, None, None, C, g, 4)
    ref = t_message_composite(q.detach(), q.detach(), q.detach(), None, None, C, g.src.long(), g.dst.long(), 3, 4)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------- raw calls
FWD = ("dtype n_nodes hidden heads row_ptr src max_pairs q ld_q k ld_k v ld_v vec_in pk ld_pk pv ld_pv cutoff unit "
       "x_out vec_out flags pk_rows order stream").split()
BWD = ("dtype n_nodes hidden heads row_ptr src max_pairs q ld_q k ld_k v ld_v vec_in pk ld_pk pv ld_pv cutoff unit "
       "grad_x grad_vec gq gk gv gvec_in gpk gpv gcut gunit dpk dpv gdist accumulate pk_rows order stream").split()
BWD2 = ("dtype n_nodes hidden heads row_ptr src transpose max_pairs q ld_q k ld_k v ld_v vec_in pk ld_pk pv ld_pv "
        "cutoff unit grad_x grad_vec gg_q ld_ggq gg_k ld_ggk gg_v ld_ggv gg_vec gg_pk ld_ggpk gg_pv ld_ggpv gg_cut "
        "gg_unit d_grad_x d_grad_vec d_q ld_dq d_k ld_dk d_v ld_dv d_vec d_pk ld_dpk d_pv ld_dpv d_cut d_unit "
        "edge_scratch pk_rows gg_pkv_scale flags stream").split()
ENTRY = {"fwd": ("tmdnet_et_message_fwd", FWD, "flags"), "bwd": ("tmdnet_et_message_bwd", BWD, "accumulate"),
         "bwd2": ("tmdnet_et_message_bwd2", BWD2, "flags")}


def _base(graph, heads, I):
    N, H = I["q"].shape
    a = dict(dtype=nat.dtype_code(I["q"].dtype), n_nodes=N, hidden=H, heads=heads, row_ptr=graph.row_ptr,
             src=graph.src, max_pairs=graph.n_edges, cutoff=I["C"], stream=nat.stream(I["q"].device))
    for nm in ("q", "k", "v", "pk", "pv"):
        a[nm] = I[nm]
        a["ld_" + nm] = 0 if I[nm] is None else I[nm].stride(0)
    return a


def _call(which, args, bits=0):
    """The entry point with the named arguments (tensors by pointer; everything unnamed NULL / 0) and the scalar
    bit.  Returns the status code."""
    name, names, flagname = ENTRY[which]
    args = dict(args)
    args[flagname] = int(args.get(flagname, 0)) | ET_SCALAR | bits
    vals = []
    for nm in names:
        v = args.pop(nm, None)
        if nm.startswith("ld_") or nm in ("dtype", "n_nodes", "hidden", "heads", "max_pairs", "flags", "accumulate"):
            vals.append(int(v or 0))
        elif nm == "stream":
            vals.append(v)
        else:
            vals.append(nat.ptr(v))
    assert not args, f"unknown arguments {sorted(args)}"
    rc = getattr(nat.load(), name)(*vals)
    torch.cuda.synchronize()
    return int(rc)


def _outputs(which, graph, I, fill):
    """Every output of the entry point, filled with ``fill``."""
    N, H = I["q"].shape
    E, o = graph.n_edges, dict(dtype=I["q"].dtype, device=DEV)
    node, edge, cut = (lambda: torch.full((N, H), fill, **o)), (lambda: torch.full((E, H), fill, **o)), \
        (lambda: torch.full((E,), fill, **o))
    if which == "fwd":
        return dict(x_out=node())
    if which == "bwd":
        # the first backward writes gpk / gpv with the row stride of pk / pv: buffers of that stride
        like = lambda t: torch.full((E, t.stride(0)), fill, **o)[:, :H]  # noqa: E731
        return dict(gq=node(), gk=node(), gv=node(), gpk=like(I["pk"]), gpv=like(I["pv"]), gcut=cut())
    return dict(d_grad_x=node(), d_q=node(), d_k=node(), d_v=node(), d_pk=edge(), d_pv=edge(), d_cut=cut())


def _full_args(which, graph, heads, I, outs, ggs=None):
    a = _base(graph, heads, I)
    a.update(outs)
    if which != "fwd":
        a["grad_x"] = I["gx"]
    if which == "bwd2":
        a["transpose"] = graph.transpose
        for nm, g in zip(("gg_q", "gg_k", "gg_v", "gg_pk", "gg_pv", "gg_cut"), ggs):
            a[nm] = g
    return a


# ----------------------------------------------------------------------------- 3. order
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_order_gives_identical_bits(dtype):
    graph = W._graph("reduced")
    I = _inputs(graph, 128, dtype, 49, strided=True)
    order = torch.arange(graph.n_nodes - 1, -1, -1, dtype=torch.int32, device=DEV)
    for which in ("fwd", "bwd"):
        plain, perm = _outputs(which, graph, I, float("nan")), _outputs(which, graph, I, float("nan"))
        assert _call(which, _full_args(which, graph, 8, I, plain)) == 0
        assert _call(which, dict(_full_args(which, graph, 8, I, perm), order=order)) == 0
        for k in plain:
            assert not bool(torch.isnan(plain[k]).any()), (which, k)
            assert torch.equal(plain[k], perm[k]), (which, k)


# ----------------------------------------------------------------------------- 4. refusals
SENTINEL = 7.5
ABSENT = {"fwd": ["vec_in", "unit", "vec_out", "pk_rows"],
          "bwd": ["vec_in", "unit", "grad_vec", "gvec_in", "gunit", "dpk", "dpv", "gdist", "pk_rows"],
          "bwd2": ["vec_in", "unit", "grad_vec", "gg_vec", "gg_unit", "d_grad_vec", "d_vec", "d_unit", "pk_rows",
                   "gg_pkv_scale"]}
BITS = {"fwd": [nat.ET_V_PLANAR, nat.ET_PREACT],
        "bwd": [nat.ACC_VEC_RESIDUAL, nat.ACC_EDGE, nat.ET_V_PLANAR, nat.ACC_GRADS, nat.ET_TWO_PASS, nat.ET_PREACT],
        "bwd2": [nat.ET_V_PLANAR, nat.BWD2_ACC_EDGE, nat.BWD2_ACC_GVEC]}


def _refused(which, graph, heads, I, ggs, want, **change):
    outs = _outputs(which, graph, I, SENTINEL)
    bits = change.pop("bits", 0)
    args = _full_args(which, graph, heads, I, outs, ggs)
    args.update(change)
    rc = _call(which, args, bits)
    assert rc == want, (which, sorted(change), bits, rc)
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), (which, sorted(change), bits, k)


@pytest.mark.parametrize("which", ["fwd", "bwd", "bwd2"])
def test_vector_form_operands_are_refused(which):
    """Every operand and bit of the vector form gives BAD_ARGUMENT with nothing launched: the outputs keep their
    sentinel."""
    graph = W._graph("tiny")
    I = _inputs(graph, 32, F32, 51)
    ggs = _cotangents(graph, 32, I, 52)
    ggs = [g.float() for g in ggs]
    N, E = graph.n_nodes, graph.n_edges
    # the plain call is accepted (the sentinel is overwritten)
    outs = _outputs(which, graph, I, SENTINEL)
    assert _call(which, _full_args(which, graph, 4, I, outs, ggs)) == 0
    assert all(not bool((t == SENTINEL).any()) for t in outs.values())
    for nm in ABSENT[which]:
        if nm == "pk_rows":
            extra = torch.arange(E, dtype=torch.int32, device=DEV)
        else:
            extra = torch.zeros(max(N, E) * 3 * 32, dtype=F32, device=DEV)
        _refused(which, graph, 4, I, ggs, BAD_ARGUMENT, **{nm: extra})
    for bit in BITS[which]:
        _refused(which, graph, 4, I, ggs, BAD_ARGUMENT, bits=bit)


@pytest.mark.parametrize("which", ["fwd", "bwd", "bwd2"])
@pytest.mark.parametrize("H,heads", [(96, 8), (128, 64)], ids=["H96x8", "H128x64"])
def test_widths_outside_the_envelope_are_unsupported(H, heads, which):
    graph = W._graph("tiny")
    I = _inputs(graph, H, F32, 53)
    ggs = [g.float() for g in _cotangents(graph, H, I, 54)]
    _refused(which, graph, heads, I, ggs, UNSUPPORTED)


def test_second_order_needs_the_transpose():
    graph = W._graph("tiny")
    I = _inputs(graph, 32, F32, 55)
    ggs = [g.float() for g in _cotangents(graph, 32, I, 56)]
    _refused("bwd2", graph, 4, I, ggs, UNSUPPORTED, transpose=None)


# ----------------------------------------------------------------------------- 5. the vector form
def test_same_results_as_the_vector_form():
    """(64, 8), fp64: the ET entry points without the bit on v / pv widened to 3H with zero v1 | v2 blocks, vec_in
    NULL and unit zeros.  x_out, gq, gk, gpk and gcut agree with the scalar form's to 1e-12."""
    H, heads, d = 64, 8, 8
    graph = W._graph("reduced")
    I = _inputs(graph, H, F64, 57)
    N, E = graph.n_nodes, graph.n_edges

    def widen(t):
        w = torch.zeros(t.shape[0], heads, 3, d, dtype=F64, device=DEV)
        w[:, :, 0, :] = t.view(-1, heads, d)
        return w.view(t.shape[0], 3 * H)

    v3, pv3 = widen(I["v"]), widen(I["pv"])
    u = torch.zeros(E, 3, dtype=F64, device=DEV)
    o = dict(dtype=F64, device=DEV)
    xo, vo = torch.empty(N, H, **o), torch.empty(N, 3, H, **o)
    kernels.et_message_fwd_launch(I["q"], I["k"], v3, None, I["pk"], pv3, I["C"], u, graph, heads, xo, vo)
    gq, gk, gv3 = torch.empty(N, H, **o), torch.empty(N, H, **o), torch.empty(N, 3 * H, **o)
    gpk, gpv3, gC, gu = torch.empty(E, H, **o), torch.empty(E, 3 * H, **o), torch.empty(E, **o), torch.empty(E, 3, **o)
    kernels.et_message_bwd_launch(I["q"], I["k"], v3, None, I["pk"], pv3, I["C"], u, graph, heads, I["gx"],
                                  torch.zeros(N, 3, H, **o), gq, gk, gv3, None, gpk, gpv3, gC, gu)
    f = _outputs("fwd", graph, I, float("nan"))
    b = _outputs("bwd", graph, I, float("nan"))
    assert _call("fwd", _full_args("fwd", graph, heads, I, f)) == 0
    assert _call("bwd", _full_args("bwd", graph, heads, I, b)) == 0
    rep = _report()
    for name, got, ref in (("x_out", f["x_out"], xo), ("gq", b["gq"], gq), ("gk", b["gk"], gk),
                           ("gpk", b["gpk"], gpk), ("gcut", b["gcut"], gC)):
        rep.check("vector form " + name, got, ref, None, 1e-12)
    rep.done()
