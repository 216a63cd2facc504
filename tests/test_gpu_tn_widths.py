"""The TensorNet edge kernels (csrc/tn_message.hip) across channel widths H, against their composites in fp64.

The kernels compile one code path per width form -- nblk = ceil(H / 64) channel blocks, the last one ragged
when H % 64 != 0 (lanes masked by ``on``, clamped by ``hc``); the embedding's destination pass covers 1, 2 or 4
blocks per wave (nblk = 3 in the 4-block form with a dead block) and, above 256 channels, runs once per group
of four blocks; it takes 8 waves per node below 8192 atoms and 2 from there up; the second order runs the same
kernels on dual numbers at 4 waves -- and every kernel walks a row two edges per wave and iteration with a
one-edge tail.  The shared graph has rows of 1, 2-3, 9-16, 17-32 and more than 33 edges, so that at 4 and 8
waves some waves see no edge, some one (tail only), some one full pair, some a pair plus a tail.

Reference: ``kernels.tn_embed_composite`` / ``kernels.tn_message_composite`` in fp64 on the SAME inputs (the
fp32 inputs upcast), gradients by ``torch.autograd.grad``.  Bars: fp64 kernels 1e-12 forward, 1e-11 first order,
1e-10 second order (those of test_tn_compact_edge_kernels_match_composite and test_gpu_tn_second_order); fp32
kernels the form of test_gpu_gemm_routing._check's x3 bar, per output tensor

    e_k <= 2 * e_c + 4 * 2**-24 * scale

with e_k / e_c the max abs error against fp64 of the kernel / of the composite run in fp32 on the GPU, and
scale the max abs of the fp64 result (the factor 2 and the 4 ulp of scale allow for another legitimate
summation order and a composite that happens to be lucky).  Every figure is printed (``pytest -s``).

Per-edge inputs are symmetric under edge reversal as in a real model (W, C, ea functions of |r|; u flips), and
per-edge gradients are compared per pair: the kernels attribute a pair's gradient to the row edge, the
composite to its reverse.
"""
import copy
import functools

import pytest
import torch

from oracle import model_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUT = 4.5
F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -24


# ----------------------------------------------------------------------------- graphs
def _shared_positions():
    """60 hand-placed atoms in one molecule: a 44-atom blob inside one cutoff around atom 0, nine atoms walking
    out of it (rows thinning from 40 to 11 edges), a six-atom chain spaced just under the cutoff (rows of
    2-3) and one atom far from everything (its self loop only).  No distance is within 4e-3 of the cutoff."""
    g = torch.Generator().manual_seed(7)
    v = torch.randn(44, 3, generator=g, dtype=F64)
    r = torch.rand(44, 1, generator=g, dtype=F64) ** (1 / 3)
    blob = 2.2 * r * v / v.norm(dim=1, keepdim=True)
    blob[0] = 0.0
    k = torch.arange(9, dtype=F64)
    rot = torch.tensor([[0.6, 0.8, 0.0], [-0.8, 0.6, 0.0], [0.0, 0.0, 1.0]], dtype=F64)
    halo = torch.stack([3.4 + 0.35 * k, 0 * k, 0 * k], 1) @ rot
    c = torch.arange(6, dtype=F64)
    chain = torch.stack([40.0 + 4.4 * c, 0 * c, 0 * c], 1)
    far = torch.tensor([[0.0, 0.0, 200.0]], dtype=F64)
    return torch.cat([blob, halo, chain, far])


def _build(pos, cutoff, cap, static=False):
    from torchmdnet import kernels
    pos = pos.to(DEV)
    batch = torch.zeros(pos.shape[0], dtype=torch.long, device=DEV)
    return kernels.build_graph(pos, batch, 0.0, cutoff, cap, loop=True, strategy="brute",
                               static_capacity=cap if static else None)


def _row_lengths(graph):
    rp = graph.row_ptr.cpu().long()
    return rp[1:] - rp[:-1]


@functools.lru_cache(maxsize=None)
def _shared_graph():
    graph = _build(_shared_positions(), CUT, 4096)
    lens = _row_lengths(graph)
    # the row-length classes the two-edge walk needs at S = 4 and 8
    assert int((lens == 1).sum()) >= 1
    assert int(((lens >= 2) & (lens <= 3)).sum()) >= 1
    assert int(((lens >= 9) & (lens <= 16)).sum()) >= 1
    assert int(((lens >= 17) & (lens <= 32)).sum()) >= 1
    assert int((lens >= 33).sum()) >= 40
    assert int(lens[0]) >= 40  # atom 0 (the multiplicity's self loop) sits in the blob
    assert graph.symmetric
    return graph


def _with_mult(graph, mult):
    g = copy.copy(graph)
    g.self0_mult = mult
    return g


def _lattice_positions(n):
    """n atoms: a jittered 21^3 simple-cubic lattice (spacing 1) in index order with four isolated atoms at
    indices 1-4, so a truncation to fewer atoms keeps the layout of the rows it keeps."""
    g = torch.Generator().manual_seed(11)
    m = 21
    i = torch.arange(m ** 3)
    grid = torch.stack([i // (m * m), (i // m) % m, i % m], 1).to(F64)
    grid = grid + 0.18 * (2 * torch.rand(grid.shape, generator=g, dtype=F64) - 1)
    iso = torch.tensor([[-50.0, 0, 0], [-60.0, 0, 0], [-70.0, 0, 0], [-80.0, 0, 0]], dtype=F64)
    return torch.cat([grid[:1], iso, grid[1:n - 4]])


# ----------------------------------------------------------------------------- inputs, bars
def _embed_inputs(graph, H, dtype, seed):
    """(P, Q, W, C, u, gE) in ``dtype`` on the GPU, pair-symmetric."""
    T = graph.transpose.long().cpu()
    n_e = T.shape[0]
    N = graph.n_nodes
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    P, Q, W, C, u, gE = rn(N, H), rn(N, H), rn(n_e, 3 * H), torch.rand(n_e, generator=g, dtype=F64), rn(n_e, 3), \
        rn(9, N, H)
    W, C, u = W + W[T], C + C[T], u - u[T]
    return [t.to(dtype).to(DEV) for t in (P, Q, W, C, u, gE)]


def _msg_inputs(graph, H, dtype, seed):
    """(ea, Tc, gmsg, gadd) in ``dtype`` on the GPU, ea pair-symmetric."""
    T = graph.transpose.long().cpu()
    n_e, N = T.shape[0], graph.n_nodes
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    ea, Tc, gm, gadd = rn(n_e, 3 * H), rn(9, N, H), rn(9, N, H), rn(9, N, H)
    ea = ea + ea[T]
    return [t.to(dtype).to(DEV) for t in (ea, Tc, gm, gadd)]


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _guarded(rows, *cols, dtype):
    """A NaN-filled [rows, *cols] per-edge output as a view of a buffer one row longer, and that extra row: it
    must stay NaN (a store past the last edge row lands there and is seen, not outside the buffer)."""
    buf = _nan(rows + 1, *cols, dtype=dtype)
    return buf[:rows], buf[rows:]


def _untouched(*guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


def _pair_syms(graph):
    T = graph.transpose.long()
    even, odd, same = (lambda g: g + g[T]), (lambda g: g - g[T]), (lambda g: g)
    return same, even, odd


def _check(name, got, ref, comp, tol64):
    """fp64: max abs error relative to the result's max abs below ``tol64``; fp32: the e_k <= 2 e_c + 4 ulp bar
    (module docstring).  A NaN anywhere (a lane that did not write) fails either."""
    ref = ref.detach()
    scale = float(ref.abs().max())
    e_k = float((got.detach().double() - ref).abs().max())
    if got.dtype == F64:
        print(f"{name}: fp64 e_k {e_k:.3g} scale {scale:.3g} rel {e_k / scale:.3g}")
        assert e_k / scale < tol64, (name, e_k, scale)
        return
    e_c = float((comp.detach().double() - ref).abs().max())
    print(f"{name}: fp32 e_k {e_k:.3g} e_c {e_c:.3g} scale {scale:.3g} e_k/e_c {e_k / max(e_c, 1e-300):.3g}")
    assert e_k <= 2 * e_c + 4 * ULP * scale, (name, e_k, e_c, scale)


def _grads(fn, leaves, gout):
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    return torch.autograd.grad(fn(*leaves), leaves, gout)


def _refs(fn, leaves, gout, dtype):
    """(value, gradients) of the composite in fp64 on the upcast inputs and, for fp32 kernels, in fp32."""
    up = [t.double() for t in leaves]
    r64 = (fn(*up), _grads(fn, up, gout.double()))
    r32 = (fn(*leaves), _grads(fn, leaves, gout)) if dtype == F32 else (None, [None] * len(leaves))
    return r64, r32


# ----------------------------------------------------------------------------- 1. width x dtype x multiplicity
def _check_embed_first_order(graph, H, dtype, tag, seed=4):
    from torchmdnet import kernels
    N, E = graph.n_nodes, graph.n_edges
    P, Q, W, C, u, gE = _embed_inputs(graph, H, dtype, seed)
    comp = lambda *a: kernels.tn_embed_composite(*a, graph)  # noqa: E731
    (ref, refg), (c32, c32g) = _refs(comp, [P, Q, W, C, u], gE, dtype)
    out = _nan(9, N, H, dtype=dtype)
    kernels.tn_embed_fwd_launch(P, Q, W, C, u, graph, out)
    _check(f"{tag} embed_fwd", out, ref, c32, 1e-12)
    edge = [_guarded(*t.shape, dtype=dtype) for t in (W, C, u)]
    gs = [_nan(N, H, dtype=dtype), _nan(N, H, dtype=dtype)] + [v for v, _ in edge]
    kernels.tn_embed_bwd_launch(P, Q, W, C, u, graph, gE, *gs)
    assert _untouched(*[g for _, g in edge]), f"{tag} embed_bwd wrote past the last edge row"
    same, even, odd = _pair_syms(graph)
    for nm, a, b, c, sym in zip(("gP", "gQ", "gW", "gC", "gu"), gs, refg, c32g, (same, same, even, even, odd)):
        _check(f"{tag} embed_bwd {nm}", sym(a), sym(b), None if c is None else sym(c), 1e-11)
    return gs


@pytest.mark.parametrize("mult", [1.0, 4.0])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [64, 100, 192, 256])
def test_edge_kernels_match_composite_across_widths(H, dtype, mult):
    """tmdnet_tn_embed_fwd / _bwd and tmdnet_tn_message_fwd / _bwd(_add) at nblk = 1, 2 (ragged), 3 (the 4-block
    destination pass with a dead block) and 4, both dtypes, with and without atom 0's self-loop multiplicity;
    outputs pre-filled with NaN."""
    from torchmdnet import kernels
    graph = _with_mult(_shared_graph(), mult)
    N = graph.n_nodes
    tag = f"H{H} m{mult:g}"
    _check_embed_first_order(graph, H, dtype, tag)
    ea, Tc, gm, gadd = _msg_inputs(graph, H, dtype, 5)
    comp = lambda *a: kernels.tn_message_composite(*a, graph)  # noqa: E731
    (ref, refg), (c32, c32g) = _refs(comp, [ea, Tc], gm, dtype)
    msg = _nan(9, N, H, dtype=dtype)
    kernels.tn_message_fwd_launch(ea, Tc, graph, msg)
    _check(f"{tag} msg_fwd", msg, ref, c32, 1e-12)
    _, even, _ = _pair_syms(graph)
    for add in (None, gadd):
        (gea, guard), gT = _guarded(*ea.shape, dtype=dtype), _nan(9, N, H, dtype=dtype)
        kernels.tn_message_bwd_launch(ea, Tc, graph, gm, gea, gT, gadd=add)
        w = "" if add is None else "+gadd"
        assert _untouched(guard), f"{tag} msg_bwd{w} wrote past the last edge row"
        _check(f"{tag} msg_bwd{w} gea", even(gea), even(refg[0]), None if c32g[0] is None else even(c32g[0]), 1e-11)
        plus = (lambda t: t) if add is None else (lambda t: t + add.to(t.dtype))
        _check(f"{tag} msg_bwd{w} gT", gT, plus(refg[1]), None if c32g[1] is None else plus(c32g[1]), 1e-11)


# ----------------------------------------------------------------------------- 2. pair rows
@pytest.mark.parametrize("mult", [1.0, 4.0])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [100, 256])
def test_pair_row_message_matches_composite_across_widths(H, dtype, mult):
    """tmdnet_tn_message_{fwd,bwd}_pairs (one factor row per edge pair) against the composite through the
    differentiable gather ``_ea_edges``: message, pair-row factor gradient, component gradient + addend."""
    from torchmdnet import kernels
    graph = _with_mult(_shared_graph(), mult)
    pairs = kernels.pair_index(graph)
    N, Pn = graph.n_nodes, pairs[1].shape[0]
    g = torch.Generator().manual_seed(6)
    ea, Tc, gm, gadd = [torch.randn(*s, generator=g, dtype=F64).to(dtype).to(DEV)
                        for s in ((Pn, 3 * H), (9, N, H), (9, N, H), (9, N, H))]
    comp = lambda e, t: kernels.tn_message_composite(kernels._ea_edges(e, pairs), t, graph)  # noqa: E731
    (ref, refg), (c32, c32g) = _refs(comp, [ea, Tc], gm, dtype)
    tag = f"pairs H{H} m{mult:g}"
    msg = _nan(9, N, H, dtype=dtype)
    kernels.tn_message_fwd_launch(ea, Tc, graph, msg, pairs=pairs)
    _check(f"{tag} msg_fwd", msg, ref, c32, 1e-12)
    (gea, guard), gT = _guarded(Pn, 3 * H, dtype=dtype), _nan(9, N, H, dtype=dtype)
    kernels.tn_message_bwd_launch(ea, Tc, graph, gm, gea, gT, gadd=gadd, pairs=pairs)
    assert _untouched(guard), f"{tag} msg_bwd wrote past the last pair row"
    _check(f"{tag} msg_bwd gea", gea, refg[0], c32g[0], 1e-11)
    _check(f"{tag} msg_bwd gT", gT, refg[1] + gadd.double(), None if c32g[1] is None else c32g[1] + gadd, 1e-11)


# ----------------------------------------------------------------------------- 3. second order (and 6: H = 320)
def _embed_autograd(kind, leaves, graph, tang):
    """kernels.tn_embed (kind "hip") or its composite: value, first-order gradients (create_graph) and the
    gradients of <tang, first-order gradients> w.r.t. (P, Q, W, C, u, gE)."""
    from torchmdnet import kernels
    xs = [t.detach().clone().requires_grad_(True) for t in leaves]
    fn = kernels.tn_embed if kind == "hip" else kernels.tn_embed_composite
    out = fn(*xs[:5], graph)
    first = torch.autograd.grad(out, xs[:5], xs[5], create_graph=True)
    s = sum((a * t.to(a.dtype)).sum() for a, t in zip(first, tang))
    return out, first, torch.autograd.grad(s, xs)


def _check_embed_autograd(H, dtype, mult):
    graph = _with_mult(_shared_graph(), mult)
    leaves = _embed_inputs(graph, H, dtype, 8)
    # cotangents of the first-order gradients obey the kernels' pair precondition like the inputs
    tang = _embed_inputs(graph, H, F64, 9)[:5]
    up = [t.double() for t in leaves]
    ref = _embed_autograd("composite", up, graph, tang)
    c32 = _embed_autograd("composite", leaves, graph, tang) if dtype == F32 else None
    got = _embed_autograd("hip", leaves, graph, tang)
    same, even, odd = _pair_syms(graph)
    tag = f"H{H} m{mult:g} tn_embed"
    _check(f"{tag} fwd", got[0], ref[0], None if c32 is None else c32[0], 1e-12)
    syms = (same, same, even, even, odd, same)
    names = ("P", "Q", "W", "C", "u", "gE")
    for order, tol in ((1, 1e-11), (2, 1e-10)):
        for i, (a, b) in enumerate(zip(got[order], ref[order])):
            c = None if c32 is None else syms[i](c32[order][i])
            _check(f"{tag} order {order} d{names[i]}", syms[i](a), syms[i](b), c, tol)


@pytest.mark.parametrize("mult", [1.0, 4.0])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [100, 256])
def test_embedding_second_order_across_widths(H, dtype, mult):
    """kernels.tn_embed differentiated twice (tn_node.SECOND_ORDER at its default: tmdnet_tn_embed_bwd2, the
    first-order kernels on dual numbers at 4 waves) against the composite differentiated twice."""
    _check_embed_autograd(H, dtype, mult)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [100, 256])
def test_message_second_order_across_widths(H, dtype):
    """kernels.tn_message differentiated twice (the hand path: forward and first-backward launches on the
    cotangents) against the composite differentiated twice."""
    from torchmdnet import kernels
    graph = _with_mult(_shared_graph(), 4.0)
    leaves = _msg_inputs(graph, H, dtype, 10)[:3]  # ea, Tc, gmsg
    t_ea, t_T = _msg_inputs(graph, H, F64, 11)[:2]  # t_ea pair-symmetric like ea

    def run(kind, ls):
        xs = [t.detach().clone().requires_grad_(True) for t in ls]
        fn = kernels.tn_message if kind == "hip" else kernels.tn_message_composite
        first = torch.autograd.grad(fn(xs[0], xs[1], graph), xs[:2], xs[2], create_graph=True)
        s = (first[0] * t_ea.to(first[0].dtype)).sum() + (first[1] * t_T.to(first[1].dtype)).sum()
        return first, torch.autograd.grad(s, xs)

    ref = run("composite", [t.double() for t in leaves])
    c32 = run("composite", leaves) if dtype == F32 else None
    got = run("hip", leaves)
    same, even, _ = _pair_syms(graph)
    for order, syms, names, tol in ((0, (even, same), ("ea", "Tc"), 1e-11),
                                    (1, (even, same, same), ("ea", "Tc", "gmsg"), 1e-10)):
        for i, (a, b) in enumerate(zip(got[order], ref[order])):
            c = None if c32 is None else syms[i](c32[order][i])
            _check(f"H{H} tn_message order {order + 1} d{names[i]}", syms[i](a), syms[i](b), c, tol)


# ----------------------------------------------------------------------------- 4. static capacity, values
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_static_capacity_values_match_dynamic_graph(dtype):
    """The same atoms on a static-capacity graph (capacity > pairs, the HIP-graph step's layout), H = 192: every
    output and the valid rows of every per-edge gradient equal the dynamic graph's bit for bit (same rows, same
    order), the tail rows are zero, and the host and device forms of atom 0's multiplicity agree bit for bit."""
    from torchmdnet import kernels
    H = 192
    dyn = _with_mult(_shared_graph(), 4.0)
    E, N = dyn.n_edges, dyn.n_nodes
    cap = E + 37
    st = _build(_shared_positions(), CUT, cap, static=True)
    assert int(st.num_pairs_dev.item()) == E and st.n_edges == cap
    assert torch.equal(st.src[:E], dyn.src) and torch.equal(st.row_ptr, dyn.row_ptr)
    host = _with_mult(st, 4.0)
    dev = copy.copy(st)
    dev.self0_dev = (st.num_pairs_dev, E + 3)  # 1 + (E + 3 - E) = 4
    emb = _embed_inputs(dyn, H, dtype, 4)
    msg = _msg_inputs(dyn, H, dtype, 5)
    g = torch.Generator().manual_seed(12)

    def padded(t):  # capacity rows: the dynamic graph's, then finite junk no row refers to
        junk = torch.randn(cap - E, *t.shape[1:], generator=g, dtype=F64).to(t.dtype).to(DEV)
        return torch.cat([t, junk])

    def run(graph, pad):
        P, Q, W, C, u, gE = emb
        ea, Tc, gm, gadd = msg
        if pad:
            W, C, u, ea = padded(W), padded(C), padded(u), padded(ea)
        n_e = W.shape[0]
        out = _nan(9, N, H, dtype=dtype)
        kernels.tn_embed_fwd_launch(P, Q, W, C, u, graph, out)
        edge = [_guarded(*t.shape, dtype=dtype) for t in (W, C, u)]
        gs = [_nan(N, H, dtype=dtype), _nan(N, H, dtype=dtype)] + [v for v, _ in edge]
        kernels.tn_embed_bwd_launch(P, Q, W, C, u, graph, gE, *gs)
        m = _nan(9, N, H, dtype=dtype)
        kernels.tn_message_fwd_launch(ea, Tc, graph, m)
        (gea, guard), gT = _guarded(n_e, 3 * H, dtype=dtype), _nan(9, N, H, dtype=dtype)
        kernels.tn_message_bwd_launch(ea, Tc, graph, gm, gea, gT, gadd=gadd)
        assert _untouched(guard, *[g for _, g in edge]), "a store past the last edge row"
        return dict(E=out, gP=gs[0], gQ=gs[1], gW=gs[2], gC=gs[3], gu=gs[4], msg=m, gea=gea, gT=gT)

    r_dyn, r_host, r_dev = run(dyn, False), run(host, True), run(dev, True)
    edge = ("gW", "gC", "gu", "gea")
    for k in r_dyn:
        assert torch.isfinite(r_dyn[k]).all(), k
        assert torch.equal(r_host[k], r_dev[k]), f"{k}: host and device multiplicity differ"
        valid = r_host[k][:E] if k in edge else r_host[k]
        assert torch.equal(valid, r_dyn[k]), f"{k}: static-capacity graph differs from the dynamic one"
        if k in edge:
            assert (r_host[k][E:] == 0).all(), f"{k}: padding rows not zeroed"
    # and the values themselves against fp64 (the dynamic graph's are those of case 1 at H = 192)
    P, Q, W, C, u, gE = emb
    comp = lambda *a: kernels.tn_embed_composite(*a, dyn)  # noqa: E731
    (ref, refg), (c32, c32g) = _refs(comp, [P, Q, W, C, u], gE, dtype)
    same, even, odd = _pair_syms(dyn)
    _check("static E", r_host["E"], ref, c32, 1e-12)
    for nm, b, c, sym in zip(("gP", "gQ", "gW", "gC", "gu"), refg, c32g, (same, same, even, even, odd)):
        a = r_host[nm][:E] if nm in edge else r_host[nm]
        _check(f"static {nm}", sym(a), sym(b), None if c is None else sym(c), 1e-11)
    ea, Tc, gm, gadd = msg
    comp = lambda *a: kernels.tn_message_composite(*a, dyn)  # noqa: E731
    (ref, refg), (c32, c32g) = _refs(comp, [ea, Tc], gm, dtype)
    _check("static msg", r_host["msg"], ref, c32, 1e-12)
    _check("static gea", even(r_host["gea"][:E]), even(refg[0]), None if c32 is None else even(c32g[0]), 1e-11)
    _check("static gT", r_host["gT"], refg[1] + gadd.double(), None if c32 is None else c32g[1] + gadd, 1e-11)


# ----------------------------------------------------------------------------- 5. the 8192-atom form switch
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_embed_backward_across_8192_atom_switch(dtype):
    """The embedding's destination pass takes 2 waves per node from 8192 atoms up and 8 below: 8200 sparse atoms
    (jittered lattice, mean row ~6 edges, rows of 1) against the composite, and the same layout truncated to
    8000 atoms, so a wrong result traces to the form and not to the inputs."""
    for n in (8000, 8200):
        graph = _with_mult(_build(_lattice_positions(n), 1.15, 16 * n), 4.0)
        lens = _row_lengths(graph)
        assert graph.n_nodes == n and int((lens == 1).sum()) >= 4
        assert 5.0 < float(lens.double().mean()) < 7.0
        _check_embed_first_order(graph, 64, dtype, f"n{n}", seed=13)


# ----------------------------------------------------------------------------- 6. past 256 channels
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_embedding_past_256_channels(dtype):
    """H = 320 (nblk = 5: the destination pass in two launches of four blocks, the second with three dead blocks
    adding its per-edge sums to the first's): forward, backward and double backward of kernels.tn_embed, and
    the launch entries with NaN-filled outputs."""
    graph = _with_mult(_shared_graph(), 4.0)
    _check_embed_first_order(graph, 320, dtype, "H320")
    _check_embed_autograd(320, dtype, 4.0)


def test_tensornet_320_channels_matches_oracle():
    """A TensorNet wider than 256 channels (1 layer, 16 RBF) on three QM9-like molecules: energy and forces
    against the fp64 oracle at the project's 1e-4, and the force-loss backward runs (no refusal from inside
    backward)."""
    from conftest import yaml_args
    from torchmdnet.models.model import create_model
    args = yaml_args("tensornet", embedding_dimension=320, num_layers=1, num_rbf=16, derivative=True)
    torch.manual_seed(0)
    m = create_model(args)
    z, pos, batch = O.qm9_like(3)
    y_ref, f_ref = O.energy_forces(m.state_dict(), dict(args), z, pos, batch,
                                   static_shapes=m.representation_model.static_shapes)
    m = m.to(DEV)
    y, f = m(z.to(DEV), pos.float().to(DEV), batch.to(DEV))
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max())  # noqa: E731
    print(f"H320 model: energy rel {rel(y, y_ref):.3g} forces rel {rel(f, f_ref):.3g}")
    assert rel(y, y_ref) < 1e-4 and rel(f, f_ref) < 1e-4
    (y.pow(2).sum() + f.pow(2).sum()).backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
