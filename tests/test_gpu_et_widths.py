"""The Equivariant-Transformer edge kernels (csrc/et_message.hip, csrc/et_fused.hip) across channel widths, row
lengths, launch forms and layouts, against their composites in fp64.

The message kernels compile one code path per lane width V = H / 32 in {1, 2, 4, 8} (the second order V = H / 64,
the neighbour embedding 1, 2 or 4), per head width in lanes lph = d / V, per waves-per-node count S in {4, 2, 1}
(switching at 4096 and 8192 atoms; fp64 at V = 8 always 1) and per backward form (destination + source in one
grid, in two launches, with injected projection cotangents, the three dr-mode forms), and walk a row in chunks
of 64 edges, S waves x 64 / L slots per step.  The shared graph is made of cliques of 1, 2, 3, 5, 8, 9, 16, 17,
33, 63, 64, 65, 128 and 130 atoms far apart, every atom with its self loop, so the rows have exactly those
lengths: one slot, a partial step, exactly one chunk, one chunk and one edge, two chunks, two chunks and two
edges.  The atom order is shuffled, so a clique's rows are not contiguous.  Isolated atoms appended up to 4097
and 8193 nodes switch S and leave a partially filled last block.

Reference: ``kernels.et_message_composite`` / ``kernels.nbr_embed_composite`` in fp64 on the SAME inputs (the
fp32 inputs upcast), gradients by ``torch.autograd.grad``.  Bars as in test_gpu_tn_widths: fp64 kernels 1e-12
forward, 1e-11 first order, 1e-10 second order (max abs error over max abs value, per tensor); fp32 kernels,
per output tensor,

    e_k <= 2 * e_c + 4 * 2**-24 * scale

with e_k / e_c the max abs error against fp64 of the kernel / of the composite run in fp32 on the GPU, and
scale the max abs of the fp64 result.  Every figure is printed (``pytest -s``) before anything is asserted.

Per-edge inputs are pair-symmetric as in a model (pk, pv, C even under edge reversal, u odd and 0 on a self
loop), and first-order per-edge gradients are compared per pair.

The fused-projection kernels (et_fused.hip) are driven as et_stack drives them (fep_split on planar-ordered
[dk | dv] weight rows, fep_frag_set with the pair numbers, the two launch functions) against
pre = W rbf(r) + b formed in fp64 from the fp32 weights and fed to the composite, autograd down to r; their
e_c is that of the unfused fp32 path (fp32 pre, fp32 composite), never of the fused kernel.

Worst fp32 e_k / e_c measured on an MI355X, per kernel family, the larger of two runs (the composite's
index_add is atomic, so e_c moves a little from run to run); the worst fp64 relative error is 1.5e-15, and no
fp32 tensor uses more than 0.6 of its bar:

    message, default form (k_fwd, k_bwd_both)          1.90   g_pv at (128, 16)
    backward launch forms (dst + src, ACC_GRADS, dr)   1.96   g_pv at (256, 8)
    waves per node (4097 / 8193 nodes)                 1.72   x of the last node at 4097
    layouts (planar, pair rows, strided)               2.06   g_k, strided (1.40 in the other run)
    runtime activation codes                           1.51   g_pv
    static capacity                                    1.74   g_pv
    second order (k_bwd2)                              1.62   g_pk of the first order it starts from
    neighbour embedding                                1.32   d x, second order, H = 128
    fused projection (fep::k_*)                        1.50   g_u, R = 32 gauss cutoff_lower 0.5; g_r at most 1.12

so the fused kernels meet the project's bar with the factor 2 unchanged.
"""
import contextlib
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUT = 4.5
F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -24
CLIQUES = (1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64, 65, 128, 130)  # 544 atoms, 47,392 edges
REDUCED = (1, 2, 3, 9, 17, 63, 64, 65, 130)  # 354 atoms, 29,574 edges: the widest and the second-order cases


# ----------------------------------------------------------------------------- graphs
def _lattice_ball():
    """The 130 points of a simple-cubic lattice of spacing 0.64 nearest its origin, nearest first: within a
    radius of 2.03, so a jittered clique has every distance in (0.53, 4.2)."""
    i = torch.arange(-4, 5)
    grid = torch.cartesian_prod(i, i, i).to(F64)
    order = torch.argsort((grid ** 2).sum(1), stable=True)
    return 0.64 * grid[order[:130]]


def _positions(sizes, n_nodes=None):
    """(positions, expected row length per atom): cliques 40 apart on a grid, shuffled; then isolated atoms 10
    apart, far from the cliques, up to ``n_nodes``."""
    g = torch.Generator().manual_seed(17)
    ball = _lattice_ball()
    parts = []
    for i, k in enumerate(sizes):
        centre = 40.0 * torch.tensor([float(i % 4), float(i // 4), 0.0], dtype=F64)
        parts.append(centre + ball[:k] + 0.03 * (2 * torch.rand(k, 3, generator=g, dtype=F64) - 1))
    pos = torch.cat(parts)
    lens = torch.cat([torch.full((k,), k, dtype=torch.long) for k in sizes])
    perm = torch.randperm(pos.shape[0], generator=g)
    pos, lens = pos[perm], lens[perm]
    if n_nodes is not None:
        j = torch.arange(n_nodes - pos.shape[0])
        iso = 10.0 * torch.stack([j % 20, (j // 20) % 20, j // 400], 1).to(F64)
        pos = torch.cat([pos, iso + torch.tensor([0.0, 0.0, 500.0], dtype=F64)])
        lens = torch.cat([lens, torch.ones(j.shape[0], dtype=torch.long)])
    return pos, lens


def _build(pos, cap, static=False):
    from torchmdnet import kernels
    pos = pos.to(DEV)
    batch = torch.zeros(pos.shape[0], dtype=torch.long, device=DEV)
    return kernels.build_graph(pos, batch, 0.0, CUT, cap, loop=True, strategy="brute",
                               static_capacity=cap if static else None)


def _row_lengths(graph):
    rp = graph.row_ptr.cpu().long()
    return rp[1:] - rp[:-1]


_KINDS = {"full": (CLIQUES, None), "reduced": (REDUCED, None), "tiny": ((1, 2, 3), None),
          "n4097": (CLIQUES, 4097), "n8193": (CLIQUES, 8193)}


@functools.lru_cache(maxsize=None)
def _graph(kind):
    sizes, n_nodes = _KINDS[kind]
    pos, lens = _positions(sizes, n_nodes)
    n_iso = 0 if n_nodes is None else n_nodes - sum(sizes)
    graph = _build(pos, sum(k * k for k in sizes) + n_iso)
    # conditions of every case below, not measurements
    assert torch.equal(_row_lengths(graph), lens), "row lengths are not the clique sizes"
    want = sorted([k for k in sizes for _ in range(k)] + [1] * n_iso)
    assert sorted(_row_lengths(graph).tolist()) == want
    assert graph.n_edges == sum(k * k for k in sizes) + n_iso
    assert graph.symmetric
    r = graph.distances.detach()[graph.src != graph.dst]
    if r.numel():
        assert float(r.min()) > 0.5 + 4e-3 and float(r.max()) < CUT - 4e-3
    return graph


def _v_perm(H, heads):
    """Column j of a planar v / pv row ([x | v1 | v2], H channels each) = column perm[j] of the per-head order
    ([h][x | v1 | v2], d channels each)."""
    d = H // heads
    j = torch.arange(3 * H)
    part, h, c = j // H, (j % H) // d, j % d
    return (h * 3 * d + part * d + c).to(DEV)


# ----------------------------------------------------------------------------- figures, bars
class _Report:
    """Prints every figure and collects the misses; ``done`` asserts there were none."""

    def __init__(self, family):
        self.family, self.miss = family, []

    def check(self, name, got, ref, comp, tol64):
        ref = ref.detach()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = float(ref.abs().max())
        e_k = float((got.detach().double() - ref).abs().max())  # NaN (a lane that did not write) misses either bar
        if got.dtype == F64:
            print(f"ETW|{self.family}|{name}|f64|e_k {e_k:.3g}|scale {scale:.3g}|rel {e_k / max(scale, 1e-300):.3g}")
            if not e_k < tol64 * scale:
                self.miss.append((name, e_k, scale))
            return
        e_c = float((comp.detach().double() - ref).abs().max())
        print(f"ETW|{self.family}|{name}|f32|e_k {e_k:.3g}|e_c {e_c:.3g}|scale {scale:.3g}|"
              f"ratio {e_k / max(e_c, 1e-300):.3g}")
        if not e_k <= 2 * e_c + 4 * ULP * scale:
            self.miss.append((name, e_k, e_c, scale))

    def require(self, cond, what):
        if not cond:
            print(f"ETW|{self.family}|{what}|FAILED")
            self.miss.append(what)

    def done(self):
        assert not self.miss, self.miss


def _nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _guarded(rows, *cols, dtype):
    """A NaN-filled [rows, *cols] output as a view of a buffer one row longer, and that extra row: it must stay
    NaN (a store past the last row lands there and is seen, not outside the buffer)."""
    buf = _nan(rows + 1, *cols, dtype=dtype)
    return buf[:rows], buf[rows:]


def _untouched(*guards):
    return all(bool(torch.isnan(g).all()) for g in guards)


@contextlib.contextmanager
def _tuning(both_max=None, merged_min=None):
    from torchmdnet import kernels
    prev = []
    try:
        for key, val in ((kernels.TUNE_ET_BOTH_MAX_NODES, both_max), (kernels.TUNE_ET_MERGED_MIN_NODES, merged_min)):
            if val is not None:
                prev.append((key, kernels.set_tuning(key, val)))
        yield
    finally:
        for key, val in reversed(prev):
            kernels.set_tuning(key, val)


# ----------------------------------------------------------------------------- inputs, reference
NAMES = ("q", "k", "v", "vec", "pk", "pv", "C", "u")


def _inputs(graph, H, dtype, seed):
    """Message operands in ``dtype`` on the GPU: node rows, PAIR rows pkP / pvP / dpkP / dpvP / CP (an edge reads
    row pr[e], so per-edge values are even under reversal), u odd, the output cotangents gx / gvec."""
    from torchmdnet import kernels
    pr, pe = kernels.pair_index(graph)
    E = graph.n_edges
    T = graph.transpose.long().cpu()
    N, P = graph.n_nodes, pe.shape[0]
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    d = dict(q=rn(N, H), k=rn(N, H), v=rn(N, 3 * H), vec=rn(N, 3, H), pkP=rn(P, H), pvP=rn(P, 3 * H),
             dpkP=rn(P, H), dpvP=rn(P, 3 * H), CP=torch.rand(P, generator=g, dtype=F64), gx=rn(N, H),
             gvec=rn(N, 3, H))
    u0 = rn(E, 3)
    d["u"] = u0 - u0[T]
    d = {k: t.to(dtype).to(DEV) for k, t in d.items()}
    d["pr"] = pr
    rows = pr.long()
    for k in ("pk", "pv", "dpk", "dpv", "C"):
        d[k] = d[k + "P"].index_select(0, rows)
    return d


def _composite(graph, heads, acts=0):
    from torchmdnet import kernels
    src, dst, N = graph.src.long(), graph.dst.long(), graph.n_nodes
    return lambda *a: kernels.et_message_composite(*a, src, dst, N, heads, acts)


def _first_order(fn, leaves, gouts):
    xs = [t.detach().clone().requires_grad_(True) for t in leaves]
    out = fn(*xs)
    return [o.detach() for o in out], list(torch.autograd.grad(out, xs, gouts))


def _reference(graph, heads, I, dtype, acts=0):
    """dict(out, grads[, out32, grads32]) of the composite in fp64 on the upcast inputs and, for fp32 kernels, in
    fp32; and the dr-mode contraction <g_pk, dpk> + <g_pv, dpv> of its gradients."""
    fn = _composite(graph, heads, acts)
    leaves = [I[n] for n in NAMES]
    R = {}
    R["out"], R["grads"] = _first_order(fn, [t.double() for t in leaves], (I["gx"].double(), I["gvec"].double()))
    R["g_r"] = (R["grads"][4] * I["dpk"].double()).sum(1) + (R["grads"][5] * I["dpv"].double()).sum(1)
    if dtype == F32:
        R["out32"], R["grads32"] = _first_order(fn, leaves, (I["gx"], I["gvec"]))
        R["g_r32"] = (R["grads32"][4] * I["dpk"]).sum(1) + (R["grads32"][5] * I["dpv"]).sum(1)
    return R


# ----------------------------------------------------------------------------- launches
PAD = 8  # guard columns of the strided [N, 5H + PAD] buffers


def _operands(graph, heads, I, planar=False, pairs=False, strided=False):
    """What the launch functions take: v / pv (and dpv) in the planar order, pk / pv as pair rows with the edge's
    row numbers, q / k / v as column views of one [N, 5H + PAD] buffer (its last PAD columns NaN)."""
    H = I["q"].shape[1]
    perm = _v_perm(H, heads) if planar else None
    lay = (lambda t: t.index_select(1, perm)) if planar else (lambda t: t)
    sfx = "P" if pairs else ""
    A = dict(q=I["q"], k=I["k"], v=lay(I["v"]), vec=I["vec"], pk=I["pk" + sfx], pv=lay(I["pv" + sfx]),
             dpk=I["dpk" + sfx], dpv=lay(I["dpv" + sfx]), C=I["C"], u=I["u"], rows=I["pr"] if pairs else None,
             lay=lay, strided=strided)
    if strided:
        N = I["q"].shape[0]
        buf = _nan(N, 5 * H + PAD, dtype=I["q"].dtype)
        buf[:, :H], buf[:, H:2 * H], buf[:, 2 * H:5 * H] = A["q"], A["k"], A["v"]
        A["q"], A["k"], A["v"] = buf[:, :H], buf[:, H:2 * H], buf[:, 2 * H:5 * H]
    return A


def _fwd(graph, heads, A, flags=0):
    from torchmdnet import kernels
    N, H = A["q"].shape
    dtype = A["q"].dtype
    (xo, g0), (vo, g1) = _guarded(N, H, dtype=dtype), _guarded(N, 3, H, dtype=dtype)
    kernels.et_message_fwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph, heads,
                                  xo, vo, flags=flags, pk_rows=A["rows"])
    return [xo, vo], _untouched(g0, g1)


def _bwd(graph, heads, A, I, flags=0, dr=False, prefill=None):
    """One tmdnet_et_message_bwd call into NaN-filled (or pre-filled) buffers.  Returns (the gradients in NAMES
    order -- g_pk / g_pv None in dr mode --, g_r or None, whether every guard row / column kept its NaN)."""
    from torchmdnet import kernels
    N, H = A["q"].shape
    E, dtype = graph.n_edges, A["q"].dtype
    guards = []
    if A["strided"]:
        gbuf, g = _guarded(N, 5 * H + PAD, dtype=dtype)
        gq, gk, gv = gbuf[:, :H], gbuf[:, H:2 * H], gbuf[:, 2 * H:5 * H]
        guards += [g, gbuf[:, 5 * H:]]
    else:
        (gq, a), (gk, b), (gv, c) = (_guarded(N, w, dtype=dtype) for w in (H, H, 3 * H))
        guards += [a, b, c]
    (gw, a), (gC, b), (gu, c) = _guarded(N, 3, H, dtype=dtype), _guarded(E, dtype=dtype), _guarded(E, 3, dtype=dtype)
    guards += [a, b, c]
    gpk = gpv = g_r = None
    if dr:
        g_r, a = _guarded(E, dtype=dtype)
        guards.append(a)
    else:
        (gpk, a), (gpv, b) = _guarded(E, H, dtype=dtype), _guarded(E, 3 * H, dtype=dtype)
        guards += [a, b]
    if prefill is not None:
        for buf, p in zip((gq, gk, gv, gw, gpk, gpv), prefill):
            buf.copy_(p)
    kernels.et_message_bwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph, heads,
                                  I["gx"], I["gvec"], gq, gk, gv, gw, gpk, gpv, gC, gu, accumulate=flags,
                                  pk_rows=A["rows"], dpk=A["dpk"] if dr else None, dpv=A["dpv"] if dr else None,
                                  g_r=g_r)
    return [gq, gk, gv, gw, gpk, gpv, gC, gu], g_r, _untouched(*guards)


def _syms(graph, n_edges=None):
    E = graph.n_edges if n_edges is None else n_edges
    T = graph.transpose[:E].long()
    same, even, odd = (lambda g: g), (lambda g: g + g[T]), (lambda g: g - g[T])
    return dict(q=same, k=same, v=same, vec=same, pk=even, pv=even, C=even, u=odd, g_r=even)


def _check_outputs(rep, tag, outs, R):
    for i, nm in enumerate(("x", "vec_out")):
        c = R["out32"][i] if "out32" in R else None
        rep.check(f"{tag} fwd {nm}", outs[i], R["out"][i], c, 1e-12)


def _check_grads(rep, tag, graph, grads, g_r, R, lay, prefill=None, n_edges=None):
    """The backward's outputs against the reference, per tensor; per-edge tensors per pair; v / pv gradients in
    the kernel's layout; with ``prefill`` the expectation is pre-fill + gradient."""
    S = _syms(graph, n_edges)
    E = graph.n_edges if n_edges is None else n_edges
    for i, nm in enumerate(NAMES):
        if grads[i] is None:
            continue
        got = grads[i][:E] if nm in ("pk", "pv", "C", "u") else grads[i]
        ref = R["grads"][i]
        c = R["grads32"][i] if "grads32" in R else None
        if nm in ("v", "pv"):
            ref, c = lay(ref), None if c is None else lay(c)
        if prefill is not None and i < 6:
            ref, c = ref + prefill[i].double(), None if c is None else c + prefill[i]
        sym = S[nm]
        rep.check(f"{tag} bwd g{nm}", sym(got), sym(ref), None if c is None else sym(c), 1e-11)
    if g_r is not None:
        rep.check(f"{tag} bwd g_r", S["g_r"](g_r[:E]), S["g_r"](R["g_r"]),
                  S["g_r"](R["g_r32"]) if "g_r32" in R else None, 1e-11)


@functools.lru_cache(maxsize=1)
def _case_data(kind, H, heads, dtype, seed, acts=0):
    """(graph, inputs, reference) of one case, shared by the layouts / forms that run on the same inputs; none of
    them writes into it."""
    graph = _graph(kind)
    I = _inputs(graph, H, dtype, seed)
    return graph, I, _reference(graph, heads, I, dtype, acts)


def _plain_case(rep, tag, kind, H, heads, dtype, seed=21, acts=0, planar=False, pairs=False, strided=False):
    """Forward and default backward of one (graph, width, dtype, layout) against the composite."""
    from torchmdnet import _native as nat
    graph, I, R = _case_data(kind, H, heads, dtype, seed, acts)
    A = _operands(graph, heads, I, planar, pairs, strided)
    flags = acts | (nat.ET_V_PLANAR if planar else 0)
    outs, clean = _fwd(graph, heads, A, flags)
    rep.require(clean, f"{tag} fwd: a store past the last node row")
    _check_outputs(rep, tag, outs, R)
    grads, _, clean = _bwd(graph, heads, A, I, flags)
    rep.require(clean, f"{tag} bwd: a store into a guard row or column")
    _check_grads(rep, tag, graph, grads, None, R, A["lay"])
    return I, R, A, outs, grads


# ----------------------------------------------------------------------------- 1. widths x dtype
WIDTHS = [(16, 2), (32, 4), (64, 8), (64, 1), (128, 8), (128, 1), (256, 8), (256, 4), (32, 32), (128, 16)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H,heads", WIDTHS, ids=[f"H{h}x{n}" for h, n in WIDTHS])
def test_message_kernels_match_composite_across_widths(H, heads, dtype):
    """k_fwd and k_bwd_both at V = 1, 1, 2, 2, 4, 4, 8, 8 (fp64 V = 8: one wave per node) and head groups of
    lph = 8, 8, 4, 32, 4, 32, 4, 8 lanes, then lph = 1 and 2; rows of 1 to 130 edges (the reduced graph at 256
    channels); NaN-filled outputs with guard rows."""
    rep = _Report("message")
    _plain_case(rep, f"H{H}x{heads}", "reduced" if H == 256 else "full", H, heads, dtype)
    rep.done()


# ----------------------------------------------------------------------------- 2. backward launch forms
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [128, 256])
def test_backward_launch_forms_match_composite(H, dtype):
    """tmdnet_et_message_bwd in every form it can take, each against the composite: both passes in one grid,
    destination then source, either with injected projection cotangents (TMDNET_ACC_GRADS: buffers pre-filled,
    expectation pre-fill + gradient), and dr mode (pair rows, g_r per pair against <g_pk, dpk> + <g_pv, dpv> of
    the COMPOSITE's gradients) as both-in-one-grid, two-pass and merged."""
    from torchmdnet import _native as nat
    heads = 8
    rep = _Report("message-forms")
    graph, I, R = _case_data("reduced" if H == 256 else "full", H, heads, dtype, 22)
    A = _operands(graph, heads, I)
    Ap = _operands(graph, heads, I, pairs=True)
    g = torch.Generator().manual_seed(23)
    prefill = [torch.randn(*R["grads"][i].shape, generator=g, dtype=F64).to(dtype).to(DEV) for i in range(6)]
    for form, both_max in (("both", None), ("dst+src", 0)):
        with _tuning(both_max=both_max):
            tag = f"H{H} {form}"
            grads, _, clean = _bwd(graph, heads, A, I, 0)
            rep.require(clean, f"{tag}: a store into a guard row")
            _check_grads(rep, tag, graph, grads, None, R, A["lay"])
            grads, _, clean = _bwd(graph, heads, A, I, nat.ACC_GRADS, prefill=prefill)
            rep.require(clean, f"{tag} acc: a store into a guard row")
            _check_grads(rep, tag + " acc", graph, grads, None, R, A["lay"], prefill=prefill)
    for form, tune, fl in (("dr-both", dict(), 0), ("dr-two-pass", dict(both_max=0, merged_min=0), nat.ET_TWO_PASS),
                           ("dr-merged", dict(merged_min=0), 0)):
        with _tuning(**tune):
            tag = f"H{H} {form}"
            grads, g_r, clean = _bwd(graph, heads, Ap, I, fl, dr=True)
            rep.require(clean, f"{tag}: a store into a guard row")
            _check_grads(rep, tag, graph, grads, g_r, R, Ap["lay"])
    rep.done()


# ----------------------------------------------------------------------------- 3. waves per node
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["n4097", "n8193"])
def test_waves_per_node_switches_match_composite(kind, dtype):
    """The clique graph plus isolated atoms up to 4097 nodes (two waves per node in the backward, the last block
    half filled) and 8193 nodes (one wave per node, the last block a quarter filled), H = 128, 8 heads; the last
    node's row and the highest-numbered clique atom's row also on their own."""
    rep = _Report("message-waves")
    graph = _graph(kind)
    H, heads = 128, 8
    _, R, _, outs, grads = _plain_case(rep, kind, kind, H, heads, dtype, seed=24)
    for row in (graph.n_nodes - 1, sum(CLIQUES) - 1):
        c = R.get("out32")
        rep.check(f"{kind} fwd x row {row}", outs[0][row], R["out"][0][row], None if c is None else c[0][row], 1e-12)
        for i in (0, 1, 2, 3):
            c = R.get("grads32")
            rep.check(f"{kind} bwd g{NAMES[i]} row {row}", grads[i][row], R["grads"][i][row],
                      None if c is None else c[i][row], 1e-11)
    rep.done()


# ----------------------------------------------------------------------------- 4. layouts
@pytest.mark.parametrize("layout", ["planar", "pairs", "planar+pairs", "strided"])
@pytest.mark.parametrize("H,heads,dtype", [(128, 8, F32), (64, 8, F64)], ids=["H128-f32", "H64-f64"])
def test_layouts_match_composite(H, heads, dtype, layout):
    """TMDNET_ET_V_PLANAR (v / pv / their gradients as three H-wide blocks), pair-shared projection rows (pk_rows
    of kernels.pair_index, pk / pv with P rows), both, and q / k / v as column views of one wider buffer with the
    gradients written into views of another whose other columns must keep their NaN."""
    rep = _Report("message-layouts")
    _plain_case(rep, f"H{H} {layout}", "full", H, heads, dtype, seed=25, planar="planar" in layout,
                pairs="pairs" in layout, strided=layout == "strided")
    rep.done()


# ----------------------------------------------------------------------------- 5. activations at width
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_runtime_activation_codes_at_four_channels_per_lane(dtype):
    """ShiftedSoftplus projections / Tanh attention at H = 128, 8 heads: the runtime-code instantiation of the
    kernels at V = 4 (the 4 x 4 activation table of test_gpu_activations runs V = 1)."""
    from torchmdnet import kernels
    rep = _Report("message-acts")
    acts = kernels.et_act_flags(kernels.ACT_CODES["ShiftedSoftplus"], kernels.ACT_CODES["Tanh"])
    _plain_case(rep, "H128 ssp/tanh", "full", 128, 8, dtype, seed=26, acts=acts)
    rep.done()


# ----------------------------------------------------------------------------- 6. static capacity
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_static_capacity_matches_dynamic_graph(dtype):
    """The same atoms on a static-capacity graph (capacity > edges), H = 128, 8 heads: every output and the valid
    rows of every per-edge gradient equal the dynamic graph's bit for bit, the rows past row_ptr[N] are exactly
    zero (plain and dr mode), the guard row past the capacity stays NaN; and the values against fp64."""
    rep = _Report("message-static")
    H, heads = 128, 8
    dyn, I, R = _case_data("full", H, heads, dtype, 27)
    E = dyn.n_edges
    cap = E + 37
    st = _build(_positions(CLIQUES)[0], cap, static=True)
    assert int(st.num_pairs_dev.item()) == E and st.n_edges == cap
    assert torch.equal(st.src[:E], dyn.src) and torch.equal(st.row_ptr, dyn.row_ptr)
    A = _operands(dyn, heads, I)
    g = torch.Generator().manual_seed(28)
    Ast = dict(A)
    for k in ("pk", "pv", "dpk", "dpv", "C", "u"):  # capacity rows: the dynamic graph's, then finite junk
        junk = torch.randn(cap - E, *A[k].shape[1:], generator=g, dtype=F64).to(dtype).to(DEV)
        Ast[k] = torch.cat([A[k], junk])
    res = {}
    for name, graph, ops in (("dyn", dyn, A), ("static", st, Ast)):
        outs, c0 = _fwd(graph, heads, ops)
        grads, _, c1 = _bwd(graph, heads, ops, I)
        _, g_r, c2 = _bwd(graph, heads, ops, I, dr=True)
        rep.require(c0 and c1 and c2, f"{name}: a store into a guard row")
        res[name] = outs + grads + [g_r]
    edge = (6, 7, 8, 9, 10)  # g_pk, g_pv, g_C, g_u, g_r within outs + grads + [g_r]
    for i, (a, b) in enumerate(zip(res["dyn"], res["static"])):
        rep.require(bool(torch.isfinite(a).all()), f"tensor {i}: not finite on the dynamic graph")
        valid = b[:E] if i in edge else b
        rep.require(torch.equal(valid, a), f"tensor {i}: the static-capacity graph differs from the dynamic one")
        if i in edge:
            rep.require(bool((b[E:] == 0).all()), f"tensor {i}: padding rows not zeroed")
    _check_outputs(rep, "static", res["static"][:2], R)
    _check_grads(rep, "static", dyn, res["static"][2:10], res["static"][10], R, A["lay"], n_edges=E)
    rep.done()


# ----------------------------------------------------------------------------- 7. second order
def _second_order_case(rep, H, heads, dtype, mode, monkeypatch):
    """_ETMessageBwd differentiated (tmdnet_et_message_bwd2) against double autograd through the composite,
    all ten inputs; ``mode``: "scratch" / "atomic" source pass, or "pairs" (the launch with pk_rows)."""
    from torchmdnet import kernels
    if mode == "atomic":
        monkeypatch.setattr(kernels, "BWD2_SCRATCH_MAX_BYTES", 0)
    graph = _graph("reduced")
    I = _inputs(graph, H, dtype, 29)
    leaves = [I["gx"], I["gvec"]] + [I[n] for n in NAMES]
    g = torch.Generator().manual_seed(30)
    ggs = [torch.randn(*I[n].shape, generator=g, dtype=F64).to(DEV) for n in NAMES]
    fn = _composite(graph, heads)

    def composite(ls, gg):
        xs = [t.detach().clone().requires_grad_(True) for t in ls]
        first = torch.autograd.grad(fn(*xs[2:]), xs[2:], (xs[0], xs[1]), create_graph=True)
        return [t.detach() for t in first], torch.autograd.grad(first, xs, [a.to(ls[0].dtype) for a in gg])

    def hip(ls, gg):
        gg = [a.to(ls[0].dtype) for a in gg]
        if mode == "pairs":
            out = kernels.et_message_bwd2_launch(ls[2], ls[3], ls[4], ls[5], I["pkP"], I["pvP"], ls[8], ls[9], graph,
                                                 heads, ls[0], ls[1], gg, pk_rows=I["pr"])
            return None, out
        xs = [t.detach().clone().requires_grad_(True) for t in ls]
        first = kernels._ETMessageBwd.apply(*xs, graph, heads)
        return [t.detach() for t in first], torch.autograd.grad(first, xs, gg)

    ref = composite([t.double() for t in leaves], ggs)
    c32 = composite(leaves, ggs) if dtype == F32 else None
    got = hip(leaves, ggs)
    tag = f"H{H} {mode}"
    if got[0] is not None:
        S = _syms(graph)
        for i, nm in enumerate(NAMES):
            c = None if c32 is None else S[nm](c32[0][i])
            rep.check(f"{tag} order 1 g{nm}", S[nm](got[0][i]), S[nm](ref[0][i]), c, 1e-11)
    for i, nm in enumerate(("gx", "gvec") + NAMES):
        rep.check(f"{tag} order 2 d{nm}", got[1][i], ref[1][i], None if c32 is None else c32[1][i], 1e-10)


@pytest.mark.parametrize("mode", ["scratch", "atomic"])
@pytest.mark.parametrize("H,dtype", [(64, F64), (128, F64), (128, F32), (256, F64)],
                         ids=["H64-f64", "H128-f64", "H128-f32", "H256-f64"])
def test_message_second_order_across_widths(H, dtype, mode, monkeypatch):
    """k_bwd2 at V = H / 64 = 1, 2 (eight waves per node) and 4, rows of 1 to 130 edges, the source-node terms by
    the scratch-row source pass and by atomics."""
    rep = _Report("message-2nd")
    _second_order_case(rep, H, 8, dtype, mode, monkeypatch)
    rep.done()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_message_second_order_with_pair_rows(dtype, monkeypatch):
    """tmdnet_et_message_bwd2 reading pair-shared projection rows through pk_rows, H = 128."""
    rep = _Report("message-2nd")
    _second_order_case(rep, 128, 8, dtype, "pairs", monkeypatch)
    rep.done()


# ----------------------------------------------------------------------------- 8. neighbour embedding
@pytest.mark.parametrize("with_self", [False, True], ids=["plain", "self"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [32, 128, 256])
def test_neighbour_embedding_across_widths(H, dtype, with_self):
    """kernels.nbr_embed (k_nb_fwd / k_nb_bwd_dst / _src / k_nb_bwd2_*) at 1, 2 and 4 channels per lane against
    nbr_embed_composite: forward, first and second order; with_self: the [x_self | x_nb] output of the same
    launch and its gradient read in place (row stride 2 H)."""
    from torchmdnet import kernels
    rep = _Report("nbr-embed")
    graph = _graph("full")
    pr = kernels.pair_index(graph)[0].long().cpu()
    N, P = graph.n_nodes, kernels.pair_index(graph)[1].shape[0]
    T = graph.transpose.long()
    src, dst = graph.src.long(), graph.dst.long()
    g = torch.Generator().manual_seed(31)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    x, xs, w, C = rn(N, H), rn(N, H), rn(P, H)[pr], torch.rand(P, generator=g, dtype=F64)[pr]
    go = rn(N, 2 * H if with_self else H)
    wts = [rn(N, H), rn(P, H)[pr], rn(P)[pr]] + ([rn(N, H)] if with_self else [])  # even on the per-edge gradients
    leaves = [t.to(dtype).to(DEV) for t in [x, w, C] + ([xs] if with_self else [])]
    go, wts = go.to(DEV), [t.to(DEV) for t in wts]

    def run(kind, ls):
        ins = [t.detach().clone().requires_grad_(True) for t in ls]
        x_self = ins[3] if with_self else None
        if kind == "hip":
            out = kernels.nbr_embed(ins[0], ins[1], ins[2], graph, x_self=x_self)
        else:
            out = kernels.nbr_embed_composite(ins[0], ins[1], ins[2], src, dst, N)
            out = torch.cat([x_self, out], 1) if with_self else out
        first = torch.autograd.grad(out, ins, go.to(out.dtype), create_graph=True)
        s = sum((a * b.to(a.dtype)).sum() for a, b in zip(first, wts))
        second = torch.autograd.grad(s, ins, allow_unused=True)
        return out.detach(), [t.detach() for t in first], second

    ref = run("composite", [t.double() for t in leaves])
    c32 = run("composite", leaves) if dtype == F32 else None
    got = run("hip", leaves)
    tag = f"H{H}" + (" self" if with_self else "")
    rep.check(f"{tag} fwd", got[0], ref[0], None if c32 is None else c32[0], 1e-12)
    even, same = (lambda t: t + t[T]), (lambda t: t)
    names, syms = ("x", "w", "C", "x_self"), (same, even, even, same)
    for i in range(len(leaves)):
        c = None if c32 is None else syms[i](c32[1][i])
        rep.check(f"{tag} order 1 g{names[i]}", syms[i](got[1][i]), syms[i](ref[1][i]), c, 1e-11)
    for i in range(len(leaves)):
        if ref[2][i] is None:  # x_self: its gradient does not depend on any input
            rep.require(got[2][i] is None or float(got[2][i].abs().max()) == 0, f"{tag} order 2 d{names[i]} not zero")
            continue
        rep.check(f"{tag} order 2 d{names[i]}", got[2][i], ref[2][i], None if c32 is None else c32[2][i], 1e-10)
    rep.done()


# ----------------------------------------------------------------------------- 9. fused-projection kernels
def _rbf_params(R, rbf_type, cl):
    """(mu, beta, code) of the reference's ExpNormalSmearing / GaussianSmearing at their initial values."""
    from torchmdnet import _native as nat
    if rbf_type == "expnorm":
        start = math.exp(-(CUT - cl))
        mu = torch.linspace(start, 1.0, R, dtype=F32)
        beta = torch.full((R,), (2.0 / R * (1.0 - start)) ** -2, dtype=F32)
        return mu.to(DEV), beta.to(DEV), nat.RBF_EXPNORM
    mu = torch.linspace(cl, CUT, R, dtype=F32)
    beta = torch.full((R,), -0.5 / float(mu[1] - mu[0]) ** 2, dtype=F32)
    return mu.to(DEV), beta.to(DEV), nat.RBF_GAUSS


def _fused_figures(rep, R, rbf_type, cl, planar, seed, counts=None):
    """One forward and one backward launch of the fused kernels on the full clique graph against fp64."""
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    H, heads = 128, 8
    graph = _graph("full")
    N, E = graph.n_nodes, graph.n_edges
    pairs = kernels.pair_index(graph)
    I = _inputs(graph, H, F32, seed)
    mu, beta, code = _rbf_params(R, rbf_type, cl)
    g = torch.Generator().manual_seed(seed + 100)
    W = (torch.randn(4 * H, R, generator=g, dtype=F64) / math.sqrt(R)).to(F32).to(DEV)  # per-head [dk | dv] rows
    b = (0.5 * torch.randn(4 * H, generator=g, dtype=F64)).to(F32).to(DEV)
    r = graph.distances.detach().to(F32)
    T = graph.transpose.long()
    assert torch.equal(r[T], r), "distances not pair-symmetric"
    perm = _v_perm(H, heads)
    one = torch.cat([torch.arange(H, device=DEV), H + perm])  # the image's rows are always in the planar order
    src, dst = graph.src.long(), graph.dst.long()

    def unfused(dt):
        """(outputs, gradients w.r.t. q, k, v, vec, C, u, r) of pre = W rbf(r) + b -> composite in ``dt``."""
        xs = [I[n].to(dt).detach().clone().requires_grad_(True) for n in ("q", "k", "v", "vec", "C", "u")]
        rr = r.to(dt).detach().clone().requires_grad_(True)
        f = kernels.rbf_composite(rr, mu.to(dt), beta.to(dt), cl, CUT, code)
        pre = f @ W.to(dt).t() + b.to(dt)
        out = kernels.et_message_composite(xs[0], xs[1], xs[2], xs[3], pre[:, :H], pre[:, H:], xs[4], xs[5], src,
                                           dst, N, heads)
        grads = torch.autograd.grad(out, xs + [rr], (I["gx"].to(dt), I["gvec"].to(dt)))
        return [o.detach() for o in out], list(grads)

    ref, c32 = unfused(F64), unfused(F32)
    lay = (lambda t: t.index_select(1, perm)) if planar else (lambda t: t)
    flags = nat.ET_V_PLANAR if planar else 0
    fep = kernels.fep_split(W.index_select(0, one).contiguous(), b.index_select(0, one).contiguous())
    frag = kernels.fep_frag_set(graph, r, (mu, beta, cl, CUT, code), pairs)
    q, k, v = I["q"], I["k"], lay(I["v"]).contiguous()
    (xo, g0), (vo, g1) = _guarded(N, H, dtype=F32), _guarded(N, 3, H, dtype=F32)
    kernels.et_fused_fwd_launch(q, k, v, I["vec"], I["C"], I["u"], fep, frag, graph, heads, xo, vo, flags=flags)
    (gq, a0), (gk, a1), (gv, a2), (gw, a3) = (_guarded(N, *s, dtype=F32) for s in ((H,), (H,), (3 * H,), (3, H)))
    (gC, a4), (gu, a5), (g_r, a6) = (_guarded(E, *s, dtype=F32) for s in ((), (3,), ()))
    kernels.et_fused_bwd_launch(q, k, v, I["vec"], I["C"], I["u"], fep, frag, graph, heads, I["gx"], I["gvec"], gq,
                                gk, gv, gw, gC, gu, g_r, accumulate=flags)
    if counts is not None:
        rep.require(counts == {"fwd": 1, "bwd": 1}, f"the fused launches did not run: {counts}")
    tag = f"R{R} {rbf_type} cl{cl:g} {'planar' if planar else 'per-head'} s{seed}"
    rep.require(_untouched(g0, g1, a0, a1, a2, a3, a4, a5, a6), f"{tag}: a store into a guard row")
    for i, nm in enumerate(("x", "vec_out")):
        rep.check(f"{tag} fwd {nm}", (xo, vo)[i], ref[0][i], c32[0][i], 1e-12)
    even, odd, same = (lambda t: t + t[T]), (lambda t: t - t[T]), (lambda t: t)
    for nm, got, i, sym in (("gq", gq, 0, same), ("gk", gk, 1, same), ("gv", gv, 2, same), ("gvec", gw, 3, same),
                            ("gC", gC, 4, even), ("gu", gu, 5, odd), ("g_r", g_r, 6, even)):
        a, c = ref[1][i], c32[1][i]
        if nm == "gv":
            a, c = lay(a), lay(c)
        rep.check(f"{tag} bwd {nm}", sym(got), sym(a), sym(c), 1e-11)


FUSED_CASES = [(64, "expnorm", 0.0), (32, "expnorm", 0.0), (64, "gauss", 0.0), (32, "gauss", 0.5),
               (64, "expnorm", 0.5)]


@pytest.mark.parametrize("planar", [False, True], ids=["per-head", "planar"])
@pytest.mark.parametrize("R,rbf_type,cl", FUSED_CASES, ids=[f"R{a}-{b}-cl{c:g}" for a, b, c in FUSED_CASES])
def test_fused_projection_kernels_match_fp64(R, rbf_type, cl, planar, monkeypatch):
    """tmdnet_et_fused_fwd_f32 / _bwd_f32 (H = 128, 8 heads) per tensor: x, vec_out, gq, gk, gv, gvec and gC, gu,
    g_r per pair; rows of 1, 3 (a partial 16-edge tile), 16 (one tile), 17 (a tile and an edge), 33, 64, 65, 130."""
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    assert kernels.fep_supported(128, 8, R, F32)
    lib, counts = nat.load(), {"fwd": 0, "bwd": 0}
    fwd0, bwd0 = lib.tmdnet_et_fused_fwd_f32, lib.tmdnet_et_fused_bwd_f32

    def counted(key, fn):
        def call(*a):
            counts[key] += 1
            return fn(*a)
        return call

    monkeypatch.setattr(lib, "tmdnet_et_fused_fwd_f32", counted("fwd", fwd0))
    monkeypatch.setattr(lib, "tmdnet_et_fused_bwd_f32", counted("bwd", bwd0))
    rep = _Report("fused")
    _fused_figures(rep, R, rbf_type, cl, planar, 33, counts)
    rep.done()


# ----------------------------------------------------------------------------- 10. envelope edges
REFUSED = [(96, 8), (192, 8), (128, 64), (96, 3)]


@pytest.mark.parametrize("H,heads", REFUSED, ids=[f"H{h}x{n}" for h, n in REFUSED])
def test_refused_widths_raise_and_write_nothing(H, heads):
    """V = H / 32 must be 1, 2, 4 or 8 and a head at least V channels: anything else is a RuntimeError from
    nat.check, from kernels.et_message and from the launch functions, whose NaN-filled outputs stay untouched."""
    from torchmdnet import kernels
    graph = _graph("tiny")
    I = _inputs(graph, H, F32, 34)
    with pytest.raises(RuntimeError, match="tmdnet_et_message_fwd failed"):
        kernels.et_message(*[I[n] for n in NAMES], graph, heads)
    A = _operands(graph, heads, I)
    N, E = graph.n_nodes, graph.n_edges
    xo, vo = _nan(N, H, dtype=F32), _nan(N, 3, H, dtype=F32)
    with pytest.raises(RuntimeError, match="tmdnet_et_message_fwd failed"):
        kernels.et_message_fwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph,
                                      heads, xo, vo)
    outs = [_nan(*s, dtype=F32) for s in ((N, H), (N, H), (N, 3 * H), (N, 3, H), (E, H), (E, 3 * H), (E,), (E, 3))]
    with pytest.raises(RuntimeError, match="tmdnet_et_message_bwd failed"):
        kernels.et_message_bwd_launch(A["q"], A["k"], A["v"], A["vec"], A["pk"], A["pv"], A["C"], A["u"], graph,
                                      heads, I["gx"], I["gvec"], *outs)
    torch.cuda.synchronize()
    assert _untouched(xo, vo, *outs)


def test_model_outside_the_fused_envelope_runs_the_plain_kernels(monkeypatch):
    """fep_supported false (H = 64) with FEP_MIN_EDGES at 0: the model must not call the fused launches, and runs
    the plain message kernel instead."""
    from conftest import yaml_args
    from torchmdnet import et_stack, kernels
    from torchmdnet.models.model import create_model
    assert not kernels.fep_supported(64, 8, 32, F32)
    calls = {"fused": 0, "plain": 0}
    plain0 = kernels.et_message_fwd_launch

    def fused(*a, **k):
        calls["fused"] += 1
        raise AssertionError("a fused launch outside fep_supported")

    def plain(*a, **k):
        calls["plain"] += 1
        return plain0(*a, **k)

    monkeypatch.setattr(kernels, "et_fused_fwd_launch", fused)
    monkeypatch.setattr(kernels, "et_fused_bwd_launch", fused)
    monkeypatch.setattr(kernels, "et_message_fwd_launch", plain)
    monkeypatch.setattr(et_stack, "FEP_MIN_EDGES", 0)
    torch.manual_seed(0)
    m = create_model(yaml_args("equivariant-transformer", embedding_dimension=64, num_heads=8, num_layers=2,
                               num_rbf=32, max_num_neighbors=128, derivative=True, output_model="Scalar")).to(DEV)
    g = torch.Generator().manual_seed(35)
    n = 96  # a water cluster: 32 molecules in a 10 A cube
    pos = (10.0 * torch.rand(n, 3, generator=g)).to(DEV)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3).to(DEV)
    y, f = m(z, pos, torch.zeros(n, dtype=torch.long, device=DEV))
    assert calls["fused"] == 0 and calls["plain"] >= 2, calls  # one plain forward per layer at least
    assert torch.isfinite(y).all() and torch.isfinite(f).all()
