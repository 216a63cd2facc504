"""Case tables, operand builders and float64 references of the dense-GEMM edge tests (tests/test_gpu_gemm_edges.py,
tests/gemm_env_worker.py; checked on the CPU by tests/test_gemm_ref_cpu.py).  Nothing here touches a kernel.

Two operand modes:

  "exact"   A, B, A2, B2, bias and the initial C are fp32 integers drawn uniformly from {-3 .. 3}, row scales from
            {0.5, 1, 2}.  Every product and partial sum is an integer of magnitude <= 9 (K + K2) + 6 < 2**24
            (``exact_bound``), exact in fp32 under any summation order, K split or partial-tile reduction -- and
            the integers fit the first bf16 piece of the x3 split.  The kernel's result is compared bit for bit.
  "random"  randn operands, the right operand divided by sqrt(K); compared against fp64 at the bar
            e_k <= factor * e_c + 4 * 2**-24 * scale (``within_bar``).

Input padding is NaN, output padding is SENT: an operand is the [:rows, :cols] slice of a taller, wider buffer.
The kernels clamp row and column indices into the valid range, so a NaN is never a legitimate read.

Restated launch rules (from csrc/gemm.hip, to be kept in step with it): ``grouped_form`` is gemm_run's choice of
k_gemm<NW, KMAX>, ``x3_form`` is tmdnet_gemm_x3_f32's tile width / grid / remap, ``tn_plan_v`` and ``tn_split``
are the weight-gradient split-K plans, ``tn_workspace_bytes`` the workspace query."""
import hashlib
import itertools
import math
from collections import namedtuple

import torch

SENT = -77.0
ULP = 2.0 ** -24
INT_MAX = 3

# One dense problem C = epilogue(A op(B) + bias + beta C0): tb = B is [N][K] (NT) else [K][N] (NN); the six
# options are the subsets of section B.
Spec = namedtuple("Spec", "M N K tb bias beta pre act rscale dpre", defaults=(0, 0, 0, 0, 0, 0))
OPTIONS = ("bias", "beta", "pre", "act", "rscale", "dpre")


def spec_name(s):
    opts = "".join(o[0] if o != "beta" else "B" for o in OPTIONS if getattr(s, o)) or "-"
    return f"{s.M}x{s.N}x{s.K}{'NT' if s.tb else 'NN'}:{opts}"


def is_plain(s):
    return not (s.pre or s.act or s.rscale or s.dpre)


def exact_output(s):
    """Whether C itself is exact in exact mode (SiLU and its derivative are not; ``pre`` always is)."""
    return not (s.act or s.dpre)


def exact_bound(K, K2=0):
    """Largest magnitude an exact-mode partial sum can reach: 9 per product, 3 for the bias, 3 for C0."""
    return INT_MAX * INT_MAX * (K + K2) + 2 * INT_MAX


# ----------------------------------------------------------------------------- restated launch rules
def grouped_form(kmax, nw_small=4, nw_large=16, kb4=1):
    """(NW, KMAX, per) of gemm_run for a launch whose longest K is kmax: per = 16-wide K blocks of the longest
    per-wave slice; per > KMAX means the slice loops over load batches with a partial last batch."""
    nw = nw_large if kmax >= 256 else nw_small
    per = (kmax // 16 + nw - 1) // nw
    if nw <= 2:
        return 2, 8, per
    if nw >= 16:
        return 16, min(max(per, 1), 4), per
    if nw >= 8:
        return 8, (2 if per <= 2 else 8), per
    if per <= 2:
        return 4, (1 if kb4 <= 1 else 2), per
    return 4, (4 if per <= 4 else 8), per


def x3_form(M, N):
    """(tile width BN, nx, ny, remap) of tmdnet_gemm_x3_f32; 128 rows per workgroup."""
    bn = 64 if N <= 64 else 128 if (N < 256 or M >= 131072) else 64
    nx, ny = (N + bn - 1) // bn, (M + 127) // 128
    return bn, nx, ny, nx > 1


def tn_split(tiles, kmax, target=1024):
    S = (target + tiles - 1) // tiles
    S = min(S, max(1, kmax // 256))
    return max(1, min(S, 64))


def tn_plan_v(shapes, split=True, target=1024):
    """shapes: (M, Nr, KT) per problem (Nr = columns of B that are read).  Returns (S per problem, tiles per
    problem, partial tiles)."""
    nt = [((M + 63) // 64) * max(1, (Nr + 63) // 64) for M, Nr, _ in shapes]
    work = sum(n * KT for n, (_, _, KT) in zip(nt, shapes))
    rows = max(256, (work + target - 1) // target)
    S = [max(1, min(64, (KT + rows - 1) // rows)) if split else 1 for _, _, KT in shapes]
    parts = sum(n * s for n, s in zip(nt, S) if s > 1)
    return S, nt, parts


def tn_workspace_bytes(probs):
    """probs: (M, N, K, K2, ones) per problem, N counting the ones column."""
    tiles = sum(((M + 31) // 32) * ((N + 31) // 32) for M, N, _, _, _ in probs)
    kmax = max(K + K2 for _, _, K, K2, _ in probs)
    _, _, parts = tn_plan_v([(M, N - 1 if ones else N, K + K2) for M, N, K, K2, ones in probs])
    S = tn_split(tiles, kmax)
    return max(4 * 1024 * tiles * S if S > 1 else 0, 4 * (64 * 64 + 64) * parts)


def tn_form(M, Nb, K, K2=0, ones=False, aligned=True, ws=True, tn_v=None):
    """The weight-gradient kernel one problem reaches: (name, waves, split S)."""
    N = Nb + int(ones)
    have_ws = ws and tn_workspace_bytes([(M, N, K, K2, ones)]) > 0
    if aligned:
        S = tn_plan_v([(M, Nb, K + K2)], have_ws)[0][0]
        narrow = Nb <= 32
        form = tn_v if tn_v else (2 if narrow else 1)
        nw = 8 if (K + K2 >= 8192 and S == 1) else 4
        return (f"v2<{nw},{2 if narrow else 4}>" if form == 2 else f"v<{nw}>"), nw, S
    tiles = ((M + 31) // 32) * ((N + 31) // 32)
    S = tn_split(tiles, K + K2) if have_ws else 1
    nw = 16 if (K + K2 >= 8192 and S == 1) else 4
    return f"tn<{nw}>", nw, S


# ----------------------------------------------------------------------------- case tables
K_LADDER = (16, 32, 48, 64, 128, 144, 160, 192, 208, 240, 256, 272, 512, 528, 768, 784, 1024, 1040, 1280, 2048)
LADDER_MN = (37, 70)
DEFAULT_FORMS = {(4, 1), (4, 4), (16, 1), (16, 2), (16, 3), (16, 4)}


def ladder_specs():
    M, N = LADDER_MN
    return [Spec(M, N, K, tb, bias=1) for K in K_LADDER for tb in (1, 0)]


EDGE_M = (1, 31, 32, 33, 65)
EDGE_N = (1, 15, 16, 17, 32, 33, 70)


def edge_specs(K):
    """The 32-tile edges at one K; beta on for every other case."""
    return [Spec(M, N, K, tb, bias=(i // 2) % 2, beta=i % 2)
            for i, (M, N, tb) in enumerate(itertools.product(EDGE_M, EDGE_N, (1, 0)))]


GROUP4 = (Spec(33, 17, 16, 1, bias=1), Spec(1, 70, 640, 0, beta=1), Spec(64, 32, 272, 1),
          Spec(37, 33, 96, 0, bias=1, beta=1))
GROUPS = {
    "as_listed": GROUP4,
    "reversed": GROUP4[::-1],
    # the problem of fewest tiles between the others, and (every listed problem has two tiles or more: 2, 3, 2, 4)
    # the same order with a true one-tile problem in its place
    "fewest_between": (GROUP4[2], GROUP4[0], GROUP4[3], GROUP4[1]),
    "one_tile_between": (GROUP4[2], Spec(17, 30, 16, 1, bias=1), GROUP4[3], GROUP4[1]),
    "all_below_256": (Spec(33, 17, 16, 1, bias=1), Spec(1, 70, 240, 0, beta=1), Spec(64, 32, 144, 1),
                      Spec(37, 33, 96, 0, bias=1, beta=1)),
}


def option_subsets(M, N, K, tb):
    return [Spec(M, N, K, tb, *bits) for bits in itertools.product((0, 1), repeat=6)]


EPI_GROUPED = ((33, 17, 48, 1), (37, 70, 272, 0))
EPI_X3 = ((129, 80, 96, 1), (129, 48, 160, 0))

X3_M = (1, 127, 128, 129, 300)
X3_K = (32, 64, 96, 128, 160, 288)
X3_N = (16, 48, 64, 80, 128, 144, 272)
X3_WIDE = (131072, 256, 32)


def x3_ladder_specs():
    return [Spec(129, N, K, tb, bias=1, beta=(K // 32) % 2) for N in (80, 272) for K in X3_K for tb in (1, 0)]


def x3_edge_specs(K):
    return [Spec(M, N, K, tb, bias=(i + tb) % 2, beta=(j + tb) % 2)
            for i, M in enumerate(X3_M) for j, N in enumerate(X3_N) for tb in (1, 0)]


TN_M = (63, 64, 65)
TN_NB = (31, 32, 33, 63, 64, 65)
TN_K = (15, 16, 17, 600)
TN_K2 = 37  # not a multiple of 16: a wave's row range crosses the segment boundary
TN_LONG = (2048, 2048, 8192)  # M, Nb, K of the unsplit long-K problem
# One weight-gradient problem C [M][Nb (+1)] (+)= A^T [B | 1] (+ A2^T [B2 | 1 or 0]); cb: the ones column to Cb
TNSpec = namedtuple("TNSpec", "M Nb K K2 ones ones2 cb beta", defaults=(0, 0, 0, 0, 0))


def tn_name(s):
    return f"{s.M}x{s.Nb}x{s.K}+{s.K2}:o{s.ones}{s.ones2}c{s.cb}b{s.beta}"


def tn_edge_specs(K):
    """Every (M, Nb) edge pair at one K: without / with ones, without / with a second segment (its ones column on
    and off), Cb on every other ones case, beta alternating."""
    out = []
    for i, (M, Nb) in enumerate(itertools.product(TN_M, TN_NB)):
        for j, (ones, K2, ones2) in enumerate(((0, 0, 0), (1, 0, 0), (0, TN_K2, 0), (1, TN_K2, 1), (1, TN_K2, 0))):
            out.append(TNSpec(M, Nb, K, K2, ones, ones2, cb=int(bool(ones) and (i + j) % 2 == 0), beta=(i + j) % 2))
    return out


TN_EMPTY = (TNSpec(65, 33, 0, 0, beta=0), TNSpec(65, 33, 0, 0, beta=1), TNSpec(64, 32, 0, 0, ones=1, cb=1, beta=1),
            TNSpec(65, 33, 0, TN_K2, beta=0), TNSpec(65, 33, 0, TN_K2, ones=1, ones2=1, beta=1))
EMB_N = (8191, 8192, 8200)
EMB_H = (32, 64, 33)
EMB_TYPES = 100
EMB_ABSENT = 57  # a type no atom has


def tn_group_specs(n):
    """n small problems of mixed shapes (TN_MAX = 32 share a launch; a longer list is split by wgrad_tn)."""
    shapes = list(itertools.product(TN_M, (31, 33, 64, 65)))
    return [TNSpec(*shapes[i % len(shapes)], 40 + 17 * (i % 5), TN_K2 if i % 3 == 0 else 0, ones=i % 2,
                   ones2=(i % 2) * (i % 3 == 0), cb=int(i % 4 == 1), beta=(i // 2) % 2) for i in range(n)]


# ----------------------------------------------------------------------------- operands
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _values(shape, mode, g, scale=1.0):
    if mode == "exact":
        return torch.randint(-INT_MAX, INT_MAX + 1, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g) * scale


def padded(vals, ld, fill, device, extra_rows=2):
    """(buffer, view): ``vals`` as the [:rows, :cols] slice of a ``fill``-ed [rows + extra_rows][ld] buffer."""
    r, c = vals.shape
    buf = torch.full((r + extra_rows, ld), fill, dtype=torch.float32)
    buf[:r, :c] = vals
    buf = buf.to(device)
    return buf, buf[:r, :c]


def padding_untouched(buf, rows, cols):
    """Everything of an output buffer outside [:rows, :cols] still holds SENT."""
    return bool((buf[rows:] == SENT).all()) and bool((buf[:rows, cols:] == SENT).all())


def build(s, mode, device, seed=0, x3=False):
    """Operands of one Spec: a dict with A, B, bias, C, pre, rscale, dpre (views / None), C0 (the initial C
    values), and the output buffers Cbuf / prebuf.  lda = K + 4, ldb = K + 8 (NT) or N + 3 (NN; N + 8 for x3,
    whose 16-byte loads need it), ldc = N + 5 (N + 8 for x3), pre / dpre on one row stride N + 12."""
    g = _gen(1000003 * seed + 7919 * s.M + 31 * s.N + s.K + 2 * s.tb)
    nan = float("nan")
    o = {}
    _, o["A"] = padded(_values((s.M, s.K), mode, g), s.K + 4, nan, device)
    bs = 1.0 / math.sqrt(s.K)
    if s.tb:
        _, o["B"] = padded(_values((s.N, s.K), mode, g, bs), s.K + 8, nan, device)
    else:
        _, o["B"] = padded(_values((s.K, s.N), mode, g, bs), s.N + (8 if x3 else 3), nan, device)
    o["bias"] = _values((s.N,), mode, g).to(device) if s.bias else None
    c0 = _values((s.M, s.N), mode, g)
    o["C0"] = c0.to(device)
    ldc = s.N + (8 if x3 else 5)
    if s.beta:
        o["Cbuf"], o["C"] = padded(c0, ldc, SENT, device)
    else:
        o["Cbuf"], o["C"] = padded(torch.full((s.M, s.N), SENT), ldc, SENT, device)
    ldx = s.N + 12
    o["prebuf"], o["pre"] = padded(torch.full((s.M, s.N), SENT), ldx, SENT, device) if s.pre else (None, None)
    if s.rscale:
        if mode == "exact":
            o["rscale"] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (s.M,), generator=g)].to(device)
        else:
            o["rscale"] = (torch.rand(s.M, generator=g) + 0.5).to(device)
    else:
        o["rscale"] = None
    o["dpre"] = padded(torch.randn(s.M, s.N, generator=g), ldx, nan, device)[1] if s.dpre else None
    return o


def dsilu(x):
    sg = torch.sigmoid(x)
    return sg * (1 + x * (1 - sg))


def reference(s, o, dtype=torch.float64):
    """(C, pre) of one Spec in ``dtype``.  The order is stated here once: v = A op(B) + bias + beta C0 goes to
    ``pre``; then C = silu(v) * rscale[:, None] * silu'(dpre).  With dtype = float32 on the GPU this is the
    composite whose error e_c the random-mode bar is relative to (library GEMM, F.silu)."""
    A, B = o["A"].to(dtype), o["B"].to(dtype)
    v = A @ (B.t() if s.tb else B)
    if s.bias:
        v = v + o["bias"].to(dtype)
    if s.beta:
        v = v + o["C0"].to(dtype)
    pre = v
    c = torch.nn.functional.silu(v) if s.act else v
    if s.rscale:
        c = c * o["rscale"].to(dtype)[:, None]
    if s.dpre:
        c = c * dsilu(o["dpre"].to(dtype))
    return c, pre


def gemm_args(s, o):
    """The argument tuple of kernels.Gemm for one built Spec."""
    return (o["A"], o["B"], bool(s.tb), o["bias"], o["C"], bool(s.beta), int(s.act), o["pre"], o["rscale"], o["dpre"])


def build_tn(s, mode, device, seed=0, aligned=True, lda=None):
    """Operands of one TNSpec: the wgrad_tn problem dict ``p`` plus C0 / Cb0 and the output buffers.  Aligned:
    lda = M + 4 rounded up to a multiple of 4, ldb likewise from Nb + 8; misaligned: odd row strides (the 32-tile
    kernel); ``lda`` overrides A's.  ldc = N + 5."""
    g = _gen(1000003 * seed + 7919 * s.M + 31 * s.Nb + s.K + 3 * s.K2)
    nan = float("nan")

    def ld(cols, pad):
        v = cols + pad
        return (v + 3) // 4 * 4 if aligned else v | 1

    N = s.Nb + int(bool(s.ones or s.ones2) and not s.cb)
    o = {"spec": s}
    p = {"beta": bool(s.beta), "ones": bool(s.ones), "ones2": bool(s.ones2)}
    KT = max(1, s.K + s.K2)
    for a, b, K in (("A", "B", s.K), ("A2", "B2", s.K2)):
        if a == "A2" and K == 0:
            continue
        _, p[a] = padded(_values((K, s.M), mode, g), lda or ld(s.M, 4), nan, device)
        _, p[b] = padded(_values((K, s.Nb), mode, g, 1.0 / math.sqrt(KT)), ld(s.Nb, 8), nan, device)
    c0 = _values((s.M, N), mode, g)
    o["C0"] = c0.to(device)
    o["Cbuf"], p["C"] = padded(c0 if s.beta else torch.full((s.M, N), SENT), N + 5, SENT, device)
    if s.cb:
        cb0 = _values((s.M,), mode, g)
        o["Cb0"] = cb0.to(device)
        o["Cbbuf"] = torch.full((s.M + 3,), SENT)
        if s.beta:
            o["Cbbuf"][:s.M] = cb0
        o["Cbbuf"] = o["Cbbuf"].to(device)
        p["Cb"] = o["Cbbuf"][:s.M]
    o["p"] = p
    return o


def reference_tn(o, dtype=torch.float64, rows=None):
    """(C, Cb or None) of one built TNSpec in ``dtype``: the sum over the rows of both segments (only the first
    ``rows`` of each when given), the ones column last, + beta times the initial values."""
    s, p = o["spec"], o["p"]
    anyones = bool(s.ones or s.ones2)
    dev = o["C0"].device
    res = torch.zeros((s.M, s.Nb + int(anyones)), dtype=dtype, device=dev)
    for a, b, ones in (("A", "B", s.ones), ("A2", "B2", s.ones2)):
        if a not in p:
            continue
        A, B = p[a].to(dtype), p[b].to(dtype)
        if rows is not None:
            A, B = A[:rows], B[:rows]
        res[:, :s.Nb] += A.t() @ B
        if ones:
            res[:, s.Nb] += A.sum(0)
    if s.cb:
        c, cb = res[:, :s.Nb], res[:, s.Nb]
        if s.beta:
            c, cb = c + o["C0"].to(dtype), cb + o["Cb0"].to(dtype)
        return c, cb
    return (res + o["C0"].to(dtype) if s.beta else res), None


def build_embedding(n, H, mode, device, seed=0):
    """(z, grad view, out buffer [types + 2][H], out0): n atoms of EMB_TYPES types, none of type EMB_ABSENT."""
    g = _gen(77 * seed + n + 13 * H)
    z = torch.randint(0, EMB_TYPES - 1, (n,), generator=g)
    z = torch.where(z >= EMB_ABSENT, z + 1, z)
    _, grad = padded(_values((n, H), mode, g, 1.0 / math.sqrt(n / EMB_TYPES)), H + 4 if H % 4 == 0 else H + 4 | 1,
                     float("nan"), device)
    out0 = _values((EMB_TYPES, H), mode, g)
    return z.to(device), grad, out0.to(device)


def reference_embedding(z, grad, out0, accumulate, dtype=torch.float64):
    ref = out0.to(dtype) if accumulate else torch.zeros_like(out0, dtype=dtype)
    return ref.index_add(0, z, grad.to(dtype))


# ----------------------------------------------------------------------------- comparison
def max_abs_err(got, ref, chunk=16384):
    """max |got - ref| over row chunks (no full-size float64 temporaries of the large cases)."""
    if got.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    e = 0.0
    for i in range(0, got.shape[0], chunk):
        e = max(e, float((got[i:i + chunk].to(ref.dtype) - ref[i:i + chunk]).abs().max()))
    return e


def within_bar(e_k, e_c, scale, factor=2.0):
    return e_k <= factor * e_c + 4 * ULP * scale


def digest(tensors):
    """A hex digest of fp32 tensors' bits (the worker prints it; the parent forms it from the references)."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to("cpu", torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()
