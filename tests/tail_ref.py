"""Float64 restatements of the kernels at the tail of every forward and training step, for
tests/test_gpu_tail_widths.py and tests/test_tail_ref_cpu.py: LayerNorm to second order (csrc/layernorm.hip), the
per-molecule sums (csrc/reduce.hip) and the two-term MSE loss (csrc/loss.hip).  Plain torch on the CPU: no GPU, no
native library.  Every function takes its operands as given (the float32 ones of a float32 kernel) and computes in
float64; tests/test_tail_ref_cpu.py holds each against float64 autograd of F.layer_norm, index_add and F.mse_loss.

Also here: the error measures of the GPU tests and the makers of their inputs, in two families.

    exact    small integers and halves: every partial sum, in any order and with or without fused multiply-adds,
             is a multiple of 1/2 below 2^22 in magnitude and so a float32 value; the kernel's answer must equal
             the float64 one bit for bit.  ``exact_headroom`` is the proof obligation (checked on the CPU for
             every case list).
    random   randn, held to a bound derived from the summation (``sum_bound``, ``mse2_bound``).
"""
import torch

F32, F64 = torch.float32, torch.float64
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
EXACT_LIMIT = 2.0 ** 22  # |std| = 2 doubles it: still below 2^23, where halves stop being float32 values


def _d(t):
    return None if t is None else t.detach().double().cpu()


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, w, b, eps):
    """(y, mean, rstd) of nn.LayerNorm over the last dimension of x [rows, C]: the biased variance, two passes."""
    x, w, b = _d(x), _d(w), _d(b)
    mean = x.mean(1)
    xc = x - mean[:, None]
    rstd = ((xc * xc).mean(1) + eps).rsqrt()
    return xc * rstd[:, None] * w + b, mean, rstd


def ln_bwd(x, w, mean, rstd, gy):
    """(gx, gw, gb) from the saved row statistics: gx = r (G - mean G - h mean(G h)), G = gy w, h = (x - mean) r;
    gw = colsum gy h; gb = colsum gy."""
    x, w, mean, rstd, gy = map(_d, (x, w, mean, rstd, gy))
    r = rstd[:, None]
    h = (x - mean[:, None]) * r
    G = gy * w
    gx = r * (G - G.mean(1, keepdim=True) - h * (G * h).mean(1, keepdim=True))
    return gx, (gy * h).sum(0), gy.sum(0)


def ln_bwd2(x, w, mean, rstd, gy, X, Wb, Bb):
    """(d_gy, d_x, d_w, T): the VJP of ln_bwd for cotangents (X, Wb, Bb) of (gx, gw, gb), any of them None, by the
    formulas in the header comment of k_bwd2 (csrc/layernorm.hip); d_w = colsum gy T."""
    x, w, mean, rstd, gy, X, Wb, Bb = map(_d, (x, w, mean, rstd, gy, X, Wb, Bb))
    C = x.shape[1]
    X = torch.zeros_like(x) if X is None else X
    Wb = torch.zeros_like(w) if Wb is None else Wb
    Bb = torch.zeros_like(w) if Bb is None else Bb
    m = lambda t: t.mean(1, keepdim=True)  # noqa: E731
    r = rstd[:, None]
    h = (x - mean[:, None]) * r
    G = gy * w
    T = r * (X - m(X) - h * m(X * h))
    d_gy = w * T + Wb * h + Bb
    u = -r * (G * m(X * h) + m(G * h) * X) + Wb * gy
    v = (X * (G - m(G) - h * m(G * h))).sum(1, keepdim=True)
    d_x = r * (u - m(u) - h * m(u * h)) - v * r * r * h / C
    return d_gy, d_x, (gy * T).sum(0), T


def ln_inputs(rows, C, seed=0, offset=0.0):
    """float32 (x, w, b, gy, X, Wb, Bb) on the CPU; x = offset + randn."""
    g = torch.Generator().manual_seed(1000 * C + rows + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F32)  # noqa: E731
    x = rn(rows, C) + offset
    return x, 1 + 0.5 * rn(C), rn(C), rn(rows, C), rn(rows, C), rn(C), rn(C)


def row_err(a, ref):
    """Worst row of (max |a - ref| in the row / max |ref| in the row); inf if a row whose reference is identically
    zero is not exactly zero.  1-D operands are one row."""
    a, ref = _d(a), _d(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert bool(torch.isfinite(a).all())
    a, ref = a.reshape(-1, a.shape[-1]) if a.dim() > 1 else a[None], ref.reshape(-1, ref.shape[-1]) if ref.dim() > 1 \
        else ref[None]
    if a.numel() == 0:
        return 0.0
    err, top = (a - ref).abs().amax(1), ref.abs().amax(1)
    if bool(err[top == 0].any()):
        return float("inf")
    return float((err / top.clamp(min=1e-300)).max())


def col_err(a, ref, scale):
    """Worst column of |a - ref| / scale, scale the column's sum of absolute terms; inf if a column of scale 0 is
    not exact."""
    a, ref, scale = _d(a), _d(ref), _d(scale)
    assert a.shape == ref.shape == scale.shape
    assert bool(torch.isfinite(a).all())
    if a.numel() == 0:
        return 0.0
    err = (a - ref).abs()
    if bool(err[scale == 0].any()):
        return float("inf")
    return float((err / scale.clamp(min=1e-300)).max())


# ----------------------------------------------------------------------------- molecule sums
def _opt(v, default):
    return default if v is None else float(_d(v).reshape(-1)[0])


def atom_sum(x, batch, n_mol, std, mean):
    """y[b] = mean + std * sum_{batch[n] = b} x[n]; ids outside [0, n_mol) are dropped; None std / mean: 1 / 0."""
    x, batch = _d(x).reshape(-1), batch.detach().cpu()
    on = (batch >= 0) & (batch < n_mol)
    y = torch.zeros(n_mol, dtype=F64).index_add_(0, batch[on], x[on])
    return _opt(mean, 0.0) + _opt(std, 1.0) * y


def dot_rows(h, w, b0):
    """Per-atom h[n] . w + b0 (what tmdnet_dot_sum_fwd leaves in atom_buf)."""
    return _d(h) @ _d(w).reshape(-1) + _opt(b0, 0.0)


def dot_sum(h, w, b0, batch, n_mol, std, mean):
    """y[b] = mean + std * sum_{batch[n] = b} (h[n] . w + b0)."""
    return atom_sum(dot_rows(h, w, b0), batch, n_mol, std, mean)


def dot_sum_bwd(gy, batch, n_mol, std, w):
    """gh[n, k] = std * gy[batch[n]] * w[k], rows with an id outside [0, n_mol) zero.  K = 1 and w = 1 is the
    atom sum's."""
    gy, w, batch = _d(gy).reshape(-1), _d(w).reshape(-1), batch.detach().cpu()
    on = (batch >= 0) & (batch < n_mol)
    a = torch.zeros(batch.shape[0], dtype=F64)
    a[on] = _opt(std, 1.0) * gy[batch[on]]
    return a[:, None] * w[None, :]


def sum_bound(h, w, b0, batch, n_mol, std, mean, dtype):
    """Per molecule of m atoms: (m + K + 4) u (|std| sum_n (sum_k |h_nk w_k| + |b0|) + |mean|): the first-order
    worst case of an m-term and a K-term sum in any order, the scale and the add.  h [n] with w None is the atom
    sum (K = 1)."""
    h, batch = _d(h), batch.detach().cpu()
    if w is None:
        h, w = h.reshape(-1, 1), torch.ones(1, dtype=F64)
    K = h.shape[1]
    on = (batch >= 0) & (batch < n_mol)
    rows = (h.abs() @ _d(w).reshape(-1).abs()) + abs(_opt(b0, 0.0))
    mag = torch.zeros(n_mol, dtype=F64).index_add_(0, batch[on], rows[on])
    m = torch.zeros(n_mol, dtype=F64).index_add_(0, batch[on], torch.ones(int(on.sum()), dtype=F64))
    return (m + K + 4) * U[dtype] * (abs(_opt(std, 1.0)) * mag + abs(_opt(mean, 0.0)))


BATCH_KINDS = ("sorted", "shuffled", "empty", "range")


def make_batch(kind, n, n_mol, seed=0):
    """int64 molecule ids.  sorted: non-decreasing, every molecule non-empty once n >= n_mol; shuffled: the same,
    permuted; empty: sorted with every third molecule (the first and the last among them) left empty, n_mol >= 3;
    range: shuffled, then every seventh id made n_mol, n_mol + 5 or a negative one in turn (n >= 2: at least one of
    each sign)."""
    g = torch.Generator().manual_seed(7919 * n + 31 * n_mol + seed)
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    if kind == "empty" and n_mol >= 3:
        keep = torch.tensor([b for b in range(n_mol) if b % 3 != 0 and b != n_mol - 1] or [1])
        ids = keep[torch.randint(0, len(keep), (n,), generator=g)].sort().values
        return ids
    ids = torch.cat([torch.arange(min(n, n_mol)), torch.randint(0, n_mol, (max(0, n - n_mol),), generator=g)])
    ids = ids.sort().values
    if kind in ("sorted", "empty"):
        return ids
    ids = ids[torch.randperm(n, generator=g)]
    if kind == "range" and n >= 2:
        bad = torch.tensor([n_mol, -1, n_mol + 5, -3])
        where = torch.arange(0, n, 7)
        if len(where) < 2:
            where = torch.tensor([0, 1])
        ids[where] = bad[torch.arange(len(where)) % 4]
    return ids


def has_empty(batch, n_mol):
    return len(set(batch.tolist()) & set(range(n_mol))) < n_mol


def sum_inputs(family, n, K, dtype, seed=0, hmax=8, wmax=3):
    """(h [n, K], w [K], b0 [1], std [1], mean [1]) on the CPU.  exact: h in halves of |h| <= hmax, w and b0
    integers of |w| <= wmax, std = 2, mean = -3; random: randn, std = 1.7, mean = -0.6."""
    g = torch.Generator().manual_seed(104729 * n + 17 * K + seed)
    if family == "exact":
        h = torch.randint(-2 * hmax, 2 * hmax + 1, (n, K), generator=g).to(dtype) / 2
        w = torch.randint(-wmax, wmax + 1, (K,), generator=g).to(dtype)
        w[w == 0] = 1
        return h, w, torch.tensor([2.0], dtype=dtype), torch.tensor([2.0], dtype=dtype), torch.tensor([-3.0],
                                                                                                        dtype=dtype)
    h = torch.randn(n, K, generator=g, dtype=dtype)
    w = torch.randn(K, generator=g, dtype=dtype)
    return (h, w, torch.randn(1, generator=g, dtype=dtype), torch.tensor([1.7], dtype=dtype),
            torch.tensor([-0.6], dtype=dtype))


def exact_headroom(h, w, b0, batch, n_mol):
    """Largest per-molecule sum of |h_nk w_k| + |b0| over EXACT_LIMIT; below 1 with every term a multiple of 1/2,
    every partial sum in every order is a float32 value (and std = 2, an integer mean keep it one)."""
    h = _d(h)
    if w is None:
        h, w = h.reshape(-1, 1), torch.ones(1, dtype=F64)
    for t, unit in ((h, 0.5), (_d(w), 1.0), (torch.tensor([_opt(b0, 0.0)]), 1.0)):
        assert bool((t / unit == (t / unit).round()).all()), "a value off the exact family's grid"
    on = (batch >= 0) & (batch < n_mol)
    rows = (h.abs() @ _d(w).reshape(-1).abs()) + abs(_opt(b0, 0.0))
    mag = torch.zeros(n_mol, dtype=F64).index_add_(0, batch[on], rows[on])
    return float(mag.max()) / EXACT_LIMIT if n_mol else 0.0


ATOM_SUM_N = (0, 1, 1023, 1024, 1025, 4096, 4097, 5000, 8193)  # 4096 | 4097: k_atom_sum | k_atom_runs
SUM_BWD_N = (1, 255, 256, 257, 4097)
DOT_K = (1, 15, 16, 17, 63, 64, 65, 100, 128)
DOT_N, DOT_MOLS = 203, 9
DOT_ROUTE = tuple((n, 32, 9, kind) for n in (4096, 4097) for kind in ("sorted", "range"))  # kernels.dot_sum's switch
MAX_MOLECULES = 8192


def kinds_for(n_mol):
    """A single molecule cannot be left empty among others: no "empty" kind there (n = 0 is its empty case)."""
    return tuple(k for k in BATCH_KINDS if not (n_mol < 3 and k == "empty"))


ATOM_SUM_CASES = tuple((n, m, k) for n in ATOM_SUM_N for m in (1, 37) for k in kinds_for(m))
SUM_BWD_CASES = tuple((n, 37, k) for n in SUM_BWD_N for k in BATCH_KINDS)
DOT_CASES = tuple((DOT_N, K, DOT_MOLS, "range" if i % 2 else "empty") for i, K in enumerate(DOT_K))
CEILING_CASE = (MAX_MOLECULES + 5, MAX_MOLECULES, "sorted")


def atom_case(family, n, n_mol, kind, dtype):
    """(x [n], batch, std, mean)."""
    h, _, _, std, mean = sum_inputs(family, n, 1, dtype)
    return h.reshape(-1), make_batch(kind, n, n_mol), std, mean


def dot_case(family, n, K, n_mol, kind, dtype):
    """(h [n, K], w, b0, batch, std, mean)."""
    h, w, b0, std, mean = sum_inputs(family, n, K, dtype)
    return h, w, b0, make_batch(kind, n, n_mol), std, mean


def exact_sum_cases():
    """(name, h, w, b0, batch, n_mol) of every exact-family case the GPU tests run (float32: the float64 ones
    hold the same values)."""
    for n, m, k in ATOM_SUM_CASES + (CEILING_CASE,):
        x, batch, _, _ = atom_case("exact", n, m, k, F32)
        yield f"atom_sum n={n} n_mol={m} {k}", x, None, None, batch, m
    for n, K, m, k in DOT_CASES + DOT_ROUTE:
        h, w, b0, batch, _, _ = dot_case("exact", n, K, m, k, F32)
        yield f"dot_sum n={n} K={K} n_mol={m} {k}", h, w, b0, batch, m


# ----------------------------------------------------------------------------- loss
def mse2(a1, b1, w1, a2, b2, w2):
    """w1 mean((a1 - b1)^2) + w2 mean((a2 - b2)^2), an empty side contributing 0 (the kernel's contract;
    F.mse_loss gives NaN there)."""
    return w1 * mse(a1, b1) + w2 * mse(a2, b2)


def mse(a, b):
    a, b = _d(a).reshape(-1), _d(b).reshape(-1)
    return float(((a - b) ** 2).mean()) if a.numel() else 0.0


def mse2_bwd(a1, b1, w1, a2, b2, w2, g):
    """(d1, d2) = (g w1 2 (a1 - b1) / n1, g w2 2 (a2 - b2) / n2)."""
    side = lambda a, b, w: g * w * 2.0 * (_d(a) - _d(b)) / max(1, a.numel())  # noqa: E731
    return side(a1, b1, w1), side(a2, b2, w2)


def mse2_scale(a1, b1, w1, a2, b2, w2):
    return abs(w1) * mse(a1, b1) + abs(w2) * mse(a2, b2)


def mse2_bound(family, n1, n2, dtype):
    """Relative to mse2_scale.  exact (integer differences, both sums of squares exact): two multiplies, two
    divides and one add, 5 u.  random: strided per-thread sums (n / 1024 terms), a 64-lane butterfly and 16 wave
    partials on top: (n / 1024 + 16 + 5) u."""
    return 5 * U[dtype] if family == "exact" else (max(n1, n2) / 1024 + 16 + 5) * U[dtype]


LOSS_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 3000)
# every pair with an empty side, the diagonal, both orders of (1, 3000), and the steps across a wave and across the
# 1024-thread workgroup in both orders
LOSS_PAIRS = tuple(sorted({(0, n) for n in LOSS_SIZES} | {(n, 0) for n in LOSS_SIZES}
                          | {(n, n) for n in LOSS_SIZES if n in (1, 64, 1024, 3000)}
                          | {(1, 3000), (3000, 1), (63, 65), (65, 63), (1023, 1025), (1025, 1023), (64, 1024)}))


def loss_inputs(family, n1, n2, dtype, seed=0):
    """(a1, b1, a2, b2) on the CPU.  exact: integers of |v| <= 8, so each squared difference is at most 256 and a
    sum of 3000 of them stays far below 2^24; random: randn."""
    g = torch.Generator().manual_seed(65537 * n1 + n2 + seed)
    if family == "exact":
        mk = lambda n: torch.randint(-8, 9, (n,), generator=g).to(dtype)  # noqa: E731
    else:
        mk = lambda n: torch.randn(n, generator=g, dtype=dtype)  # noqa: E731
    return mk(n1), mk(n1), mk(n2), mk(n2)


def ceil_div(a, b):
    return -(-a // b)


def wgrad_chunk(rows):
    """csrc/layernorm.hip wgrad_chunk: rows per partial block of the weight gradient."""
    return max(16, ceil_div(rows, 256))


def ln_cpl(C):
    """Values per lane of the LayerNorm row kernels (TMD_LN_CPL)."""
    return 2 if C <= 128 else 4 if C <= 256 else 6 if C <= 384 else 8 if C <= 512 else 16
