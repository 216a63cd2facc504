"""The row-counted dk/dv projections (the ``rows`` operand of ``tmdnet_proj_f32`` / ``tmdnet_proj_act_f32``, csrc/gemm.hip
``tmd::proj``): with an int32 device row count the kernels write the rows below ``min(M, max(0, count))`` only.

Contract checked here, all as int32 bit patterns (no tolerance anywhere):
  * rows below the effective count == the same call without a count (same tiles, split, order, epilogue);
  * rows at or past it keep the sentinel the output was pre-filled with (no store at all), as do the guard
    columns of a wider buffer (``ldc > N``: S / D are column slices of one buffer in the model);
  * a null count == the uncounted launch, through the C ABI.
Shapes: K = 32 and 64, a whole and a partial 64-column tile (N = 64, 80), M = 160 = one whole and one partial
128-row tile, with and without dA / D; counts on every side of the 16-row block, the 128-row tile and M, plus the
two clamps (165 > M, -3 < 0); the 256-row tiles from M = 65536.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5EED5EED
COUNTS = (0, 1, 15, 16, 17, 127, 128, 129, 159, 160, 165, -3)
M0 = 160


def _filled(M, N, pad=0):
    """[M, N] fp32 view (row stride N + 2 * pad) of a sentinel-filled buffer, and the buffer."""
    buf = torch.full((M, N + 2 * pad), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf[:, pad:pad + N], buf


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    g = torch.Generator().manual_seed(1000 * K + N + M)
    A = torch.rand(M, K, generator=g).to(DEV)  # RBF rows: [0, 1]
    dA = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    return A, dA, W, b


def _run(kind, M, N, K, der, code, count, pad=0):
    """One launch into sentinel-filled outputs; ``count`` None: no row count.  Returns the bit patterns of the
    outputs' buffers (guard columns included)."""
    from torchmdnet import kernels
    A, dA, W, b = _operands(M, N, K)
    rows = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    if kind == "proj":
        out, buf = _filled(M, N, pad)
        got = kernels.proj(A, W, b, out=out, rows=rows)
        assert got.data_ptr() == out.data_ptr()
        return (_bits(buf),)
    S, sbuf = _filled(M, N, pad)
    D, dbuf = _filled(M, N, pad) if der else (None, None)
    got = kernels.proj_act(A, dA if der else None, W, b, code, out=(S, D), rows=rows)
    assert got is not None and got[0].data_ptr() == S.data_ptr()
    return (_bits(sbuf),) + ((_bits(dbuf),) if der else ())


@functools.lru_cache(maxsize=None)
def _full(kind, M, N, K, der, code, pad=0):
    """The launch without a count: computed once per shape, shared by every count."""
    return _run(kind, M, N, K, der, code, None, pad)


def _check_counts(kind, M, N, K, der, code, counts, pad=0):
    full = _full(kind, M, N, K, der, code, pad)
    for f in full:  # every row of the uncounted launch was written; the guard columns were not
        assert not bool((f[:, pad:pad + N] == SENTINEL).any())
        assert bool((f[:, :pad] == SENTINEL).all()) and bool((f[:, pad + N:] == SENTINEL).all())
    for c in counts:
        eff = min(M, max(0, c))
        for name, got, ref in zip("SD", _run(kind, M, N, K, der, code, c, pad), full):
            assert torch.equal(got[:eff], ref[:eff]), (kind, name, c, "live rows differ from the uncounted launch")
            assert bool((got[eff:] == SENTINEL).all()), (kind, name, c, "a row at or past the count was written")


@pytest.mark.parametrize("N", [64, 80])
@pytest.mark.parametrize("K", [32, 64])
def test_proj_rows_stops_at_the_count(K, N):
    _check_counts("proj", M0, N, K, False, 0, COUNTS)


@pytest.mark.parametrize("der", [False, True], ids=["S", "S+D"])
@pytest.mark.parametrize("N", [64, 80])
@pytest.mark.parametrize("K", [32, 64])
def test_proj_act_rows_stops_at_the_count(K, N, der):
    _check_counts("act", M0, N, K, der, 0, COUNTS)


@pytest.mark.parametrize("K", [32, 64])
def test_proj_act_rows_other_activation(K):
    """tanh (code 2): the generic-activation branch of the epilogue."""
    _check_counts("act", M0, 80, K, True, 2, COUNTS)


@pytest.mark.parametrize("kind,der", [("proj", False), ("act", False), ("act", True)])
def test_rows_with_a_wider_output_buffer(kind, der):
    """ldc > N: the outputs are column slices of a wider buffer, whose other columns stay untouched."""
    _check_counts(kind, M0, 80, 64, der, 0, COUNTS, pad=16)


@pytest.mark.parametrize("kind,K", [("proj", 64), ("act", 64), ("proj", 32)])
def test_rows_large_tiles(kind, K):
    """From 65536 rows the dispatchers pick the 256-row tiles (256 x 128 at K = 64, 256 x 64 at K = 32)."""
    _check_counts(kind, 65536, 16, K, False, 0, (65535 - 300, 70))


def test_null_rows_equal_the_old_entry_points():
    """tmdnet_proj_f32 / tmdnet_proj_act_f32 through the C ABI, with a device row count against rows = NULL (the
    uncounted launch): rows below the count are the same bits, rows at or past it are not written."""
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    lib = nat.load()
    M, N = M0, 80
    for K in (32, 64):
        A, dA, W, b = _operands(M, N, K)
        wp = kernels.proj_split(W)
        st = nat.stream(A.device)
        for c in (M, M - 37):
            rows = torch.tensor([c], dtype=torch.int32, device=DEV)
            old, _ = _filled(M, N)
            new, _ = _filled(M, N)
            common = (M, N, K, nat.ptr(A), K, nat.ptr(wp), N * K, nat.ptr(b))
            nat.check(lib.tmdnet_proj_f32(*common, nat.ptr(old), N, None, st), "tmdnet_proj_f32")
            nat.check(lib.tmdnet_proj_f32(*common, nat.ptr(new), N, nat.ptr(rows), st), "tmdnet_proj_f32")
            assert not bool((_bits(old) == SENTINEL).any())
            assert torch.equal(_bits(old)[:c], _bits(new)[:c]) and bool((_bits(new)[c:] == SENTINEL).all())
            for der in (False, True):
                outs = [[_filled(M, N)[0] for _ in range(2)] for _ in range(2)]
                common = (M, N, K, nat.ptr(A), nat.ptr(dA) if der else None, K, nat.ptr(wp), N * K, nat.ptr(b), 0)
                (So, Do), (Sn, Dn) = outs
                nat.check(lib.tmdnet_proj_act_f32(*common, nat.ptr(So), nat.ptr(Do) if der else None, N, None, st),
                          "tmdnet_proj_act_f32")
                nat.check(lib.tmdnet_proj_act_f32(*common, nat.ptr(Sn), nat.ptr(Dn) if der else None, N,
                                                  nat.ptr(rows), st), "tmdnet_proj_act_f32")
                assert torch.equal(_bits(So)[:c], _bits(Sn)[:c]) and torch.equal(_bits(Do)[:c], _bits(Dn)[:c])
                assert not bool((_bits(So) == SENTINEL).any())
                assert bool((_bits(Sn)[c:] == SENTINEL).all()) and bool((_bits(Dn)[c:] == SENTINEL).all())
                assert bool((_bits(Do) == SENTINEL).any()) != der


def test_rows_argument_checks():
    """The argument checks hold with a row count given; a misaligned count pointer is refused."""
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    lib = nat.load()
    A, dA, W, b = _operands(M0, 64, 64)
    wp = kernels.proj_split(W)
    out, _ = _filled(M0, 64)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = nat.stream(A.device)
    import ctypes
    odd = ctypes.c_void_p(rows.data_ptr() + 2)
    assert lib.tmdnet_proj_f32(M0, 64, 64, nat.ptr(A), 64, nat.ptr(wp), 64 * 64, nat.ptr(b), nat.ptr(out), 64,
                               odd, st) == kernels.GEMM_UNSUPPORTED
    assert lib.tmdnet_proj_f32(M0, 64, 48, nat.ptr(A), 64, nat.ptr(wp), 64 * 64, nat.ptr(b), nat.ptr(out), 64,
                               nat.ptr(rows), st) == kernels.GEMM_UNSUPPORTED
    assert lib.tmdnet_proj_act_f32(M0, 64, 64, nat.ptr(A), None, 64, nat.ptr(wp), 64 * 64, nat.ptr(b), 0,
                                   nat.ptr(out), nat.ptr(out), 64, nat.ptr(rows), st) != 0  # D without dA
    assert bool((_bits(out) == SENTINEL).all())  # nothing was launched
    with pytest.raises(RuntimeError):
        kernels.proj(A, W, b, rows=torch.zeros(1, dtype=torch.int64, device=DEV))
