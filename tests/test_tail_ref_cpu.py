"""tests/tail_ref.py against float64 autograd of F.layer_norm, index_add and F.mse_loss (first order; LayerNorm to
second order), to 1e-10 of each output's largest value, and its input makers for the conditions
tests/test_gpu_tail_widths.py relies on: the exact family is exact, an out-of-range batch has ids on both sides, a
batch with empty molecules has one."""
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R

F32, F64 = torch.float32, torch.float64
EPS = 1e-5


def _close(a, ref, what):
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err, top = float((a - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max|d| = {err:.3e}, max|ref| = {top:.3e}")
    assert err <= 1e-10 * top, (what, err, top)


LN_CASES = [(5, 100, 0.0), (3, 1, 0.0), (4, 65, 0.0), (4, 65, 1000.0)]


@pytest.mark.parametrize("rows,C,offset", LN_CASES, ids=[f"{r}x{c}+{int(o)}" for r, c, o in LN_CASES])
def test_layer_norm_restatement_against_autograd(rows, C, offset):
    x, w, b, gy, X, Wb, Bb = (t.double() for t in R.ln_inputs(rows, C, offset=offset))
    xs, ws, bs, gs = (t.clone().requires_grad_(True) for t in (x, w, b, gy))
    y = F.layer_norm(xs, (C,), ws, bs, EPS)
    gx, gw, gb = torch.autograd.grad(y, (xs, ws, bs), gs, create_graph=True)
    yr, mean, rstd = R.ln_fwd(x, w, b, EPS)
    _, mean_a, rstd_a = torch.native_layer_norm(x, [C], w, b, EPS)
    _close(yr, y, "y")
    _close(mean, mean_a.reshape(-1), "mean")
    _close(rstd, rstd_a.reshape(-1), "rstd")
    for name, a, ref in zip(("gx", "gw", "gb"), R.ln_bwd(x, w, mean, rstd, gy), (gx, gw, gb)):
        if C == 1 and name != "gb":  # one value per row: xhat = 0, so gx = 0 and gw = 0 identically; autograd
            scale = float((gy * w).abs().max() * rstd.max())  # leaves rounding noise of the terms that cancel
            assert not bool(a.any()) and float(ref.detach().abs().max()) <= 1e-10 * scale
            continue
        _close(a, ref, name)
    # second order: every subset of cotangents with one left out, and all three
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)):
        cot = [t if u else None for t, u in zip((X, Wb, Bb), use)]
        l2 = sum((g * c).sum() for g, c in zip((gx, gw, gb), cot) if c is not None)
        ref = torch.autograd.grad(l2, (gs, xs, ws), retain_graph=True, allow_unused=True)
        d_gy, d_x, d_w, T = R.ln_bwd2(x, w, mean, rstd, gy, *cot)
        for name, a, r in zip(("d_gy", "d_x", "d_w"), (d_gy, d_x, d_w), ref):
            if r is None or C == 1 and name != "d_gy":
                assert float(a.abs().max()) < 1e-9, (name, use)
                continue
            _close(a, r, f"{name} {use}")
        if cot[0] is not None and C > 1:  # T is ln_bwd's gx for G = X: the same projection
            _close(T, R.ln_bwd(x, torch.ones_like(w), mean, rstd, X)[0], "T")


@pytest.mark.parametrize("n,n_mol,kind", [(50, 7, "shuffled"), (50, 7, "range"), (50, 7, "empty"), (0, 3, "sorted")])
def test_molecule_sum_restatements_against_index_add(n, n_mol, kind):
    h, w, b0, batch, std, mean = R.dot_case("random", n, 5, n_mol, kind, F64)
    on = (batch >= 0) & (batch < n_mol)
    safe = batch.clamp(0, n_mol - 1)
    hs, ws, bs = (t.clone().requires_grad_(True) for t in (h, w, b0))
    rows = (hs @ ws + bs) * on  # dropped ids contribute nothing
    y = torch.zeros(n_mol, dtype=F64).index_add(0, safe, rows * std) + mean
    _close(R.dot_sum(h, w, b0, batch, n_mol, std, mean), y, "dot_sum")
    _close(R.atom_sum(h[:, 0], batch, n_mol, std, mean),
           torch.zeros(n_mol, dtype=F64).index_add(0, safe, h[:, 0] * on * std) + mean, "atom_sum")
    _close(R.atom_sum(h[:, 0], batch, n_mol, None, None),
           torch.zeros(n_mol, dtype=F64).index_add(0, safe, h[:, 0] * on), "atom_sum, no std / mean")
    _close(R.dot_sum(h, w, None, batch, n_mol, std, None),
           torch.zeros(n_mol, dtype=F64).index_add(0, safe, (h @ w) * on * std), "dot_sum, no b0 / mean")
    if n:
        gy = torch.randn(n_mol, dtype=F64)
        gh, = torch.autograd.grad(y, hs, gy)
        _close(R.dot_sum_bwd(gy, batch, n_mol, std, w), gh, "dot_sum_bwd")
        assert not bool(R.dot_sum_bwd(gy, batch, n_mol, std, w)[~on].any())
        _close(R.dot_rows(h, w, b0), hs @ ws + bs, "dot_rows")


@pytest.mark.parametrize("n1,n2", [(5, 9), (9, 5), (0, 4), (4, 0), (0, 0)])
def test_mse2_restatement_against_mse_loss(n1, n2):
    a1, b1, a2, b2 = R.loss_inputs("random", n1, n2, F64)
    w1, w2, g = 0.75, 1.25, 3.0
    s1, s2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
    loss = sum(w * F.mse_loss(a, b) for w, a, b in ((w1, s1, b1), (w2, s2, b2)) if a.numel())
    got = R.mse2(a1, b1, w1, a2, b2, w2)
    if n1 + n2 == 0:
        assert got == 0.0
        return
    _close(torch.tensor(got, dtype=F64), loss, "mse2")
    ref = torch.autograd.grad(loss, (s1, s2), torch.tensor(g, dtype=F64), allow_unused=True)
    for name, a, r, n in zip(("d1", "d2"), R.mse2_bwd(a1, b1, w1, a2, b2, w2, g), ref, (n1, n2)):
        assert a.shape == (n,)
        if n:
            _close(a, r, name)


# ----------------------------------------------------------------------------- the input makers
def test_exact_family_sums_are_exact_in_any_order():
    """Every exact case of the GPU tests: the values sit on the grid, the per-molecule sums of magnitudes stay
    below 2^22, and a float32 running sum in a random permutation equals the float64 sum bit for bit."""
    g = torch.Generator().manual_seed(5)
    count = 0
    for name, h, w, b0, batch, n_mol in R.exact_sum_cases():
        assert R.exact_headroom(h, w, b0, batch, n_mol) < 1.0, name
        count += 1
        if len(batch) == 0:
            continue
        terms = h.reshape(len(batch), -1) * (1 if w is None else w)  # float32 products, exact
        if b0 is not None:
            terms = torch.cat([terms, b0.expand(len(batch), 1)], 1)
        assert terms.dtype == F32
        for b in sorted(set(batch.tolist()) & set(range(n_mol)))[:3]:
            t = terms[batch == b].reshape(-1)
            t = t[torch.randperm(t.numel(), generator=g)]
            run = torch.cumsum(t, 0, dtype=F32)  # every partial sum, sequentially rounded to float32
            ref = torch.cumsum(t.double(), 0)
            assert torch.equal(run.double(), ref), name
            assert float(t.sum(dtype=F32)) == float(t.double().sum()), name
    assert count == len(R.ATOM_SUM_CASES) + 1 + len(R.DOT_CASES) + len(R.DOT_ROUTE)
    for n1, n2 in R.LOSS_PAIRS:  # integer differences: both sums of squares exact
        for a, b in zip(*[iter(R.loss_inputs("exact", n1, n2, F32))] * 2):
            sq = (a - b) ** 2
            sq = sq[torch.randperm(sq.numel(), generator=g)]
            assert torch.equal(torch.cumsum(sq, 0, dtype=F32).double(), torch.cumsum(sq.double(), 0))
            assert float(sq.double().sum()) < 2.0 ** 24


def test_batches_hold_what_their_kind_promises():
    cases = {(n, m, k) for n, m, k in R.ATOM_SUM_CASES + R.SUM_BWD_CASES + (R.CEILING_CASE,)}
    cases |= {(n, m, k) for n, _, m, k in R.DOT_CASES + R.DOT_ROUTE}
    seen = set()
    for n, m, kind in sorted(cases):
        batch = R.make_batch(kind, n, m)
        assert batch.shape == (n,) and batch.dtype == torch.int64
        seen.add(kind)
        if kind in ("sorted", "empty"):
            assert bool((batch[1:] >= batch[:-1]).all())
            assert n == 0 or (int(batch.min()) >= 0 and int(batch.max()) < m)
        if kind == "sorted" and n >= m:
            assert not R.has_empty(batch, m), (n, m)
        if kind == "empty" and n:
            assert m >= 3 and R.has_empty(batch, m), (n, m)
            assert 0 not in batch.tolist() and m - 1 not in batch.tolist()  # the first and the last bin stay empty
        if kind in ("shuffled", "range") and n > 64 and m > 1:
            assert not bool((batch[1:] >= batch[:-1]).all())
        if kind == "range" and n >= 2:  # (one atom cannot be out of range on both sides)
            assert int((batch < 0).sum()) >= 1 and int((batch >= m).sum()) >= 1, (n, m)
            assert int(((batch >= 0) & (batch < m)).sum()) >= 1 or n < 3
    assert seen == set(R.BATCH_KINDS)
    assert R.MAX_MOLECULES == 8192 and not R.has_empty(R.make_batch(*R.CEILING_CASE[2:], *R.CEILING_CASE[:2]), 8192)


def test_loss_pairs_cover_what_the_issue_lists():
    ps = set(R.LOSS_PAIRS)
    assert all((0, n) in ps and (n, 0) in ps for n in R.LOSS_SIZES)
    assert (1, 3000) in ps and (3000, 1) in ps
    assert 20 <= len(ps) <= 30
    assert {n for p in ps for n in p} == set(R.LOSS_SIZES)


def test_launch_arithmetic_restated():
    assert [R.ln_cpl(C) for C in (1, 128, 129, 256, 257, 384, 385, 512, 513, 1024)] == [2, 2, 4, 4, 6, 6, 8, 8, 16, 16]
    assert [R.wgrad_chunk(r) for r in (1, 16, 17, 4096, 4097, 4100)] == [16, 16, 16, 16, 17, 17]
    assert 4097 == 17 * 241 and 4100 % 17 == 3  # 4097 rows: 241 whole chunks of 17; 4100: a final chunk of 3
