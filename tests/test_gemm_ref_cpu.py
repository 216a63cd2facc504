"""CPU checks of tests/gemm_ref.py: the exact mode's magnitude bound for every case in the tables, the restated
launch rules of csrc/gemm.hip (which k_gemm / k_gemm_x3 / TN form each case reaches -- the claim the GPU tests'
coverage rests on), the references against plain loops, and the builders' padding."""
import ctypes
import itertools

import pytest
import torch

import gemm_ref as R


def _dense_specs():
    specs = R.ladder_specs() + R.edge_specs(32) + R.edge_specs(272)
    for g in R.GROUPS.values():
        specs += list(g)
    for c in R.EPI_GROUPED + R.EPI_X3:
        specs += R.option_subsets(*c)
    specs += R.x3_ladder_specs() + R.x3_edge_specs(96) + R.x3_edge_specs(160)
    specs.append(R.Spec(*R.X3_WIDE, 1, bias=1))
    return specs


def _tn_specs():
    specs = [s for K in R.TN_K for s in R.tn_edge_specs(K)] + list(R.TN_EMPTY)
    specs += R.tn_group_specs(33) + [R.TNSpec(*R.TN_LONG, ones=1)]
    return specs


def test_exact_mode_magnitudes_stay_below_2_24():
    """Every exact-mode sum is an integer below 2**24 in magnitude, so fp32 holds it under any summation order;
    the integers -3 .. 3 and the row scales are exact in the first bf16 piece (8 significant bits)."""
    for s in _dense_specs():
        assert R.exact_bound(s.K) * 2 < 2 ** 24, s  # (* 2: the largest row scale)
    for s in _tn_specs():
        assert R.exact_bound(s.K, s.K2) < 2 ** 24, s
    assert R.exact_bound(R.EMB_N[-1]) < 2 ** 24
    for v in list(range(-R.INT_MAX, R.INT_MAX + 1)) + [0.5, 2.0]:
        t = torch.tensor(float(v))
        assert float(t.to(torch.bfloat16)) == v


def test_exact_mode_sums_reach_no_more_than_the_bound():
    for s in (R.Spec(37, 70, 2048, 1, bias=1, beta=1), R.Spec(33, 17, 48, 0, bias=1, beta=1, pre=1, rscale=1)):
        o = R.build(s, "exact", "cpu")
        c, pre = R.reference(s, o)
        assert float(pre.abs().max()) <= R.exact_bound(s.K)
        assert torch.equal(pre.float().double(), pre) and torch.equal(c.float().double(), c)
        for k in ("A", "B", "bias", "C0"):
            v = o[k]
            assert torch.equal(v, v.round()) and float(v.abs().max()) <= R.INT_MAX
        if s.rscale:
            assert set(o["rscale"].tolist()) <= {0.5, 1.0, 2.0}


def test_k_ladder_reaches_every_default_grouped_form():
    forms = {K: R.grouped_form(K) for K in R.K_LADDER}
    assert {f[:2] for f in forms.values()} == R.DEFAULT_FORMS
    # the first K of each form named in the kernel's dispatch
    assert forms[16][:2] == forms[128][:2] == (4, 1)
    assert forms[144][:2] == forms[240][:2] == (4, 4)
    assert forms[256][:2] == (16, 1) and forms[272][:2] == forms[512][:2] == (16, 2)
    assert forms[528][:2] == forms[768][:2] == (16, 3) and forms[784][:2] == forms[1024][:2] == (16, 4)
    # a slice longer than the load batch: a partial last batch (5 = 4 + 1) and two full ones
    assert forms[1040] == (16, 4, 5) and forms[1280] == (16, 4, 5) and forms[2048] == (16, 4, 8)
    # 15 of 16 waves idle: K = 16 in a launch whose longest K is >= 256
    g = R.GROUPS["as_listed"]
    assert R.grouped_form(max(s.K for s in g))[0] == 16 and min(s.K for s in g) == 16
    assert R.grouped_form(max(s.K for s in R.GROUPS["all_below_256"]))[0] == 4


def test_env_switches_reach_the_other_grouped_forms():
    """The two child processes of test_gpu_gemm_edges.test_env_only_forms: TMDNET_GEMM_NW=8,2 and
    TMDNET_GEMM_NW=4,8 with TMDNET_GEMM_KB4=2.  (k_gemm<8,8> needs more than two blocks per wave on 8 waves,
    that is K >= 272 on the large side of the switch: "8,2" alone cannot reach it.)"""
    a = {R.grouped_form(K, 8, 2)[:2] for K in R.K_LADDER}
    b = {R.grouped_form(K, 4, 8, kb4=2)[:2] for K in R.K_LADDER}
    assert a == {(8, 2), (2, 8)}
    assert b == {(4, 2), (4, 4), (8, 2), (8, 8)}


def test_x3_cases_cover_tile_widths_grids_and_remap():
    seen = {}
    for s in R.x3_ladder_specs() + R.x3_edge_specs(96) + R.x3_edge_specs(160) + [R.Spec(*R.X3_WIDE, 1)]:
        bn, nx, ny, remap = R.x3_form(s.M, s.N)
        seen.setdefault((bn, nx * ny, remap), s)
    T = {t for _, t, _ in seen}
    assert {1, 4, 15} <= T
    assert any(remap and t % 8 for _, t, remap in seen)  # the XCD remap with T % 8 != 0
    assert R.x3_form(*R.X3_WIDE[:2]) == (128, 2, 1024, True)  # the wide 128-column form
    assert R.x3_form(129, 272) == (64, 5, 2, True) and R.x3_form(129, 80) == (128, 1, 2, False)
    assert R.x3_form(300, 272)[1:3] == (5, 3) and R.x3_form(129, 144) == (128, 2, 2, True)
    # partial 16-column blocks in both tile widths: N % 64 != 0 at BN = 64, N % 128 != 0 at BN = 128
    assert R.x3_form(1, 16)[0] == R.x3_form(1, 48)[0] == 64 and R.x3_form(1, 272)[0] == 64
    assert R.x3_form(1, 80)[0] == R.x3_form(1, 144)[0] == 128
    # fewer k-steps than the prefetch ring of the 128-column form (PD = 4), and a wrap with a remainder
    assert 32 // 32 < 4 and (160 // 32) % 4 and (288 // 32) % 4


def test_long_k_problem_is_unsplit():
    M, Nb, K = R.TN_LONG
    S, nt, parts = R.tn_plan_v([(M, Nb, K)])
    assert (S, nt, parts) == ([1], [1024], 0)
    assert R.tn_split(((M + 31) // 32) * ((Nb + 1 + 31) // 32), K) == 1
    assert R.tn_workspace_bytes([(M, Nb + 1, K, 0, True)]) == 0
    assert R.tn_form(M, Nb, K, ones=True, tn_v=1)[0] == "v<8>"
    assert R.tn_form(M, Nb, K, ones=True, tn_v=2)[0] == "v2<8,4>"
    assert R.tn_form(M, Nb, K, ones=True, aligned=False)[0] == "tn<16>"


def test_tn_cases_reach_the_forms_claimed():
    # embedding gradients pass no workspace: 8-wave / 16-wave forms from 8192 atoms on
    for n, eight in ((8191, False), (8192, True), (8200, True)):
        assert R.tn_form(R.EMB_TYPES, 32, n, ws=False)[0] == ("v2<8,2>" if eight else "v2<4,2>")
        assert R.tn_form(R.EMB_TYPES, 64, n, ws=False)[0] == ("v<8>" if eight else "v<4>")
        assert R.tn_form(R.EMB_TYPES, 33, n, ws=False, aligned=False)[0] == ("tn<16>" if eight else "tn<4>")
    # the edge grid: unsplit at K = 15 .. 17, split (partial tiles + the reduce kernels) at K = 600
    for M, Nb in itertools.product(R.TN_M, R.TN_NB):
        for K in (15, 16, 17):
            assert R.tn_form(M, Nb, K)[2] == 1 and R.tn_form(M, Nb, K, aligned=False)[2] == 1
        assert R.tn_form(M, Nb, 600)[2] > 1 and R.tn_form(M, Nb, 600, aligned=False)[2] > 1
    # narrow / non-narrow at Nb = 32 / 33
    assert R.tn_form(64, 32, 600)[0] == "v2<4,2>" and R.tn_form(64, 33, 600)[0] == "v<4>"
    assert R.tn_form(64, 33, 600, tn_v=2)[0] == "v2<4,4>" and R.tn_form(64, 32, 600, tn_v=1)[0] == "v<4>"


def test_workspace_restatement_matches_the_library():
    """tmdnet_gemm_tn_workspace_bytes is host code (no GPU): the restated plan gives its byte counts."""
    from torchmdnet import _native
    lib = _native.load()
    cases = [[(M, Nb + ones, K, K2, ones)] for M, Nb, K, K2, ones in
             itertools.product((63, 65, 2048), (31, 33, 64, 2048), (0, 17, 600, 8192, 40000), (0, 37), (0, 1))]
    cases.append([(s.M, s.Nb + int(bool(s.ones or s.ones2)), s.K, s.K2, int(bool(s.ones or s.ones2)))
                  for s in R.tn_group_specs(32)])
    for probs in cases:
        dims = (ctypes.c_int * (12 * len(probs)))()
        for i, (M, N, K, K2, ones) in enumerate(probs):
            dims[12 * i:12 * i + 12] = [M, N, K, K2, M, N, M, N, N, 0, ones, ones if K2 else 0]
        want = lib.tmdnet_gemm_tn_workspace_bytes(len(probs), dims)
        assert R.tn_workspace_bytes(probs) == want, (probs[0], len(probs))


def _loop_gemm(A, B, tb):
    M, K = A.shape
    N = B.shape[0] if tb else B.shape[1]
    out = torch.zeros(M, N, dtype=torch.float64)
    for i in range(M):
        for j in range(N):
            for k in range(K):
                out[i, j] += float(A[i, k]) * float(B[j, k] if tb else B[k, j])
    return out


@pytest.mark.parametrize("tb", [1, 0])
def test_reference_states_the_epilogue_order(tb):
    s = R.Spec(3, 5, 16, tb, 1, 1, 1, 1, 1, 1)
    o = R.build(s, "random", "cpu", seed=3)
    c, pre = R.reference(s, o)
    v = _loop_gemm(o["A"], o["B"], tb) + o["bias"].double() + o["C0"].double()
    assert torch.allclose(pre, v, rtol=0, atol=1e-12)
    x = o["dpre"].double()
    sg = 1 / (1 + torch.exp(-x))
    want = v / (1 + torch.exp(-v)) * o["rscale"].double()[:, None] * (sg + x * sg * (1 - sg))
    assert torch.allclose(c, want, rtol=0, atol=1e-12)
    # silu' against autograd
    xr = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(torch.nn.functional.silu(xr).sum(), xr)
    assert torch.allclose(R.dsilu(x), g, rtol=0, atol=1e-14)
    # each term is honoured alone: turning it off changes the result (pre is an output, not a term)
    for opt in R.OPTIONS:
        if opt == "pre":
            continue
        s2 = s._replace(**{opt: 0})
        c2, _ = R.reference(s2, o)
        assert not torch.equal(c2, c), opt


def test_builders_pad_with_nan_and_sentinel():
    s = R.Spec(5, 17, 32, 1, 1, 1, 1, 0, 1, 1)
    for x3 in (False, True):
        for tb in (1, 0):
            o = R.build(s._replace(tb=tb), "random", "cpu", x3=x3)
            A, B, C, pre, dpre = o["A"], o["B"], o["C"], o["pre"], o["dpre"]
            assert A.stride(0) == s.K + 4 and C.stride(0) == s.N + (8 if x3 else 5)
            assert B.stride(0) == (s.K + 8 if tb else s.N + (8 if x3 else 3))
            assert pre.stride(0) == dpre.stride(0) == s.N + 12 != C.stride(0)
            for t in (A, B, dpre):
                base = t._base
                assert base.shape[0] == t.shape[0] + 2 and not bool(t.isnan().any())
                assert int(base.isnan().sum()) == base.numel() - t.numel()
            assert R.padding_untouched(o["Cbuf"], s.M, s.N) and R.padding_untouched(o["prebuf"], s.M, s.N)
            assert torch.equal(C, o["C0"])  # beta: C starts as C0
            o["Cbuf"][s.M, 0] = 0.0
            assert not R.padding_untouched(o["Cbuf"], s.M, s.N)
    o = R.build(s._replace(beta=0), "exact", "cpu")
    assert bool((o["Cbuf"] == R.SENT).all())  # without beta the kernel must overwrite every element


def test_tn_reference_and_builder():
    s = R.TNSpec(5, 3, 7, 4, ones=1, ones2=0, cb=1, beta=1)
    o = R.build_tn(s, "exact", "cpu")
    p = o["p"]
    c, cb = R.reference_tn(o)
    want = torch.zeros(5, 3, dtype=torch.float64)
    wb = torch.zeros(5, dtype=torch.float64)
    for k in range(7):
        want += p["A"][k].double()[:, None] * p["B"][k].double()[None, :]
        wb += p["A"][k].double()
    for k in range(4):
        want += p["A2"][k].double()[:, None] * p["B2"][k].double()[None, :]
    assert torch.equal(c, want + o["C0"].double()) and torch.equal(cb, wb + o["Cb0"].double())
    assert p["A"].stride(0) % 4 == 0 and p["B"].stride(0) % 4 == 0 and p["C"].stride(0) == 3 + 5
    assert bool(p["A"]._base.isnan().any()) and bool((o["Cbbuf"][5:] == R.SENT).all())
    # the ones column inside C, a second segment without it, a device row count, misaligned strides
    s = R.TNSpec(5, 3, 7, 4, ones=1, ones2=0)
    o = R.build_tn(s, "exact", "cpu", aligned=False)
    c, cb = R.reference_tn(o)
    assert cb is None and c.shape == (5, 4) and torch.equal(c[:, 3], o["p"]["A"].double().sum(0))
    assert o["p"]["A"].stride(0) % 2 == 1 and o["p"]["B"].stride(0) % 2 == 1
    c0, _ = R.reference_tn(o, rows=0)
    assert not bool(c0.any())
    # empty sums
    for s in R.TN_EMPTY:
        o = R.build_tn(s, "exact", "cpu")
        if s.K2 == 0:
            c, cb = R.reference_tn(o)
            assert torch.equal(c, o["C0"].double() if s.beta else torch.zeros_like(c))


def test_embedding_builder_and_reference():
    z, grad, out0 = R.build_embedding(300, 33, "exact", "cpu")
    assert R.EMB_ABSENT not in set(z.tolist()) and int(z.max()) == R.EMB_TYPES - 1 and int(z.min()) == 0
    assert grad.stride(0) % 4 != 0 and R.build_embedding(300, 32, "exact", "cpu")[1].stride(0) == 36
    ref = R.reference_embedding(z, grad, out0, False)
    assert not bool(ref[R.EMB_ABSENT].any())
    want = torch.zeros(R.EMB_TYPES, 33, dtype=torch.float64)
    for k in range(300):
        want[int(z[k])] += grad[k].double()
    assert torch.equal(ref, want)
    assert torch.equal(R.reference_embedding(z, grad, out0, True), want + out0.double())


def test_bar_and_digest():
    assert R.within_bar(2e-6, 1e-6, 0.0) and not R.within_bar(2.1e-6, 1e-6, 0.0)
    assert R.within_bar(4 * R.ULP, 0.0, 1.0) and not R.within_bar(4.1 * R.ULP, 0.0, 1.0)
    assert R.within_bar(3e-6, 1e-6, 0.0, factor=3.0)
    a = torch.arange(6.0).reshape(2, 3)
    assert R.digest([a]) == R.digest([a.clone()]) != R.digest([a + 1])
    assert R.max_abs_err(a, a.double() + 0.5, chunk=1) == 0.5
