"""The optional operands of the folded entry points, through the C ABI: a call that mixes "absent" and "present"
operands is refused with TMDNET_BAD_ARGUMENT before anything is launched (the outputs keep their sentinel), and
the same call with and without an optional operand gives the same bits on everything both calls write.

One tiny system throughout: 4 atoms in one molecule, cutoff 5, max_pairs 16, float32.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARGUMENT = 1
N, CAP, CUT, SLOTS = 4, 16, 5.0, (16 + 4) // 2
SENT = -7


def _pos():
    return torch.tensor([[0.0, 0.0, 0.0], [1.1, 0.2, 0.0], [0.3, 1.4, 0.5], [2.0, 1.0, 1.2]], device=DEV)


def _build(strategy="brute", pair_row=False, pair_edge=False, slots=0, num_rows=False):
    """One tmdnet_nl_build with every output pre-filled with SENT.  Returns (rc, outputs dict)."""
    from torchmdnet import _native as nat
    lib = nat.load()
    pos, batch = _pos(), torch.zeros(N, dtype=torch.long, device=DEV)
    st = {"brute": nat.NL_BRUTE, "cell": nat.NL_CELL}[strategy]
    box9 = (nat.D * 9)(3 * CUT, 0, 0, 0, 3 * CUT, 0, 0, 0, 3 * CUT) if strategy == "cell" else None
    ws = torch.empty(max(int(lib.tmdnet_nl_workspace_bytes(N, st, box9, CUT)), 16), dtype=torch.uint8, device=DEV)
    i32 = lambda *sh: torch.full(sh, SENT, dtype=torch.int32, device=DEV)  # noqa: E731
    f32 = lambda *sh: torch.full(sh, float(SENT), device=DEV)  # noqa: E731
    o = dict(neighbors=i32(2, CAP), deltas=f32(CAP, 3), distances=f32(CAP), num_pairs=i32(1), row_ptr=i32(N + 1),
             transpose=i32(CAP), pair_row=i32(CAP), pair_edge=i32(SLOTS), num_pair_rows=i32(1))
    rc = lib.tmdnet_nl_build(nat.F32, st, nat.ptr(pos), nat.ptr(batch), N, box9, 0, 0.0, CUT, CAP, 1, 1,
                             nat.ptr(o["neighbors"]), nat.ptr(o["deltas"]), nat.ptr(o["distances"]),
                             nat.ptr(o["num_pairs"]), nat.ptr(o["row_ptr"]), nat.ptr(o["transpose"]), 1, nat.ptr(ws),
                             ws.numel(), nat.ptr(o["pair_row"]) if pair_row else None,
                             nat.ptr(o["pair_edge"]) if pair_edge else None, slots,
                             nat.ptr(o["num_pair_rows"]) if num_rows else None, nat.stream(pos.device))
    torch.cuda.synchronize()
    return rc, o


def _untouched(o):
    return all(bool((t == SENT).all()) for t in o.values())


@pytest.mark.parametrize("kw", [dict(pair_edge=True),  # pair_row NULL, pair_edge given
                                dict(pair_row=True, pair_edge=True, slots=0),  # pairing without slots
                                dict(strategy="cell", pair_row=True, pair_edge=True, slots=SLOTS)],
                         ids=["edge_without_row", "no_slots", "cell"])
def test_nl_build_refuses_mixed_pair_operands(kw):
    rc, o = _build(**kw)
    assert rc == BAD_ARGUMENT and _untouched(o)


def test_nl_build_same_list_with_and_without_pairing():
    rc0, a = _build()
    rc1, b = _build(pair_row=True, pair_edge=True, slots=SLOTS, num_rows=True)
    assert rc0 == 0 and rc1 == 0
    assert int(a["num_pairs"]) == N * N  # every pair and the self loops are inside the cutoff
    for k in ("neighbors", "deltas", "distances", "num_pairs", "row_ptr", "transpose"):
        assert torch.equal(a[k], b[k]), k
    assert all(bool((a[k] == SENT).all()) for k in ("pair_row", "pair_edge", "num_pair_rows"))
    assert int(b["num_pair_rows"]) == (N * N + N) // 2


def _geom(o, rows=None, rbf_rows=False, drbf_rows=False):
    """tmdnet_edge_geom_fwd (num_rbf 16) on the list ``o``; outputs pre-filled with SENT."""
    from torchmdnet import _native as nat
    lib = nat.load()
    R, E = 16, N * N
    mu, beta = torch.linspace(0.0, 1.0, R, device=DEV), torch.full((R,), 2.0, device=DEV)
    f32 = lambda *sh: torch.full(sh, float(SENT), device=DEV)  # noqa: E731
    n_rows = 0 if rows is None else rows.shape[0]
    out = dict(rbf=f32(E, R), cutoff=f32(E), unit=f32(E, 3), rbf_rows=f32(5, R), drbf_rows=f32(5, R))
    rc = lib.tmdnet_edge_geom_fwd(nat.F32, E, R, nat.RBF_EXPNORM, nat.ptr(o["neighbors"][0]), nat.ptr(o["neighbors"][1]),
                                  nat.ptr(o["deltas"]), nat.ptr(o["distances"]), nat.ptr(mu), nat.ptr(beta), 0.0, CUT,
                                  nat.ptr(out["rbf"]), nat.ptr(out["cutoff"]), nat.ptr(out["unit"]), nat.ptr(rows),
                                  n_rows, nat.ptr(out["rbf_rows"]) if rbf_rows else None,
                                  nat.ptr(out["drbf_rows"]) if drbf_rows else None, nat.stream(mu.device))
    torch.cuda.synchronize()
    return rc, out


def test_edge_geom_fwd_row_operands():
    rc, o = _build()
    assert rc == 0
    o["neighbors"] = o["neighbors"].contiguous()
    rows = torch.tensor([0, 5, 6, 15, 9], dtype=torch.int32, device=DEV)
    rc, out = _geom(o, rows=rows)  # rows without rbf_rows
    assert rc == BAD_ARGUMENT and _untouched(out)
    rc, out = _geom(o, rbf_rows=True)  # rbf_rows without rows
    assert rc == BAD_ARGUMENT and _untouched(out)
    rc_a, a = _geom(o, rows=rows, rbf_rows=True)
    rc_b, b = _geom(o, rows=rows, rbf_rows=True, drbf_rows=True)
    assert rc_a == 0 and rc_b == 0
    for k in ("rbf", "cutoff", "unit", "rbf_rows"):
        assert torch.equal(a[k], b[k]) and not bool((a[k] == SENT).any()), k
    assert bool((a["drbf_rows"] == SENT).all()) and not bool((b["drbf_rows"] == SENT).any())


def test_dot_sum_fwd_with_and_without_atom_buf():
    """K = 16, 4 atoms, 1 molecule: the one-workgroup form (atom_buf NULL) against the row pass + run sum.  Both
    sum the same 4 per-atom values in fp32 in different orders; the bound is the one test_gpu_tn_kernels.py's
    test_dot_sum_matches_composite holds the forward to (1e-6 of the largest value)."""
    from torchmdnet import _native as nat
    lib = nat.load()
    g = torch.Generator(device=DEV).manual_seed(5)
    K = 16
    h, w, b0 = (torch.randn(*s, device=DEV, generator=g) for s in ((N, K), (K,), (1,)))
    batch = torch.zeros(N, dtype=torch.long, device=DEV)
    std, mean = torch.tensor([1.7], device=DEV), torch.tensor([-0.3], device=DEV)
    ys = []
    for buf in (None, torch.empty(N, device=DEV)):
        y = torch.full((1, 1), float(SENT), device=DEV)
        rc = lib.tmdnet_dot_sum_fwd(nat.F32, N, K, nat.ptr(h), K, nat.ptr(w), nat.ptr(b0), 1, nat.ptr(batch),
                                    nat.ptr(std), nat.ptr(mean), nat.ptr(buf), nat.ptr(y), nat.stream(h.device))
        assert rc == 0
        ys.append(y)
    ref = ((h.double() @ w.double() + b0.double()).sum() * 1.7 - 0.3).reshape(1, 1)
    print("dot_sum: one workgroup", float(ys[0]), "row pass", float(ys[1]), "fp64", float(ref))
    assert float((ys[0] - ys[1]).abs().max() / ys[1].abs().max()) < 1e-6
    assert float((ys[1].double() - ref).abs().max() / ref.abs().max()) < 1e-6
