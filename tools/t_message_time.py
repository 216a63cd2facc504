"""Times the scalar form of the ET message entry points (TMDNET_ET_SCALAR, csrc/t_message.hip: the invariant
Transformer's message) against the only native way to evaluate that message before it: the vector entry points on
v / pv widened to 3H with zero v1 | v2 blocks, vec_in NULL and unit zeros.

Input: the neighbour graph (cutoff 4.5, self loops, cell list) of the 50,001-atom periodic water box that
tools/prior_box_time.py builds (bench.tn_water_box_model's positions and box); H = 128, 8 heads, float32, pk and pv
present, per-edge inputs pair-symmetric.  Forward and first backward are timed separately, each launch between two
HIP events; WARMUP untimed launches of each arm, then REPEATS rounds in which the two arms alternate; medians.

Also records one model figure, no threshold: milliseconds per GraphedEnergyForces replay of the Transformer
(H = 128, 8 layers, 64 RBF, 8 heads) on bench's 32-molecule QM9-like batch.

usage (GPU box, repo root):
  python tools/t_message_time.py [--atoms 50001] [--repeats 20] [--out FILE]
Appends one JSON line to --out (default profiles/t_message_time.jsonl).  Condition: both ratios scalar / vector
are below 1 (bytes per edge predict about 0.5); the exit status is 1 otherwise."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

WARMUP = 3
H, HEADS = 128, 8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def arms(n, dev):
    from torchmdnet import _native as nat
    from torchmdnet import kernels
    _, _, pos, batch, L = bench.tn_water_box_model(n, False, 0, dev)
    box = torch.eye(3, dtype=pos.dtype) * L
    graph = kernels.build_graph(pos, batch, 0.0, 4.5, 64 * n, loop=True, strategy="cell", box=box)
    assert graph.symmetric
    N, E = graph.n_nodes, graph.n_edges
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    T = graph.transpose.long()
    rep = torch.minimum(torch.arange(E, device=dev), T)  # an edge and its reverse share their rows
    q, k, v, gx = rn(N, H), rn(N, H), rn(N, H), rn(N, H)
    pkv = rn(E, 2 * H)[rep]
    pk, pv = pkv[:, :H].contiguous(), pkv[:, H:].contiguous()
    C = torch.rand(E, generator=g).to(dev)[rep]
    d = H // HEADS

    def widen(t):
        w = torch.zeros(t.shape[0], HEADS, 3, d, device=dev)
        w[:, :, 0, :] = t.view(-1, HEADS, d)
        return w.view(t.shape[0], 3 * H)

    v3, pv3 = widen(v), widen(pv)
    u = torch.zeros(E, 3, device=dev)
    new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out, gq, gk, gv, gpk, gpv, gC = new(N, H), new(N, H), new(N, H), new(N, H), new(E, H), new(E, H), new(E)
    xo, vo, gv3, gpv3, gu, gvec = new(N, H), new(N, 3, H), new(N, 3 * H), new(E, 3 * H), new(E, 3), \
        torch.zeros(N, 3, H, device=dev)
    lib, P, st = nat.load(), nat.ptr, nat.stream(dev)
    common = (nat.F32, N, H, HEADS, P(graph.row_ptr), P(graph.src), E, P(q), H, P(k), H, P(v), H, None, P(pk), H,
              P(pv), H, P(C), None)

    def s_fwd():
        nat.check(lib.tmdnet_et_message_fwd(*common, P(out), None, nat.ET_SCALAR, None, None, st), "scalar fwd")

    def s_bwd():
        nat.check(lib.tmdnet_et_message_bwd(*common, P(gx), None, P(gq), P(gk), P(gv), None, P(gpk), P(gpv), P(gC),
                                            None, None, None, None, nat.ET_SCALAR, None, None, st), "scalar bwd")

    def v_fwd():
        kernels.et_message_fwd_launch(q, k, v3, None, pk, pv3, C, u, graph, HEADS, xo, vo)

    def v_bwd():
        kernels.et_message_bwd_launch(q, k, v3, None, pk, pv3, C, u, graph, HEADS, gx, gvec, gq, gk, gv3, None, gpk,
                                      gpv3, gC, gu)

    return dict(fwd=(s_fwd, v_fwd), bwd=(s_bwd, v_bwd)), N, E


def model_replay_ms(dev, repeats):
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_transformer_model
    args = bench.et_args(128)
    args.update(model="transformer", prior_model=None, embedding_dimension=128, num_layers=8, num_rbf=64,
                num_heads=8, derivative=True, precision=32)
    torch.manual_seed(0)
    model = create_transformer_model(args).to(dev)
    from oracle import model_oracle as O
    z, pos, batch = O.qm9_like(32)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    gm = GraphedEnergyForces(model, z, pos, batch)
    for _ in range(WARMUP):
        gm(pos)
    ms = [timed(lambda: gm(pos)) for _ in range(repeats)]
    gm.release()
    return statistics.median(ms), int(z.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--atoms", type=int, default=50001)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t_message_time.jsonl"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats: at least 20 timed launches")
    dev = torch.device("cuda", 0)
    forms, N, E = arms(a.atoms, dev)
    rec = dict(point="t_message_water_box", atoms=N, edges=E, hidden=H, heads=HEADS, dtype="float32",
               repeats=a.repeats, warmup=WARMUP, order="the two arms alternate within every round")
    for name, (scalar, vector) in forms.items():
        for _ in range(WARMUP):
            scalar()
            vector()
        torch.cuda.synchronize()
        ts, tv = [], []
        for _ in range(a.repeats):
            ts.append(timed(scalar))
            tv.append(timed(vector))
        rec[name] = dict(scalar_ms=round(statistics.median(ts), 4), vector_ms=round(statistics.median(tv), 4),
                         ratio=round(statistics.median(ts) / statistics.median(tv), 3))
    try:
        ms, atoms = model_replay_ms(dev, a.repeats)
        rec["model_replay"] = dict(workload="Transformer H 128, 8 layers, 64 RBF, 8 heads; 32-molecule QM9-like "
                                            "batch; GraphedEnergyForces replay, energy + forces", atoms=atoms,
                                   median_ms=round(ms, 4))
    except Exception as exc:  # the kernel record is written whatever becomes of the model figure
        rec["model_replay"] = dict(error=f"{type(exc).__name__}: {exc}")
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    return 0 if rec["fwd"]["ratio"] < 1 and rec["bwd"]["ratio"] < 1 else 1


if __name__ == "__main__":
    sys.exit(main())
