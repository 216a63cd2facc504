"""Times the graph network unoptimized and optimized (``torchmdnet.optimize.optimize``: the fused filter
convolution, csrc/cfconv_fused.hip) in one process, by the protocol of DESIGN.md §3j: float32, embedding 128,
6 layers, 50 RBFs, fixed basis, Scalar head, aggr=add; 10 warm-up calls, then 15 timed windows, reported as median
(min-max) in microseconds per energy + force evaluation.

  * QM9-scale point: the 32-molecule QM9-like batch of bench.py (678 atoms): ``GraphedEnergyForces`` replays
    (200 per window) and eager calls (20 per window);
  * large-system point: a non-periodic cluster at liquid-water density (0.1 atoms / A^3, a jittered cubic
    lattice, >= 20,000 atoms): single eager evaluations (1 per window) and ``torch.cuda.max_memory_allocated``.

usage (GPU box, repo root):
  python tools/gn_optimize_time.py [--side 28] [--skip-large] [--skip-small]
  python tools/gn_optimize_time.py --trace-evals 30 [--plain]     # only N eager QM9-scale evaluations: the
      workload of a separate `rocprofv3 --kernel-trace --stats -- python tools/gn_optimize_time.py ...` run
Prints one JSON object per measurement."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

import torch  # noqa: E402

import bench  # noqa: E402

WARMUP, WINDOWS = 10, 15


def gn_args(max_num_neighbors=32):
    args = bench.et_args(128)
    args.update(model="graph-network", num_layers=6, num_rbf=50, trainable_rbf=False, aggr="add",
                max_num_neighbors=max_num_neighbors)
    return args


def models(args, dev):
    from torchmdnet.models.model import create_model
    from torchmdnet.optimize import optimize
    torch.manual_seed(0)
    plain = create_model(args)
    fused = optimize(copy.deepcopy(plain))
    return plain.to(dev), fused.to(dev)


def windows(fn, per_window):
    """median (min, max) microseconds per call over WINDOWS windows of per_window calls, host-timed around a
    device synchronisation."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(per_window):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / per_window * 1e6)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def report(**kw):
    print(json.dumps(kw), flush=True)


def small(dev):
    from torchmdnet.graphs import GraphedEnergyForces
    z, pos, batch = (t.to(dev) for t in bench.qm9_like(32, gen_seed=1))
    pos = pos.float()
    plain, fused = models(gn_args(), dev)
    ref = None
    for name, m in (("unoptimized", plain), ("optimized", fused)):
        y, f = m(z, pos.clone(), batch)
        if ref is None:
            ref = f.detach()
        edges = int(m.representation_model.distance.graph(pos, batch).num_pairs)
        report(point="qm9", model=name, atoms=int(z.numel()), edges=edges, mode="eager",
               max_force_diff_vs_unoptimized=float((f.detach() - ref).abs().max()),
               **windows(lambda: m(z, pos.clone(), batch), 20))
        gm = GraphedEnergyForces(m, z, pos, batch)
        report(point="qm9", model=name, atoms=int(z.numel()), edges=edges, mode="graph replay",
               **windows(lambda: gm(), 200))
        gm.check_capacity()
        gm.release()


def cluster(side, dev):
    """side^3 atoms on a cubic lattice of 0.1 atoms / A^3 (liquid water: 0.0334 molecules / A^3), each moved
    by up to 0.35 A per axis; O, H, H in turn."""
    a = (1.0 / 0.1) ** (1.0 / 3.0)
    gen = torch.Generator().manual_seed(4)
    idx = torch.arange(side, dtype=torch.float32)
    grid = torch.stack(torch.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3) * a
    pos = grid + 0.7 * (torch.rand(grid.shape, generator=gen) - 0.5)
    z = torch.tensor([8, 1, 1]).repeat(pos.shape[0] // 3 + 1)[:pos.shape[0]]
    return z.to(dev), pos.to(dev), torch.zeros(pos.shape[0], dtype=torch.long, device=dev)


def large(side, dev):
    z, pos, batch = cluster(side, dev)
    plain, fused = models(gn_args(max_num_neighbors=96), dev)
    ref = None
    for name, m in (("unoptimized", plain), ("optimized", fused)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y, f = m(z, pos.clone(), batch)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        if ref is None:
            ref = f.detach().clone()
        edges = int(m.representation_model.distance.graph(pos, batch).num_pairs)
        diff = float((f.detach() - ref).abs().max())
        del y, f
        report(point="cluster", model=name, atoms=int(z.numel()), edges=edges, mode="eager",
               peak_mb=round(peak / 2 ** 20, 1), resident_before_mb=round(base / 2 ** 20, 1),
               max_force_diff_vs_unoptimized=diff, max_force=float(ref.abs().max()),
               **windows(lambda: m(z, pos.clone(), batch), 1))


def trace(n, use_plain, dev):
    z, pos, batch = (t.to(dev) for t in bench.qm9_like(32, gen_seed=1))
    pos = pos.float()
    plain, fused = models(gn_args(), dev)
    m = plain if use_plain else fused
    for _ in range(n):
        m(z, pos.clone(), batch)
    torch.cuda.synchronize()
    report(point="qm9", model="unoptimized" if use_plain else "optimized", mode="trace workload", evaluations=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", type=int, default=28, help="lattice side of the cluster (28^3 = 21,952 atoms)")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--trace-evals", type=int, default=0)
    ap.add_argument("--plain", action="store_true", help="with --trace-evals: the unoptimized model")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.trace_evals:
        return trace(a.trace_evals, a.plain, dev)
    if not a.skip_small:
        small(dev)
    if not a.skip_large:
        large(a.side, dev)


if __name__ == "__main__":
    main()
