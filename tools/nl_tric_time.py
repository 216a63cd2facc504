"""Times the neighbour-list build of a large periodic system in a rectangular and in a triclinic box
(csrc/neighbors.hip: the cell strategy's rectangular and fractional-coordinate forms, and the all-pairs
`shared` strategy a triclinic box had to take before), and the ET water-box energy + force evaluation of
bench.py's `secondary_water_box` re-boxed into the triclinic cell.

Protocol: float32, N atoms (default 50,001) at water density 0.1003 / A^3, cutoff 5; every build through
kernels.neighbor_pairs_raw (symmetric list with self pairs, CSR rows and transpose map, padded); WARMUP
untimed calls, then REPEATS calls each between two HIP events recorded on the launching stream; reported as
median (min-max) in microseconds.

  (a) cell, cubic box of side L = (N / 0.1003)^(1/3)
  (b) cell, the box (L, 0, 0), (L/2, L, 0), (L/2, L/2, L): the same volume, the extreme skew validate_box admits
  (c) shared, box (b)
  ET: 128 channels, 8 layers, cutoff 5, max_num_neighbors 128, eager energy + forces in box (b), cell and shared.

usage (GPU box, repo root):  python tools/nl_tric_time.py [--atoms 50001] [--builds abc] [--skip-model] [--out FILE]
(--atoms 51354 gives L = 80.0: a cubic box of 16 whole cutoff-wide cells, no partial top cell)
Prints one JSON object per configuration and appends it to --out (default profiles/nl_tric_time.jsonl)."""
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

WARMUP, REPEATS = 5, 25
CUTOFF = 5.0
DENSITY = 0.1003


def event_times(fn, warmup, repeats):
    """microseconds of each of ``repeats`` calls, by HIP events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
            "repeats": len(us)}


def boxes(n):
    L = (n / DENSITY) ** (1.0 / 3.0)
    rect = torch.eye(3, dtype=torch.float64) * L
    tric = torch.tensor([[L, 0.0, 0.0], [L / 2, L, 0.0], [L / 2, L / 2, L]], dtype=torch.float64)
    return L, rect, tric


def positions(n, box, seed, dev):
    g = torch.Generator().manual_seed(seed)
    frac = torch.rand(n, 3, generator=g, dtype=torch.float64)
    return (frac @ box).float().to(dev)


def build_point(label, strategy, box, n, dev, sink, repeats=REPEATS, warmup=WARMUP):
    from torchmdnet import kernels
    pos = positions(n, box, 7, dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    cap = n * 96
    b32 = box.float()

    def run():
        return kernels.neighbor_pairs_raw(strategy, pos, batch, b32, True, 0.0, CUTOFF, cap, True, True,
                                          pad_output=True, want_csr=True)
    num = int(run()[3].item())
    assert num <= cap, (num, cap)
    rec = dict(point="build", config=label, strategy=strategy, atoms=n, cutoff=CUTOFF, pairs=num,
               box=[[round(v, 3) for v in row] for row in box.tolist()], **stats(event_times(run, warmup, repeats)))
    sink(rec)
    return num


def model_point(label, strategy, box, n, dev, sink):
    from torchmdnet.models.model import create_model
    args = bench.et_args(128)
    args.update(max_num_neighbors=128)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    pos = positions(n, box, 7, dev)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3 + 1)[:n].to(dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    d = model.representation_model.distance
    d.box = box.float()
    d.use_periodic = True
    d.strategy = strategy
    us = event_times(lambda: model(z, pos, batch), 2, 7)
    edges = int(d.last_num_pairs.item()) if torch.is_tensor(d.last_num_pairs) else d.last_num_pairs
    sink(dict(point="et_water_box", config=label, strategy=strategy, atoms=n, edges=edges,
              workload="ET 128 ch, 8 layers, cutoff 5, energy + forces, eager", **stats(us)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--atoms", type=int, default=50001)
    ap.add_argument("--builds", default="abc", help="which of the builds (a), (b), (c) to time")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl_tric_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def sink(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    n = a.atoms
    L, rect, tric = boxes(n)
    if "a" in a.builds:
        build_point("a: cell, rectangular", "cell", rect, n, dev, sink)
    if "b" in a.builds:
        build_point("b: cell, triclinic", "cell", tric, n, dev, sink)
    if "c" in a.builds:
        build_point("c: shared, triclinic", "shared", tric, n, dev, sink, repeats=7, warmup=2)
    if not a.skip_model:
        model_point("rectangular, cell", "cell", rect, n, dev, sink)
        model_point("triclinic, cell", "cell", tric, n, dev, sink)
        model_point("triclinic, shared", "shared", tric, n, dev, sink)


if __name__ == "__main__":
    main()
