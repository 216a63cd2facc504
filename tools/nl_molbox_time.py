"""Times the per-molecule-box neighbour build against the single-box build on the same batch
(csrc/neighbors.hip: k_pairs<.., MOLBOX> reads each destination's box from a device array; the single-box
instantiation takes the one host box as a kernel argument).

Protocol: bench.py's 32-molecule QM9-like batch (qm9_like(32, 1), float32), cutoff 5, one 20 A cube per molecule
-- as a (3, 3) host box and as a (32, 3, 3) device stack of the same cube, so both builds produce the same list
(checked bit for bit before timing).  Every build through kernels.neighbor_pairs_raw (symmetric list with self
pairs, CSR rows and transpose map, padded to 32 pairs per atom, the model's capacity); WARMUP untimed calls of
each form, then REPEATS rounds that alternate the two forms, each call between two HIP events recorded on the
launching stream; reported as median (min-max) in microseconds.  The timed region includes the host side of
neighbor_pairs_raw (output allocations, and the float64 device copy the per-molecule form passes on).

usage (GPU box, repo root):  python tools/nl_molbox_time.py [--strategy brute] [--out FILE]
Prints one JSON object per form and appends it to --out (default profiles/nl_molbox_time.jsonl)."""
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

WARMUP, REPEATS = 20, 200
CUTOFF, SIDE, MOLECULES = 5.0, 20.0, 32


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
            "repeats": len(us)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--strategy", default="brute", choices=["brute", "shared"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl_molbox_time.jsonl"))
    a = ap.parse_args()
    from torchmdnet import kernels
    dev = torch.device("cuda", 0)
    z, pos, batch = bench.qm9_like(MOLECULES, 1)
    pos, batch = pos.float().to(dev), batch.to(dev)
    n = pos.shape[0]
    cap = 32 * n
    one = torch.eye(3, dtype=torch.float32) * SIDE
    stack = (torch.eye(3, dtype=torch.float64, device=dev) * SIDE).expand(MOLECULES, 3, 3).contiguous()

    def build(box):
        return kernels.neighbor_pairs_raw(a.strategy, pos, batch, box, True, 0.0, CUTOFF, cap, True, True,
                                          pad_output=True, want_csr=True)

    forms = {"single box (3, 3), host": lambda: build(one),
             "per-molecule boxes (32, 3, 3), device": lambda: build(stack)}
    ref, got = build(one), build(stack)
    pairs = int(ref[3].item())
    assert pairs <= cap, (pairs, cap)
    assert all(torch.equal(x, y) for x, y in zip(ref, got)), "the two forms built different lists"
    for fn in forms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, fn in forms.items():
            us[k].append(timed(fn))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for k in forms:
        rec = dict(point="build", form=k, strategy=a.strategy, atoms=n, molecules=MOLECULES, cutoff=CUTOFF,
                   box_side=SIDE, pairs=pairs, dtype="float32", **stats(us[k]))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
