"""Times what a periodic pair prior adds to an evaluation of a large periodic system: TensorNet + ZBL, energy +
forces, on the 50,001-atom water box of tests/test_gpu_tn_large.py (bench.tn_water_box_model: TensorNet-rMD17
architecture, cutoff 4.5, cell list, dynamic shapes), eager.

Three configurations of the same weights and positions, one JSON line each:

  1  ZBL(periodic=False)                            the prior ignores the box (what the package did before)
  2  ZBL(periodic=True)                             default strategy: brute, which build_graph moves to shared here
  3  ZBL(periodic=True, neighbor_strategy="cell")   the prior's list on the cell list

ZBL: cutoff 3.0, max_num_neighbors 48 (water density gives about 11 per atom), positions in Angstrom, energies in eV.
Protocol: the three models are built first; WARMUP untimed evaluations of each, then REPEATS rounds that go through
the three configurations in turn, so that clock and thermal drift falls on all of them alike; each evaluation
between two HIP events on the launching stream with a device synchronise at the end (the host side of the eager call
is inside the timed region); median (min-max) in milliseconds.  Line 1 also records the prior's pair count without
images, lines 2 and 3 the one with them (they must agree).

usage (GPU box, repo root):
  python tools/prior_box_time.py [--atoms 50001] [--repeats 20] [--out FILE]
Prints one JSON object per configuration and writes the three of them to --out (default
profiles/prior_box_time.jsonl), replacing what the file held: one run, three lines.  No number here is a threshold."""
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
ZBL_CUTOFF = 3.0
CONFIGS = (("non-periodic", dict(periodic=False)),
           ("periodic, default strategy", dict(periodic=True)),
           ("periodic, cell", dict(periodic=True, neighbor_strategy="cell")))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def setup(prior_args, n, dev):
    from torchmdnet.priors import ZBL
    model, z, pos, batch, L = bench.tn_water_box_model(n, False, 0, dev)
    prior = ZBL(ZBL_CUTOFF, 48, atomic_number=list(range(100)), distance_scale=1e-10, energy_scale=1.602176634e-19,
                **prior_args).to(dev)
    model.prior_model = torch.nn.ModuleList([prior])
    run = lambda: model(z, pos.clone(), batch)  # noqa: E731  (the distance module's own box reaches the prior)
    return run, prior, L


def record(name, prior, L, ms, n):
    return dict(point="tn_zbl_water_box", config=name, atoms=n, box_length=round(L, 3), zbl_cutoff=ZBL_CUTOFF,
                zbl_pairs=int(prior.last_num_pairs), dtype="float32",
                workload="TensorNet-rMD17 (128 ch, 2 layers, cutoff 4.5, cell list) + ZBL, energy + forces, eager",
                median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                repeats=len(ms), warmup=WARMUP, order="the configurations alternate within every round")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--atoms", type=int, default=50001)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_box_time.jsonl"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats: at least 20 timed evaluations")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    forms = [(name,) + setup(prior_args, a.atoms, dev) for name, prior_args in CONFIGS]
    for _, run, _, _ in forms:
        for _ in range(WARMUP):
            y, f = run()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(f).all())
    ms = {name: [] for name, _, _, _ in forms}
    for _ in range(a.repeats):
        for name, run, _, _ in forms:
            ms[name].append(timed(run))
    recs = [record(name, prior, L, ms[name], a.atoms) for name, _, prior, L in forms]
    with open(a.out, "w") as f:
        for rec in recs:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    assert recs[1]["zbl_pairs"] == recs[2]["zbl_pairs"] >= recs[0]["zbl_pairs"], "the periodic lists disagree"


if __name__ == "__main__":
    main()
