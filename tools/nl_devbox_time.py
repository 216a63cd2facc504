"""Times the cell-list build whose box lives on the device (csrc/neighbors.hip: k_cell_geom and the DEVGEOM forms of
k_cell_assign / k_cell_pairs; tmdnet_nl_build with the cell strategy and use_periodic == 2) against the host-box
cell build and against the shared build with a device box -- what a captured run with a changing cell had to
take before -- and the captured ET evaluation with ``box=`` on the cell list against the shared strategy.

Protocol: float32, N atoms (default 50,001) at water density 0.1003 / A^3, cutoff 5, in a cubic box and in a box
of the t31 shape of tests/neighbor_cases_tric.py ((31, 0, 0), (7, 23, 0), (-5, 6, 17.5)) scaled to the same
volume.  Every build through kernels.neighbor_pairs_raw (symmetric list with self pairs, CSR rows and transpose
map, padded); the device-box build's workspace is sized as GraphedEnergyForces sizes it, for the box scaled by
1.25.  The device-box list is checked bit for bit against the host-box list before timing.  WARMUP untimed calls
of each form, then REPEATS rounds that alternate the forms, each call between two HIP events on the launching
stream; median (min-max) in microseconds.  The timed region includes the host side of neighbor_pairs_raw.

  host:    cell, (3, 3) host box
  device:  cell, (1, 3, 3) device box, cell_bound = 1.25 box
  shared:  shared, (1, 3, 3) device box

Allowance of the device form over the host form (--parent: the jsonl this tool wrote at the parent commit, whose
host figure is the yardstick; without it, this run's own host figure): the two things it adds --
  * one single-workgroup launch: --launch-floor-us, the ``stream_launch`` figure of tools/launch_floor.hip from
    the same session;
  * the cstart fill over the capacity instead of the grid: hipMemsetAsync of the two sizes timed here (64
    back-to-back calls between two events), their difference, not below zero.
The record says whether the device median is within yardstick + allowance.

ET (unless --skip-model): 128 channels, 8 layers, cutoff 5, max_num_neighbors 128; GraphedEnergyForces(model, z,
pos, batch, box=box) with strategy "cell" and with "shared"; after construction (warm-up + capture), replays
alternating between the box and the box and positions scaled by 1.01, each replay between two events.

usage (GPU box, repo root):
  python tools/nl_devbox_time.py [--atoms 50001] [--launch-floor-us X] [--parent FILE] [--skip-model] [--out FILE]
Where the device-box cell build does not exist (the parent commit) its points are recorded as unsupported.
Prints one JSON object per point and appends it to --out (default profiles/nl_devbox_time.jsonl)."""
import argparse
import ctypes
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
MARGIN = 1.25
T31 = ((31.0, 0.0, 0.0), (7.0, 23.0, 0.0), (-5.0, 6.0, 17.5))


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


def boxes(n):
    vol = n / DENSITY
    cubic = torch.eye(3, dtype=torch.float64) * vol ** (1.0 / 3.0)
    t31 = torch.tensor(T31, dtype=torch.float64)
    t31 = t31 * (vol / float(torch.linalg.det(t31))) ** (1.0 / 3.0)
    return {"cubic": cubic, "t31": t31}


def positions(n, box, seed, dev):
    g = torch.Generator().manual_seed(seed)
    frac = torch.rand(n, 3, generator=g, dtype=torch.float64)
    return (frac @ box).float().to(dev)


def grid_cells(box):
    """Cells of the host rule (cell_dims) for ``box``: tests/neighbor_cases_tric.py ``grid``."""
    (a0, _, _), (b0, b1, _), (c0, c1, c2) = box.tolist()
    if b0 == 0 and c0 == 0 and c1 == 0:
        w = (a0, b1, c2)
    else:
        bc = (b1 * c2, -b0 * c2, b0 * c1 - b1 * c0)
        w = (abs(a0 * b1 * c2) / (bc[0] ** 2 + bc[1] ** 2 + bc[2] ** 2) ** 0.5,
             abs(b1 * c2) / (c1 * c1 + c2 * c2) ** 0.5, abs(c2))
    n = [max(3, int(v / CUTOFF)) for v in w]
    return n[0] * n[1] * n[2]


def memset_us(nbytes, dev):
    """One hipMemsetAsync of ``nbytes`` on the current stream (the cstart fill's call), from 64 back to back."""
    hip = ctypes.CDLL("libamdhip64.so")
    buf = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda: hip.hipMemsetAsync(ctypes.c_void_p(buf.data_ptr()), 0xFF, ctypes.c_size_t(nbytes), stream)  # noqa: E731

    def burst():
        for _ in range(64):
            call()
    for _ in range(3):
        burst()
    torch.cuda.synchronize()
    return statistics.median(timed(burst) for _ in range(15)) / 64


def build_points(name, box, n, dev, sink, floor_us, parent):
    from torchmdnet import kernels
    pos = positions(n, box, 7, dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    cap = n * 96
    b32 = box.float()
    dbox = b32.double().reshape(1, 3, 3).to(dev)  # the float32 box's values as the nine doubles the build reads
    bound = b32.double() * MARGIN

    def build(strategy, bx, **kw):
        return kernels.neighbor_pairs_raw(strategy, pos, batch, bx, True, 0.0, CUTOFF, cap, True, True,
                                          pad_output=True, want_csr=True, **kw)

    forms = {"host": lambda: build("cell", b32), "device": lambda: build("cell", dbox, cell_bound=bound),
             "shared": lambda: build("shared", dbox)}
    ref = forms["host"]()
    pairs = int(ref[3].item())
    assert pairs <= cap, (pairs, cap)
    try:
        got = forms["device"]()
        assert all(torch.equal(x, y) for x, y in zip(ref, got)), "the device-box build differs from the host-box build"
    except (RuntimeError, TypeError) as e:  # the parent commit: no device-box cell build
        sink(dict(point="build", box=name, form="device", unsupported=str(e)[:80]))
        del forms["device"]
    for fn in forms.values():
        for _ in range(WARMUP if fn is not forms["shared"] else 2):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for r in range(REPEATS):
        for k, fn in forms.items():
            if k != "shared" or r < 7:  # the all-pairs build takes milliseconds
                us[k].append(timed(fn))
    med = {}
    for k in forms:
        rec = dict(point="build", box=name, form=k, atoms=n, cutoff=CUTOFF, pairs=pairs, dtype="float32",
                   box_rows=[[round(v, 3) for v in row] for row in box.tolist()], **stats(us[k]))
        med[k] = rec["median_us"]
        sink(rec)
    if "device" in med:
        cells, room = grid_cells(b32.double()), grid_cells(bound)
        fill = max(0.0, memset_us(4 * room, dev) - memset_us(4 * cells, dev))
        yard = parent.get(name, med["host"])
        rec = dict(point="allowance", box=name, host_us=med["host"], device_us=med["device"], shared_us=med["shared"],
                   yardstick_host_us=yard, yardstick="parent commit" if name in parent else "this run",
                   launch_floor_us=floor_us, grid_cells=cells, capacity_cells=room, fill_extra_us=round(fill, 2))
        if floor_us is not None:
            rec["allowed_us"] = round(yard + floor_us + fill, 1)
            rec["within"] = bool(med["device"] <= rec["allowed_us"])
        sink(rec)


def model_point(name, strategy, box, n, dev, sink):
    from torchmdnet.graphs import GraphedEnergyForces
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
    dbox = box.to(dev)
    try:
        gm = GraphedEnergyForces(model, z, pos, batch, box=dbox)
    except RuntimeError as e:
        sink(dict(point="et_captured_box", box=name, strategy=strategy, unsupported=str(e)[:80]))
        return
    try:
        cells = [(pos, dbox), (pos * 1.01, dbox * 1.01)]
        for p, b in cells:  # both cells once, untimed
            gm(p, box=b)
        torch.cuda.synchronize()
        us = [timed(lambda: gm(cells[r % 2][0], box=cells[r % 2][1])) for r in range(8)]
        gm.check_capacity()
        sink(dict(point="et_captured_box", box=name, strategy=strategy, atoms=n, edge_capacity=gm.edge_capacity,
                  workload="ET 128 ch, 8 layers, cutoff 5, energy + forces, HIP-graph replay with box=",
                  **stats(us)))
    finally:
        gm.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--atoms", type=int, default=50001)
    ap.add_argument("--launch-floor-us", type=float, default=None)
    ap.add_argument("--parent", default=None, help="jsonl of this tool at the parent commit")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nl_devbox_time.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    parent = {}
    if a.parent:
        with open(a.parent) as f:
            for line in f:
                r = json.loads(line)
                if r.get("point") == "build" and r.get("form") == "host":
                    parent[r["box"]] = r["median_us"]

    def sink(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for name, box in boxes(a.atoms).items():
        build_points(name, box, a.atoms, dev, sink, a.launch_floor_us, parent)
    if not a.skip_model:
        for name, box in boxes(a.atoms).items():
            for strategy in ("cell", "shared"):
                model_point(name, strategy, box, a.atoms, dev, sink)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
