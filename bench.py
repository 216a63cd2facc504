#!/usr/bin/env python
"""Benchmark: ET-QM9 (128 channels, 8 layers, 64 RBF, cutoff 5) energy + forces, molecules/s.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--mode infer|train] [--dump-outputs DIR] [--full]
  (N > 1 without a launcher: bench.py starts N rank processes itself through torch.distributed.run
   before anything touches a GPU; under torchrun, WORLD_SIZE must equal N)

A plain run sets up, warms up, times the K steps and prints one JSON line (metric, value, unit,
ms_per_step, ...).  --dump-outputs DIR also writes what the last timed step returned (infer: y.npy and
neg_dy.npy, train: loss.npy; float32) into DIR; the inputs and weights are seeded, so two builds run
with the same arguments can be compared output for output.  Everything else below runs only with --full.

One step = TorchMD_Net.forward with derivative=True (y and -dy/dpos, create_graph=True exactly as
reference models/model.py:286-298) on a batch of 32 synthetic QM9-like molecules resident in HBM
(SURVEY.md §8(d) generator; weights random-init with the reference architecture).  --mode train
adds the force-matching loss, double backward, the fused RCCL gradient all-reduce and AdamW.
Weak scaling: every rank processes its own batch; value = molecules of all ranks / max-rank time.

With --full, also reported (rank 0; each leg has its own --no-... switch):
  secondary    -- the other configurations (TensorNet C3, the training steps, fit() on the data path,
                  ET-SPICE C4, TorchScript, the C5 water boxes).
  ddp_train    -- the data-parallel TRAINING step at this N: ET-SPICE C4, 16 x 40
                  atoms per GPU, E+F loss, forces with create_graph, double backward, ONE fused RCCL
                  all-reduce of the gradients, fused AdamW; HIP-graph replay of fwd + double backward on
                  every rank; molecules/s of all ranks / max-rank time (weak scaling).
  roofline     -- the ET edge-aggregation kernel (tmdnet_et_message_fwd) on a C5-scale periodic
                  water box (50,001 atoms, ~2.7 M edges), HIP events on the launching stream;
                  algorithmic bytes per launch = E*(20 + 16H) + N*(48H + 4)  (SURVEY.md §8(d)).
  roofline_c2  -- the same kernel live in the metric workload (eager / train mode: inside the timed
                  region, also without --full; hip-graph mode: a short eager pass after it).
  cpu_baseline -- oracle/model_oracle.py (plain PyTorch-CPU restatement of the reference) on the
                  same 32 molecules and weights, host cores of this box, bounded sample (N=1 only).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "torchmd-net_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_F32_PEAK_TFS = 157.3  # MI355X dense fp32 MFMA (v_mfma_f32_16x16x4_f32) spec, MI355X_MICROARCH.md
MFMA_BF16_PEAK_TFS = 2500.0  # MI355X dense bf16 MFMA, MI355X_MICROARCH.md (no sparsity)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", choices=["infer", "train"], default="infer")
    ap.add_argument("--batch", type=int, default=32, help="molecules per GPU")
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--roofline-atoms", type=int, default=50001)
    ap.add_argument("--roofline-reps", type=int, default=50)
    ap.add_argument("--eager", action="store_true", help="no HIP-graph capture (infer mode)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc traffic passes")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary lines (TensorNet C3 graph replay, ET training step)")
    ap.add_argument("--no-graphed-train", dest="graphed_train", action="store_false",
                    help="skip the HIP-graph-captured ET-QM9 training step (training.GraphedTrainStep)")
    ap.add_argument("--no-ddp-train", dest="ddp_train", action="store_false",
                    help="skip the ddp_train line (ET-SPICE graphed training step + all-reduce)")
    ap.add_argument("--cpu-extra-seconds", type=float, default=6.0,
                    help="CPU sample per extra baseline config (C2 training, C3, C4, C5 1500-atom box)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the secondary lines, ddp_train, the roofline / MFMA probes "
                         "and the CPU baseline (each still subject to its --no-... switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


def qm9_like(n_mol, gen_seed):
    """n = randint(9, 30) atoms, floor(n/2) heavy atoms in {C,N,O,F}, rest H,
    pos = randn * 1.6 A; molecules concatenated, batch = molecule id."""
    g = torch.Generator().manual_seed(gen_seed)
    zs, ps, bs = [], [], []
    for m in range(n_mol):
        n = int(torch.randint(9, 30, (1,), generator=g))
        heavy = n // 2
        z = torch.ones(n, dtype=torch.long)
        z[:heavy] = torch.tensor([6, 7, 8, 9])[torch.randint(0, 4, (heavy,), generator=g)]
        zs.append(z)
        ps.append(torch.randn(n, 3, generator=g, dtype=torch.float64) * 1.6)
        bs.append(torch.full((n,), m, dtype=torch.long))
    return torch.cat(zs), torch.cat(ps), torch.cat(bs)


def et_args(channels):
    import yaml
    with open(os.path.join(ROOT, "tests", "golden", "configs", "et_qm9.yaml")) as f:
        args = yaml.safe_load(f)
    args.update(prior_model=None, embedding_dimension=channels, derivative=True, output_model="Scalar",
                precision=32)
    return args


def maybe_spawn(a):
    """--gpus N > 1 without a launcher: start N ranks (one process per GPU) through
    torch.distributed.run as a CHILD and exit with its code.  Runs before any GPU call (this parent
    never initialises HIP).  Under a launcher, WORLD_SIZE must equal N."""
    ws_env = os.environ.get("WORLD_SIZE")
    if ws_env is not None:
        if int(ws_env) != a.gpus:
            print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={ws_env}", file=sys.stderr)
            sys.exit(2)
        return
    if a.gpus <= 1:
        return
    import socket
    import subprocess
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    phase(f"spawning {a.gpus} ranks: {' '.join(cmd[1:6])} ...")
    sys.exit(subprocess.call(cmd))


def host_cpu_info():
    """CPU model, physical cores of the machine, and the threads this process may use."""
    model, phys = None, set()
    try:
        cur = {}
        for line in open("/proc/cpuinfo"):
            if ":" not in line:
                if "core id" in cur:
                    phys.add((cur.get("physical id"), cur["core id"]))
                cur = {}
                continue
            k, v = (x.strip() for x in line.split(":", 1))
            cur[k] = v
            if k == "model name" and model is None:
                model = v
        if "core id" in cur:
            phys.add((cur.get("physical id"), cur["core id"]))
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS")
    threads = min(aff, int(omp)) if omp and omp.isdigit() and int(omp) > 0 else aff
    quota = None  # the container's CPU bandwidth limit (cgroup v2 cpu.max "quota period"), in CPUs
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    return {"cpu_model": model, "physical_cores_machine": len(phys) or None, "logical_cpus": os.cpu_count(),
            "affinity_cpus": aff, "cgroup_cpu_quota": quota, "omp_num_threads_env": omp, "threads_used": threads}


def setup_dist():
    """One process per GPU (torchrun), RCCL.  TMDNET_BENCH_REHEARSAL=1 (testing only) runs every
    rank on cuda:0 over gloo, to rehearse the multi-rank code path on a one-GPU machine."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if ws > 1 and os.environ.get("TMDNET_BENCH_REHEARSAL") == "1":
        torch.cuda.set_device(0)
        dist.init_process_group("gloo")
        return ws, rank, torch.device("cuda", 0)
    if ws > 1:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
    return ws, rank, torch.device("cuda", local if ws > 1 else 0)


def dist_info(ws, rank, dev):
    """What the process group actually is: backend, world size, and per rank its
    device index, PCI location and host -- so a multi-GPU record shows N ranks on N distinct devices."""
    props = torch.cuda.get_device_properties(dev)
    mine = [rank, dev.index if dev.index is not None else 0, int(getattr(props, "pci_domain_id", -1)),
            int(getattr(props, "pci_bus_id", -1)), int(getattr(props, "pci_device_id", -1)),
            int(os.environ.get("LOCAL_RANK", "0"))]
    rows = [mine]
    if ws > 1:
        t = torch.tensor(mine, dtype=torch.int64, device=dev)
        out = [torch.empty_like(t) for _ in range(ws)]
        dist.all_gather(out, t)
        rows = [[int(v) for v in x.cpu()] for x in out]
    info = {"world_size": ws, "backend": dist.get_backend() if ws > 1 else None,
            "device_name": props.name, "gcn_arch": getattr(props, "gcnArchName", None),
            "ranks": [{"rank": r[0], "local_rank": r[5], "device": r[1], "pci": f"{r[2]:04x}:{r[3]:02x}:{r[4]:02x}"}
                      for r in rows]}
    if ws > 1:
        info["distinct_devices"] = len({x["pci"] for x in info["ranks"]})
        try:
            v = torch.cuda.nccl.version()
            info["rccl_version"] = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
        except Exception:  # noqa: BLE001 -- informational only
            pass
    return info


def barrier(ws):
    if ws > 1:
        dist.barrier()


def max_over_ranks(x, ws, dev):
    if ws == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def et_algorithmic_bytes(E, N, H, s=4):
    return E * (4 + 4 + 12 + 4 * H * s) + N * (12 * H * s + 4)


def probe_workload(n_atoms, H, dev):
    """ET edge-aggregation forward on a C5-scale water box: returns a launcher of
    ONE tmdnet_et_message_fwd call plus (E, L)."""
    from torchmdnet import kernels
    g = torch.Generator().manual_seed(7)
    L = (n_atoms / 0.1003) ** (1.0 / 3.0)
    pos = (torch.rand(n_atoms, 3, generator=g, dtype=torch.float64) * L).float().to(dev)
    batch = torch.zeros(n_atoms, dtype=torch.long, device=dev)
    box = torch.eye(3, dtype=torch.float32) * L
    # the model renumbers large systems spatially (Morton order of cutoff cells) before its edge
    # kernels run (kernels.spatial_permutation); the probe measures the kernel in that numbering
    perm = kernels.spatial_permutation(pos, batch, 5.0, box)
    pos = pos[perm].contiguous()
    graph = kernels.build_graph(pos, batch, 0.0, 5.0, 128 * n_atoms, loop=True, strategy="cell", box=box)
    E = graph.n_edges
    dl, r = graph.deltas.detach(), graph.distances.detach()
    C = 0.5 * (torch.cos(r * math.pi / 5.0) + 1.0)
    u = dl / torch.where(r > 0, r, torch.ones_like(r)).unsqueeze(1)
    gen = torch.Generator(device=dev).manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen, dtype=torch.float32)
    q, k, v, vec = rn(n_atoms, H), rn(n_atoms, H), rn(n_atoms, 3 * H), rn(n_atoms, 3, H)
    pk, pv = rn(E, H), rn(E, 3 * H)
    lib = kernels.nat.load()
    xo = torch.empty(n_atoms, H, device=dev)
    vo = torch.empty(n_atoms, 3, H, device=dev)
    st = kernels.nat.stream(dev)
    ptr = kernels.nat.ptr

    def launch():
        rc = lib.tmdnet_et_message_fwd(0, n_atoms, H, 8, ptr(graph.row_ptr), ptr(graph.src), E, ptr(q), H,
                                       ptr(k), H, ptr(v), 3 * H, ptr(vec), ptr(pk), H, ptr(pv), 3 * H, ptr(C),
                                       ptr(u), ptr(xo), ptr(vo), PROBE_FLAGS, None, None, st)
        kernels.nat.check(rc, "tmdnet_et_message_fwd")

    # the model's layout: one dk/dv row per edge pair, read by both directions (et_stack.PAIR_ROWS)
    pair_row, pair_edge = kernels.pair_index(graph)
    P = pair_edge.shape[0]
    pk2, pv2 = pk[:P].contiguous(), pv[:P].contiguous()

    def launch_pairs():
        rc = lib.tmdnet_et_message_fwd(0, n_atoms, H, 8, ptr(graph.row_ptr), ptr(graph.src), E, ptr(q), H,
                                       ptr(k), H, ptr(v), 3 * H, ptr(vec), ptr(pk2), H, ptr(pv2), 3 * H,
                                       ptr(C), ptr(u), ptr(xo), ptr(vo), PROBE_FLAGS, ptr(pair_row), None, st)
        kernels.nat.check(rc, "tmdnet_et_message_fwd")

    # the backward in the model's layout (destination + source CSR passes, one C-ABI call): the
    # training form (per-edge projection gradient written) and the force-pass "dr" form (contracted
    # with d(dk,dv)/dr of the pair rows in-kernel, g_r accumulated)
    # (allocated on the first backward launch: the forward probes run with only their own inputs
    # resident, as in the model's forward)
    bw = {}

    def launch_bwd(dr=False):
        if not bw:
            bw["gx"], bw["gvec"] = rn(n_atoms, H), rn(n_atoms, 3, H)
            bw["gq"], bw["gk"] = torch.empty(n_atoms, H, device=dev), torch.empty(n_atoms, H, device=dev)
            bw["gv"], bw["gw"] = torch.empty(n_atoms, 3 * H, device=dev), torch.empty(n_atoms, 3, H, device=dev)
            bw["gpk"], bw["gpv"] = torch.empty(E, H, device=dev), torch.empty(E, 3 * H, device=dev)
            bw["gC"], bw["gu"], bw["gr"] = (torch.zeros(E, device=dev), torch.zeros(E, 3, device=dev),
                                            torch.zeros(E, device=dev))
            bw["dpk"], bw["dpv"] = rn(P, H), rn(P, 3 * H)
        gx, gvec, gq, gk, gv, gw = bw["gx"], bw["gvec"], bw["gq"], bw["gk"], bw["gv"], bw["gw"]
        gpk, gpv, gC, gu, gr, dpk, dpv = bw["gpk"], bw["gpv"], bw["gC"], bw["gu"], bw["gr"], bw["dpk"], bw["dpv"]
        acc = 1 | 2 | PROBE_FLAGS  # TMDNET_ACC_VEC_RESIDUAL | TMDNET_ACC_EDGE | planar rows
        rc = lib.tmdnet_et_message_bwd(
            0, n_atoms, H, 8, ptr(graph.row_ptr), ptr(graph.src), E, ptr(q), H, ptr(k), H, ptr(v), 3 * H,
            ptr(vec), ptr(pk2), H, ptr(pv2), 3 * H, ptr(C), ptr(u), ptr(gx), ptr(gvec), ptr(gq), ptr(gk), ptr(gv),
            ptr(gw), None if dr else ptr(gpk), None if dr else ptr(gpv), ptr(gC), ptr(gu),
            ptr(dpk) if dr else None, ptr(dpv) if dr else None, ptr(gr) if dr else None, acc, ptr(pair_row), None,
            st)
        kernels.nat.check(rc, "tmdnet_et_message_bwd")

    launch.pairs = launch_pairs
    launch.bwd = launch_bwd
    launch.n_pairs = P
    launch.graph, launch.inputs = graph, (q, k, v, vec, C, u)
    launch.pair_row, launch.pair_edge = pair_row, pair_edge
    return launch, E, L


def tn_message_probe_setup(n_atoms, H, dev, static=False):
    """The TensorNet message (tmdnet_tn_message_fwd_pairs / _bwd_pairs, csrc/tn_message.hip) on the C5 TensorNet
    graph: a periodic n-atom water box, cutoff 4.5, cell list, Morton-renumbered as the model does, the edge
    factors as the model's pair rows (one [3H] row per edge pair, kernels.pair_index).  Returns launchers of one
    forward and one backward (pair destination pass + source pass) plus (E, N, P)."""
    from torchmdnet import kernels
    g = torch.Generator().manual_seed(7)
    L = (n_atoms / 0.1003) ** (1.0 / 3.0)
    pos = (torch.rand(n_atoms, 3, generator=g, dtype=torch.float64) * L).float().to(dev)
    batch = torch.zeros(n_atoms, dtype=torch.long, device=dev)
    box = torch.eye(3, dtype=torch.float32) * L
    perm = kernels.spatial_permutation(pos, batch, 4.5, box)
    pos = pos[perm].contiguous()
    graph = kernels.build_graph(pos, batch, 0.0, 4.5, 64 * n_atoms, loop=True, strategy="cell", box=box)
    pairs = kernels.pair_index(graph)
    P = pairs[1].shape[0]
    gen = torch.Generator(device=dev).manual_seed(3)
    ea = torch.randn(P, 3 * H, device=dev, generator=gen)
    Tc = torch.randn(9, n_atoms, H, device=dev, generator=gen)
    msg = torch.empty_like(Tc)
    bw = {}

    def fwd():
        kernels.tn_message_fwd_launch(ea, Tc, graph, msg, pairs)

    def bwd():
        if not bw:
            bw["g"] = torch.randn(9, n_atoms, H, device=dev, generator=gen)
            bw["gea"], bw["gT"] = torch.empty_like(ea), torch.empty_like(Tc)
        kernels.tn_message_bwd_launch(ea, Tc, graph, bw["g"], bw["gea"], bw["gT"], pairs=pairs)

    return fwd, bwd, graph.n_edges, n_atoms, P, L


def tn_message_bytes(E, N, H, s=4):
    """SURVEY.md 8(d) TensorNet message, per layer: E*(4 + 3H*s) + N*(9H*s + 9H*s + 4) -- src index and the
    edge factor row per edge, the compact I/A/S tensor (9 per channel) read and the message written per node."""
    return E * (4 + 3 * H * s) + N * (18 * H * s + 4)


def tn_message_probe(a, dev):
    H = a.channels
    fwd, bwd, E, N, P, L = tn_message_probe_setup(a.roofline_atoms, H, dev)
    ms = _event_ms(fwd, a.roofline_reps)
    ms_b = _event_ms(bwd, max(4, a.roofline_reps // 2))
    nb = tn_message_bytes(E, N, H)
    pb = E * (4 + 4) + P * 3 * H * 4 + N * (18 * H * 4 + 4)  # distinct bytes in the pair layout
    # backward: gmsg + Tc read per node, both endpoints' rows per pair, the pair gradient rows written; the
    # source pass: factor rows per edge, gmsg rows, gT written
    bb = E * 4 + N * (18 * H * 4) + P * 3 * H * 4 + (E * (4 + 3 * H * 4) + N * (18 * H * 4 + 4))
    gbs = nb / (ms * 1e-3) / 1e9
    return {"kernel": "tmdnet_tn_message_fwd_pairs (tn::k_msg_fwd<float,4>): TensorNet message passing, pair-row edge "
                      "factors (the C5 TensorNet path, models/tensornet.py PAIR_MIN_EDGES)",
            "workload": f"periodic water box, {N} atoms (Morton-renumbered), L={L:.1f} A, cutoff 4.5, E={E}, P={P} pair "
                        f"rows, H={H}, fp32",
            "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": None, "bytes_per_launch": nb,
            "bytes_formula": "SURVEY.md 8(d): E*(4 + 3H*4) + N*(18H*4 + 4)",
            "pair_layout_distinct_bytes": pb, "ms_per_launch": round(ms, 4), "launches": a.roofline_reps,
            "backward": {"kernels": "k_msg_bwd_pair (pair-owner destination pass) + k_msg_bwd_src",
                         "ms_per_call": round(ms_b, 4), "bytes_per_call": bb,
                         "achieved": round(bb / (ms_b * 1e-3) / 1e9, 1),
                         "frac": round(bb / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}


def et_pair_bytes(E, N, P, H, s=4):
    """Algorithmic bytes of one forward edge-kernel launch in the model's layout (pair-shared dk/dv
    rows, et_stack.PAIR_ROWS): per edge its source index, pair-row index, cutoff and unit vector; the
    P distinct projection rows (4H); per node q, k, v, vec read and x, vec written (12H), row_ptr."""
    return E * (4 + 4 + 4 + 12) + P * 4 * H * s + N * (12 * H * s + 4)


def et_bwd_bytes(E, N, P, H, dr, s=4):
    """Algorithmic bytes of one tmdnet_et_message_bwd call (destination + source pass) in the model's
    pair-row layout, every tensor touched once: edge scalars (src, pair row, cutoff, unit vector) and
    the P projection rows read; node features q, k, v, vec and the incoming gx, gvec read; gq, gk, gv,
    gvec_in written; per edge g_cut, g_unit accumulated (read + write); training form: the per-edge
    projection gradient written (E x 4H), dr form: d(dk,dv)/dr rows read (P x 4H) and g_r accumulated."""
    b = E * (4 + 4 + 4 + 12) + N * 4 + P * 4 * H * s              # CSR / edge scalars, projection rows
    b += N * (H + H + 3 * H + 3 * H + H + 3 * H) * s              # q, k, v, vec, gx, gvec
    b += N * (H + H + 3 * H + 3 * H) * s                          # gq, gk, gv, gvec_in
    b += 2 * E * (4 + 12)                                         # g_cut, g_unit (accumulated)
    b += (P * 4 * H * s + 2 * E * 4) if dr else E * 4 * H * s     # dr: dpkv rows + g_r; else gpkv
    return b


PROBE_KERNEL = "k_fwd<float, 4, 4, 1, false, false>"  # (4 waves per node at every size since r04)
# the model runs large graphs with planar v / dv rows (et_stack.PLANAR_MIN_EDGES): probe that layout
PROBE_FLAGS = 4  # TMDNET_ET_V_PLANAR


PMC_PASSES = ("FETCH_SIZE", "WRITE_SIZE", "TCC_HIT_sum TCC_MISS_sum")
# the child's dispatch sequence (main(), --pmc-child): probe kernel name -> [(tag, count), ...] in order
PMC_CHILD = {"et::k_fwd<float, 4, 4, 1, false, false>": [("per_edge", 8), ("pairs", 8)],
             "et::k_bwd_dst<": [("bwd_dst", 4)], "et::k_bwd_src<": [("bwd_src", 4)], "et::k_bwd_merged<": [("bwd_dr", 4)],
             "fep::k_fwd<": [("fused_fwd", 8)], "fep::k_bwd_dst<": [("fused_bwd_dst", 4)],
             "fep::k_bwd_src<": [("fused_bwd_src", 4)], "fep::k_edge_combine": [("fused_edge_combine", 4)],
             "tn::k_msg_fwd<": [("tn_msg_fwd", 8)], "tn::k_msg_bwd_pair<": [("tn_msg_bwd_pair", 4)],
             "tn::k_msg_bwd_src<": [("tn_msg_bwd_src", 4)]}


def pmc_counters(a):
    """Per-launch counters of the C5 probe kernels from rocprofv3 (one pass per entry of PMC_PASSES,
    each in a child process running the probes in a fixed order): FETCH_SIZE / WRITE_SIZE in bytes
    (FETCH x2: gfx950 tallies 16-B/lane reads at half their bytes, MI355X_MICROARCH.md 'HBM';
    FETCH_SIZE counts Infinity-Cache hits too, so it is L2->fabric traffic, an upper bound on HBM
    bytes) and the L2 hit rate TCC_HIT / (TCC_HIT + TCC_MISS).  Returns ({tag: {...}}, None) or
    (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    res = {}
    for pas in PMC_PASSES:
        d = tempfile.mkdtemp(prefix="tmdnet_pmc_")
        cmd = [prof, "--pmc", *pas.split(), "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable,
               os.path.abspath(__file__), "--pmc-child", "--roofline-atoms", str(a.roofline_atoms),
               "--channels", str(a.channels)]
        try:
            subprocess.run(cmd, timeout=300, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           env=dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp")))
        except (subprocess.SubprocessError, OSError) as e:
            shutil.rmtree(d, ignore_errors=True)
            return None, f"rocprofv3 {pas} pass failed: {type(e).__name__}"
        recs = {}  # (kernel key, counter) -> [(dispatch id, value)]
        for f in glob.glob(os.path.join(d, "**", "*counter_collection*.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r.get("Kernel_Name", "")
                for key in PMC_CHILD:
                    if key in name:
                        did = int(r.get("Dispatch_Id", r.get("Correlation_Id", 0)) or 0)
                        recs.setdefault((key, r.get("Counter_Name")), []).append((did, float(r["Counter_Value"])))
        shutil.rmtree(d, ignore_errors=True)
        for (key, ctr), vals in recs.items():
            vals = [v for _, v in sorted(vals)]
            i = 0
            for tag, cnt in PMC_CHILD[key]:
                part = vals[i:i + cnt]
                i += cnt
                part = part[2:] or part  # drop warm-up dispatches
                if part:
                    res.setdefault(tag, {})[ctr] = sum(part) / len(part)
    if not res:
        return None, "no counter records for the probe kernels"
    out = {}
    for tag, c in res.items():
        e = {}
        if "FETCH_SIZE" in c:
            e["fetch_bytes"] = round(2.0 * c["FETCH_SIZE"] * 1024.0)
        if "WRITE_SIZE" in c:
            e["write_bytes"] = round(c["WRITE_SIZE"] * 1024.0)
        if "fetch_bytes" in e and "write_bytes" in e:
            e["traffic"] = e["fetch_bytes"] + e["write_bytes"]
        if c.get("TCC_HIT_sum") is not None and c.get("TCC_MISS_sum") is not None:
            tot = c["TCC_HIT_sum"] + c["TCC_MISS_sum"]
            e["l2_hit_rate"] = round(c["TCC_HIT_sum"] / tot, 4) if tot else None
        out[tag] = e
    return out, None


PMC_SOURCE = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / TCC_HIT_sum+TCC_MISS_sum (separate passes), FETCH x2 "
              "(gfx950 16-B/lane correction); includes Infinity-Cache hits")


def roofline_probe(a, dev):
    n_atoms, reps, H = a.roofline_atoms, a.roofline_reps, a.channels
    launch, E, L = probe_workload(n_atoms, H, dev)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    # back-to-back launches between one pair of HIP events recorded on the launch stream: the
    # average launch duration, comparable with rocprofv3's per-kernel average
    a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    for _ in range(reps):
        launch()
    b0.record()
    torch.cuda.synchronize()
    ms = a0.elapsed_time(b0) / reps
    nbytes = et_algorithmic_bytes(E, n_atoms, H)
    gbs = nbytes / (ms * 1e-3) / 1e9
    per_edge = {"kernel": "tmdnet_et_message_fwd (k_fwd<float,4,4,1,false,false>), one dk/dv row per edge",
                "bytes_per_launch": nbytes, "bytes_formula": "SURVEY.md 8(d): E*2068 + N*6148 (H=128)",
                "ms_per_launch": round(ms, 4), "achieved": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                "launches": reps}
    # the graded figure: the same kernel in the layout the model runs, the dk/dv stream over the
    # (E + N) / 2 pair-shared rows read through pk_rows
    for _ in range(5):
        launch.pairs()
    torch.cuda.synchronize()
    a0.record()
    for _ in range(reps):
        launch.pairs()
    b0.record()
    torch.cuda.synchronize()
    ms_p = a0.elapsed_time(b0) / reps
    pbytes = et_pair_bytes(E, n_atoms, launch.n_pairs, H)
    gbp = pbytes / (ms_p * 1e-3) / 1e9
    res = {"kernel": "tmdnet_et_message_fwd (k_fwd<float,4,4,1,false,false>) in the model's layout: pair-shared "
                     "dk/dv rows (et_stack.PAIR_ROWS, planar v rows)",
           "workload": f"periodic water box, {n_atoms} atoms (Morton-renumbered as the model does), "
                       f"L={L:.1f} A, cutoff 5, E={E}, P={launch.n_pairs} pair rows, H={H}, fp32",
           "bound": "hbm", "achieved": round(gbp, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(gbp / HBM_PEAK_GBS, 4), "traffic": None,
           "bytes_per_launch": pbytes,
           "bytes_formula": "E*(4+4+4+12) + P*4H*4 + N*(12H*4+4): edge scalars, distinct pair rows, node rows",
           "ms_per_launch": round(ms_p, 4), "launches": reps, "per_edge_layout": per_edge}
    # the backward (destination + source pass per call) in the model's layout, both forms
    bwd = {}
    for tag, dr in (("training_form", False), ("dr_force_form", True)):
        for _ in range(3):
            launch.bwd(dr)
        torch.cuda.synchronize()
        nrep = max(4, reps // 2)
        a0.record()
        for _ in range(nrep):
            launch.bwd(dr)
        b0.record()
        torch.cuda.synchronize()
        ms_b = a0.elapsed_time(b0) / nrep
        bb = et_bwd_bytes(E, n_atoms, launch.n_pairs, H, dr)
        gb = bb / (ms_b * 1e-3) / 1e9
        bwd[tag] = {"kernels": ("k_bwd_merged (both roles of a node in one pass over its row, dr form)" if dr
                                else "k_bwd_dst + k_bwd_src (one tmdnet_et_message_bwd call)"),
                    "ms_per_call": round(ms_b, 4), "bytes_per_call": bb, "achieved": round(gb, 1),
                    "frac": round(gb / HBM_PEAK_GBS, 4), "calls": nrep}
    res["backward"] = bwd
    fp = fused_projection_probe(launch, E, n_atoms, H, reps, dev,
                                {"message_forward_ms": ms_p, "merged_backward_ms": bwd["dr_force_form"]["ms_per_call"]})
    if fp is not None:
        res["fused_projection"] = fp
    if not a.no_pmc:
        pm, why = pmc_counters(a)
        if pm is None:
            res["traffic_detail"] = why
        else:
            g = pm.get("pairs", {})
            res["traffic"] = g.get("traffic")
            res["traffic_detail"] = {**g, "source": PMC_SOURCE}
            if g.get("traffic"):
                res["traffic_detail"]["traffic_over_bytes"] = round(g["traffic"] / pbytes, 3)
            per_edge["pmc"] = pm.get("per_edge")
            if fp is not None:
                fp["forward"]["pmc"] = pm.get("fused_fwd")
                fp["backward_dr"]["pmc"] = {k: pm.get(k) for k in ("fused_bwd_dst", "fused_edge_combine", "fused_bwd_src")}
            for tag, keys in (("training_form", ("bwd_dst", "bwd_src")), ("dr_force_form", ("bwd_dr",))):
                bwd[tag]["pmc"] = {k: pm.get(k) for k in keys}
                tr = sum((pm.get(k) or {}).get("traffic") or 0 for k in keys)
                if tr:
                    bwd[tag]["traffic_over_bytes"] = round(tr / bwd[tag]["bytes_per_call"], 3)
            res["_tn_pmc"] = {k: pm.get(k) for k in ("tn_msg_fwd", "tn_msg_bwd_pair", "tn_msg_bwd_src")}
    return res


def fused_setup(launch, H, dev, R=64):
    """The probe graph's inputs for the fused dk/dv-projection kernels (csrc/et_fused.hip), the path the
    model takes on C5-size graphs (et_stack.FEP_MIN_EDGES): one layer's split weight image, the
    evaluation's RBF fragments per pair row, and launchers of the forward and the force-pass backward."""
    from torchmdnet import kernels
    q, k, v, vec, C, u = launch.inputs
    if not kernels.fep_supported(H, 8, R, q.dtype):
        return None
    g = launch.graph
    N = q.shape[0]
    r = g.distances.detach()
    gen = torch.Generator(device=dev).manual_seed(11)
    W = torch.randn(4 * H, R, device=dev, generator=gen) / R ** 0.5
    b = torch.randn(4 * H, device=dev, generator=gen) * 0.1
    start = math.exp(-5.0)
    mu = torch.linspace(start, 1.0, R, device=dev)
    beta = torch.full((R,), (2.0 / R * (1 - start)) ** -2, device=dev)
    fep = kernels.fep_split(W, b)
    frag = kernels.fep_frag_set(g, r, (mu, beta, 0.0, 5.0, 0), (launch.pair_row, launch.pair_edge))
    xo, vo = torch.empty(N, H, device=dev), torch.empty(N, 3, H, device=dev)
    gx, gvec = torch.randn(N, H, device=dev, generator=gen), torch.randn(N, 3, H, device=dev, generator=gen)
    E = g.n_edges
    bufs = [torch.empty(N, H, device=dev), torch.empty(N, H, device=dev), torch.empty(N, 3 * H, device=dev),
            torch.empty(N, 3, H, device=dev), torch.zeros(E, device=dev), torch.zeros(E, 3, device=dev),
            torch.zeros(E, device=dev)]

    class F:
        pass
    f = F()
    f.R = R
    # the unfused counterparts' projection GEMMs over the P pair rows (tmdnet_proj_f32, as the model issues them)
    f_pairs = kernels.rbf_composite(r.index_select(0, launch.pair_edge.long()), mu, beta, 0.0, 5.0, 0).contiguous()
    wp = kernels.proj_split(W)
    f.proj = lambda: kernels.proj(f_pairs, W, b, wp=wp)
    f.dproj = lambda: kernels.proj(kernels.rbf_deriv(r, mu, beta, 0.0, 5.0, 0, rows=launch.pair_edge), W, None, wp=wp)
    f.fwd = lambda: kernels.et_fused_fwd_launch(q, k, v, vec, C, u, fep, frag, g, 8, xo, vo, flags=4)
    f.bwd = lambda: kernels.et_fused_bwd_launch(q, k, v, vec, C, u, fep, frag, g, 8, gx, gvec, *bufs,
                                                accumulate=1 | 2 | 4)
    f.frags = lambda: kernels.fep_frag_set(g, r, (mu, beta, 0.0, 5.0, 0), (launch.pair_row, launch.pair_edge))
    return f


def _event_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    for _ in range(reps):
        fn()
    b0.record()
    torch.cuda.synchronize()
    return a0.elapsed_time(b0) / reps


def fused_projection_probe(launch, E, N, H, reps, dev, unfused):
    """The ET message with the dk/dv projection FUSED into the edge kernels (tmdnet_et_fused_fwd_f32 /
    _bwd_f32, csrc/et_fused.hip) on the probe graph -- what the model runs per layer at C5 (E >= 131072,
    et_stack.FEP_MIN_EDGES): the RBF of r as fp16 MFMA fragments (formed once per evaluation, shared by the
    layers), [dk|dv] = W f + b (and d/dr = W f' in the backward) on the fp16 MFMA from an exact two-piece
    split (3 products per term), no projection rows written or read.  Against the unfused pair-row layout:
    forward = projection GEMM + message kernel, force-pass backward = d(dk,dv)/dr GEMM + merged dr pass.
    Rooflines: algorithmic bytes over HBM and the MFMA work over the dense fp16 peak."""
    f = fused_setup(launch, H, dev)
    if f is None:
        return None
    R = f.R
    ms = _event_ms(f.fwd, reps)
    ms_b = _event_ms(f.bwd, max(4, reps // 2))
    ms_fr = _event_ms(f.frags, 10)
    P = launch.n_pairs
    # edge scalars (src, fragment row, cutoff, unit vector), the P distinct fragment rows (two fp16 pieces of
    # R values), node rows q, k, v, vec read and x, vec written, row_ptr
    nbytes = E * (4 + 4 + 4 + 12) + P * 4 * R + N * (12 * H * 4 + 4)
    flop = 3 * 2.0 * E * R * 4 * H  # fp16 MFMA products (hi*hi, hi*lo, lo*hi)
    bbytes = E * (4 + 4 + 4 + 12) + N * 4 + P * (8 * R + 4)  # edge scalars, B and D fragment rows + scale
    bbytes += N * (H + H + 3 * H + 3 * H + H + 3 * H) * 4 + N * (H + H + 3 * H + 3 * H) * 4  # node rows in / out
    bbytes += 2 * E * (4 + 12) + 2 * E * 4                                              # g_cut, g_unit, g_r
    bflop = 3 * 2.0 * E * R * 4 * H * 3  # pre + d pre/dr (destination pass), pre again (source pass)
    res = {"kernels": "tmdnet_et_fused_fwd_f32 (fep::k_fwd, 4 heads per work item, 8 waves, one workgroup per CU, "
                      "XCD-interleaved node chunks) and tmdnet_et_fused_bwd_f32 (fep::k_bwd_dst + k_edge_combine + "
                      "k_bwd_src)",
           "model_path": "C5 energy+forces per layer (et_stack.FEP / FEP_BWD, E >= 131072)",
           "forward": {"ms_per_launch": round(ms, 4), "bytes_per_launch": nbytes,
                       "achieved_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1),
                       "frac_hbm": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "mfma_flop_per_launch": flop, "achieved_tflops_f16": round(flop / (ms * 1e-3) / 1e12, 1),
                       "peak_tflops_f16": MFMA_BF16_PEAK_TFS,
                       "frac_mfma": round(flop / (ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFS, 4)},
           "backward_dr": {"ms_per_call": round(ms_b, 4), "bytes_per_call": bbytes,
                           "achieved_gbs": round(bbytes / (ms_b * 1e-3) / 1e9, 1),
                           "frac_hbm": round(bbytes / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "mfma_flop_per_call": bflop,
                           "achieved_tflops_f16": round(bflop / (ms_b * 1e-3) / 1e12, 1),
                           "frac_mfma": round(bflop / (ms_b * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFS, 4)},
           "fragments_per_evaluation_ms": round(ms_fr, 4),
           "bound": "latency of the dependent per-tile gathers (r04 PMC, profiles/r04_fep_{fwd,bwd}_pmc.txt: most wave "
                    "cycles parked on memory waits, VALU and MFMA well below their issue rates)"}
    if unfused:
        t_proj, t_dproj = _event_ms(f.proj, 10), _event_ms(f.dproj, 10)
        uf = round(unfused["message_forward_ms"] + t_proj, 4)
        ub = round(unfused["merged_backward_ms"] + t_dproj, 4)
        res["vs_unfused"] = {"unfused_forward_ms": uf, "unfused_backward_dr_ms": ub,
                             "forward_speedup": round(uf / ms, 3) if uf else None,
                             "backward_speedup": round(ub / ms_b, 3) if ub else None,
                             "projection_gemm_ms": round(t_proj, 4), "dr_projection_ms": round(t_dproj, 4),
                             "unfused": "forward = tmdnet_proj_f32 over the P pair rows + k_fwd (pair layout); backward = "
                                        "d RBF/dr + the d(dk,dv)/dr GEMM over the pair rows + k_bwd_merged"}
    return res


def mfma_probe(E_c5, N_c5, E_c2, N_c2, H, R, dev):
    """MFMA utilisation of the feature-mix GEMMs (north_star: 'MFMA utilisation on the feature mixes
    against gfx950 peak'): the dk/dv projection Linear_{R->4H} (the largest FLOP term, SURVEY.md 8(a)
    a13) as the model issues it -- over the (E + N) / 2 edge PAIRS (both directions share a row,
    et_stack.PAIR_ROWS), per layer at C5 scale, all 8 layers stacked into one GEMM at C2 -- fp32
    in/out, HIP-event timed: the library fp32 GEMM (hipBLASLt on v_mfma_f32_16x16x4_f32) and the
    model's tmdnet_proj_f32 (bf16 MFMA on an exact three-piece split, fp32 accuracy: both arms' max
    error against fp64 is reported)."""
    from torchmdnet import kernels
    res = {}
    for tag, E, cols in (("c5_per_layer", (E_c5 + N_c5) // 2, 4 * H),
                         ("c2_stacked_8_layers", (E_c2 + N_c2) // 2, 8 * 4 * H)):
        gen = torch.Generator(device=dev).manual_seed(5)
        f = torch.rand(E, R, device=dev, generator=gen)  # RBF values lie in [0, 1]
        w = torch.randn(cols, R, device=dev, generator=gen) / R ** 0.5
        b = torch.randn(cols, device=dev, generator=gen)
        out = torch.empty(E, cols, device=dev)
        row = {"gemm": f"[{E} x {R}] @ [{R} x {cols}] + bias, fp32 in/out", "output_bytes": E * cols * 4,
               "output_write_bound_ms": round(E * cols * 4 / (HBM_PEAK_GBS * 1e9) * 1e3, 4)}
        ref = None
        if E < 100000:  # fp64 reference for the accuracy of both arms
            ref = torch.addmm(b.double(), f.double(), w.double().t())
        wp = kernels.proj_split(w)  # once per forward in the model, shared by the projection GEMMs
        for arm, fn in (("library_fp32", lambda: torch.addmm(b, f, w.t(), out=out)),
                        ("bf16x6_split", lambda: kernels.proj(f, w, b, out=out, wp=wp)),
                        ("weight_split", lambda: kernels.proj_split(w))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps = 10 if E > 100000 else 50
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            tf = 2.0 * E * R * cols / (ms * 1e-3) / 1e12
            r = {"ms_per_launch": round(ms, 4), "achieved": round(tf, 2), "frac": round(tf / MFMA_F32_PEAK_TFS, 4),
                 "write_gbs": round(E * cols * 4 / (ms * 1e-3) / 1e9, 1)}
            if arm == "weight_split":
                row[arm] = {"ms_per_launch": round(ms, 4)}
                continue
            if arm == "bf16x6_split":  # six bf16 MFMA products per fp32 product
                r["bf16_mfma_tfs"] = round(6 * tf, 1)
                r["bf16_mfma_frac"] = round(6 * tf / MFMA_BF16_PEAK_TFS, 4)
            if ref is not None:
                r["max_abs_err_vs_fp64"] = float((out.double() - ref).abs().max())
            row[arm] = r
        # headline fields = the arm the model runs (kernels.PROJ)
        row.update({k: row["bf16x6_split" if kernels.PROJ == "x3" else "library_fp32"][k]
                    for k in ("ms_per_launch", "achieved", "frac")})
        res[tag] = row
        del f, w, b, out, ref, wp
    # the hand-written grouped node-mix GEMM (tmdnet_gemm_f32, csrc/gemm.hip) at the C2 metric batch:
    # forward [q|k|v] + vec_proj in one launch, backward [q|k|v]^T + vec_proj^T (K split over 16 waves)
    Hh, Na = H, N_c2
    gen = torch.Generator(device=dev).manual_seed(6)
    rn = lambda *sh: torch.randn(*sh, device=dev, generator=gen)  # noqa: E731
    xn, vec, wq, wv = rn(Na, Hh), rn(3 * Na, Hh), rn(5 * Hh, Hh), rn(3 * Hh, Hh)
    qkv, vecp = torch.empty(Na, 5 * Hh, device=dev), torch.empty(3 * Na, 3 * Hh, device=dev)
    gxn, gvec = torch.empty(Na, Hh, device=dev), torch.empty(3 * Na, Hh, device=dev)
    node = {}
    for tag, probs, flop in (
            ("forward_qkv_vecproj", [(xn, wq, True, None, qkv, False), (vec, wv, True, None, vecp, False)],
             2.0 * Na * 5 * Hh * Hh + 2.0 * 3 * Na * 3 * Hh * Hh),
            ("backward_qkvT_vecprojT", [(qkv, wq, False, None, gxn, False), (vecp, wv, False, None, gvec, True)],
             2.0 * Na * 5 * Hh * Hh + 2.0 * 3 * Na * 3 * Hh * Hh)):
        for _ in range(5):
            kernels.gemm_group(probs)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            kernels.gemm_group(probs)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 100
        tf = flop / (ms * 1e-3) / 1e12
        node[tag] = {"ms_per_launch": round(ms, 5), "flop": flop, "achieved": round(tf, 2),
                     "frac": round(tf / MFMA_F32_PEAK_TFS, 4)}
    res["node_mix_c2"] = {"kernel": "tmdnet_gemm_f32 (grouped split-K fp32 MFMA, csrc/gemm.hip)",
                          "shape": f"N={Na} atoms, H={Hh}: [N x H][H x 5H] + [3N x H][H x 3H] per launch", **node}
    return {"kernel": "dk/dv projection GEMM (SURVEY 8(a) a13)", "bound": "mfma", "unit": "TFLOP/s",
            "peak": MFMA_F32_PEAK_TFS,
            "dtype": "fp32 in/out (the reference computes in fp32); tmdnet_proj_f32 forms it from exact bf16 pieces",
            **res}


def phase(msg):
    """Progress line on stderr (the JSON result line is the only stdout output)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs writes at most this much in all


def dump_outputs(out_dir, arrays, rank):
    """--dump-outputs: the tensors the last timed step returned as out_dir/<name>.npy (rank r > 0:
    <name>_rank<r>.npy), float32 (float64 stays float64).  An array over its share of DUMP_MAX_BYTES is
    written as a fixed sample of its flattened elements (seeded index set, ascending order)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        t = t.detach().to("cpu")
        x = (t if t.dtype == torch.float64 else t.float()).contiguous().numpy()
        if x.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(x.size, share // x.itemsize, replace=False))
            x = x.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ("" if rank == 0 else f"_rank{rank}") + ".npy"), x)


def timed_loop(step, warmup, steps, ws, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    barrier(ws)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    barrier(ws)
    return max_over_ranks(time.perf_counter() - t0, ws, dev)


def rmd17_like(n_mol, gen_seed):
    """aspirin C9H8O4 x n_mol, pos = randn * 1.6 A."""
    g = torch.Generator().manual_seed(gen_seed)
    z1 = torch.tensor([6] * 9 + [1] * 8 + [8] * 4, dtype=torch.long)
    z = z1.repeat(n_mol)
    pos = torch.randn(z.shape[0], 3, generator=g, dtype=torch.float64) * 1.6
    batch = torch.arange(n_mol, dtype=torch.long).repeat_interleave(z1.shape[0])
    return z, pos, batch


def spice_like(n_mol, gen_seed):
    """SPICE-like, 16 x 40 atoms, z = randint(1, 9), pos = randn * 2.5 A."""
    g = torch.Generator().manual_seed(gen_seed)
    z = torch.randint(1, 9, (n_mol * 40,), generator=g)
    pos = torch.randn(n_mol * 40, 3, generator=g, dtype=torch.float64) * 2.5
    batch = torch.arange(n_mol).repeat_interleave(40)
    return z, pos, batch


def spice_model_args():
    import yaml
    with open(os.path.join(ROOT, "tests", "golden", "configs", "et_spice.yaml")) as f:
        args = yaml.safe_load(f)
    args.update(prior_model=None, precision=32, derivative=True, output_model="Scalar")
    return args


def secondary_spice(a, ws, rank, dev):
    """C4: ET-SPICE (examples/ET-SPICE.yaml: 128 ch, 5 layers, cutoff 10, 128 neighbours), 16 x 40-atom
    molecules per GPU: energy + forces, HIP-graph replay."""
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_model
    torch.manual_seed(0)
    model = create_model(spice_model_args()).to(dev)
    n_mol = 16
    z, pos, batch = spice_like(n_mol, 1 + rank)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    gm = GraphedEnergyForces(model, z, pos, batch)
    el = timed_loop(lambda: gm(pos), a.warmup, a.steps, ws, dev)
    gm.check_capacity()
    gm.release()
    return {"workload": "ET-SPICE energy+forces (C4: 16 x 40 atoms, 5 layers, cutoff 10), hip-graph replay",
            "value": round(n_mol * ws * a.steps / el, 2), "unit": "molecules/s",
            "ms_per_step": round(1000 * el / a.steps, 4), "atoms_per_gpu": int(z.shape[0])}


def ddp_train(a, ws, rank, dev):
    """The data-parallel training step of SURVEY.md 8(e) at this N: ET-SPICE C4 (16 x 40 atoms per
    GPU, y / neg_dy weights 0.5 / 0.5 of ET-SPICE.yaml), forward + force pass + double backward
    replayed from one HIP graph per rank, ONE fused RCCL all-reduce of the 4.9 MB gradient, fused
    AdamW.  Every rank starts from rank 0's weights (broadcast) with its own molecules."""
    from torchmdnet.models.model import create_model
    from torchmdnet.training import GraphedTrainStep
    torch.manual_seed(0)
    model = create_model(spice_model_args()).to(dev)
    n_mol = 16
    z, pos, batch = spice_like(n_mol, 1 + rank)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    gy = torch.Generator().manual_seed(200 + rank)
    y_lab = torch.randn(n_mol, 1, generator=gy).to(dev)
    f_lab = torch.randn(z.shape[0], 3, generator=gy).to(dev)
    tr = GraphedTrainStep(model, z, pos, batch, y_lab, f_lab, lr=1e-4, y_weight=0.5, neg_dy_weight=0.5)
    nparam = int(tr.reduce.flat.numel() - 1)
    steps = a.steps
    el = timed_loop(lambda: tr.step(), a.warmup, steps, ws, dev)
    tr.check_capacity()
    tr.release()
    return {"workload": "ET-SPICE training step (C4: 16 x 40 atoms per GPU, E+F MSE 0.5/0.5, double backward"
                        + (", ONE fused RCCL all-reduce" if ws > 1 else "") + ", fused AdamW)",
            "value": round(n_mol * ws * steps / el, 2), "unit": "molecules/s", "n_gpus": ws,
            "ms_per_step": round(1000 * el / steps, 4), "steps": steps, "scaling": "weak",
            "parallelism": f"dp{ws}", "grad_allreduce_bytes": nparam * 4,
            "execution": "fwd + force pass + double backward in one HIP graph per rank; all-reduce + AdamW eager",
            "edge_capacity": tr.edge_capacity}


def secondary_tensornet(a, ws, rank, dev):
    """C3: TensorNet-rMD17 (8 x 21 atoms, O(3), static_shapes as the reference default), energy +
    forces, HIP-graph replay, molecules/s over all ranks."""
    import yaml
    from torchmdnet.graphs import GraphedEnergyForces
    from torchmdnet.models.model import create_model
    with open(os.path.join(ROOT, "tests", "golden", "configs", "tensornet_rmd17.yaml")) as f:
        args = yaml.safe_load(f)
    args.update(prior_model=None, precision=32, derivative=True)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    n_mol = 8
    z, pos, batch = rmd17_like(n_mol, 1 + rank)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    gm = GraphedEnergyForces(model, z, pos, batch)
    el = timed_loop(lambda: gm(pos), a.warmup, a.steps, ws, dev)
    gm.check_capacity()
    gm.release()
    return {"workload": "TensorNet-rMD17 energy+forces (C3: 8 x aspirin, O(3), static_shapes), hip-graph replay",
            "value": round(n_mol * ws * a.steps / el, 2), "unit": "molecules/s",
            "ms_per_step": round(1000 * el / a.steps, 4), "atoms_per_gpu": int(z.shape[0])}


def secondary_scripted(a, ws, rank, dev):
    """The bench model (C2 ET-QM9, 32 molecules per GPU) as torch.jit.script(model) -- the form MD
    engines load (reference README.md:6, tests/test_model.py:42-84) -- energy + forces, eager.  Eval mode
    (the MD-engine form) runs the whole evaluation as ONE operator (tmdnet::et_energy_forces); train mode
    keeps the differentiable operator path (tmdnet::neighbor_graph, edge_geometry, nbr_embed, et_stack).
    Beside them the same model unscripted and eager (the headline replays a HIP graph)."""
    from torchmdnet.models.model import create_model
    torch.manual_seed(0)
    model = create_model(et_args(a.channels)).to(dev)
    z, pos, batch = qm9_like(a.batch, gen_seed=1 + rank)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    steps = max(10, a.steps)
    scripted = torch.jit.script(model)  # train mode (the module default)
    el_t = timed_loop(lambda: scripted(z, pos, batch), a.warmup, steps, ws, dev)
    el_e = timed_loop(lambda: model(z, pos, batch), a.warmup, steps, ws, dev)
    model.eval()
    # eval mode, unscripted: the layers through the C++ et_stack operator (torchmd_et.CPP_EAGER)
    el_ev = timed_loop(lambda: model(z, pos, batch), a.warmup, steps, ws, dev)
    scripted_eval = torch.jit.script(model)
    el_s = timed_loop(lambda: scripted_eval(z, pos, batch), a.warmup, steps, ws, dev)
    return {"workload": "ET-QM9 energy+forces (C2 batch) through torch.jit.script(model.eval()), eager",
            "value": round(a.batch * ws * steps / el_s, 2), "unit": "molecules/s",
            "ms_per_step": round(1000 * el_s / steps, 4),
            "path": "eval mode: the whole evaluation as ONE tmdnet::et_energy_forces operator (the eager path's "
                    "launches issued from C++, no autograd graph)",
            "train_mode_ms_per_step": round(1000 * el_t / steps, 4),
            "train_mode_path": "dispatcher ops (tmdnet::neighbor_graph, edge_geometry, nbr_embed) + the interaction "
                               "layers as ONE differentiable tmdnet::et_stack operator",
            "eager_unscripted_ms_per_step": round(1000 * el_e / steps, 4),
            "eager_unscripted_eval_ms_per_step": round(1000 * el_ev / steps, 4),
            "eager_unscripted_eval_path": "model.eval(), unscripted: the interaction layers as the C++ "
                                          "tmdnet::et_stack operator (differentiable), the rest Python autograd"}


def secondary_water_box(a, ws, rank, dev):
    """C5: ET (the bench model: 128 ch, 8 layers, cutoff 5) on a periodic ~50k-atom water box,
    energy + forces through TorchMD_Net (cell-list neighbour search in the box, Morton renumbering,
    fused layer stack with planar rows), eager; one system per GPU (replicas)."""
    from torchmdnet.models.model import create_model
    n = a.roofline_atoms
    args = et_args(a.channels)
    args.update(max_num_neighbors=128)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    rep_ = model.representation_model
    g = torch.Generator().manual_seed(7 + rank)
    L = (n / 0.1003) ** (1.0 / 3.0)
    pos = (torch.rand(n, 3, generator=g, dtype=torch.float64) * L).float().to(dev)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3 + 1)[:n].to(dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    d = rep_.distance  # periodic box + cell list, as benchmarks/inference.py configures OptimizedDistance
    d.box = torch.eye(3, dtype=torch.float32) * L
    d.use_periodic = True
    d.strategy = "cell"
    steps = max(3, a.steps // 10)
    el = timed_loop(lambda: model(z, pos, batch), 2, steps, ws, dev)
    return {"workload": f"ET water box, {n} atoms, periodic L={L:.1f} A, energy+forces, eager (C5)",
            "value": round(n * ws * steps / el, 1), "unit": "atoms/s", "ms_per_step": round(1000 * el / steps, 3),
            "edges": int(d.last_num_pairs.item()) if torch.is_tensor(d.last_num_pairs) else d.last_num_pairs}


def tn_args():
    import yaml
    with open(os.path.join(ROOT, "tests", "golden", "configs", "tensornet_rmd17.yaml")) as f:
        args = yaml.safe_load(f)
    args.update(prior_model=None, precision=32, derivative=True)
    return args


def tn_water_box_model(n, static_shapes, seed, dev, precision=32):
    """C5's TensorNet arm: the TensorNet-rMD17 architecture (128 ch, 2 layers, 32 RBF, cutoff 4.5, O(3);
    the model reference benchmarks/inference.py:63-71 times) on a periodic n-atom water box (SURVEY §8(d):
    z = (8,1,1) repeated, pos = rand * L, L = (n/0.1003)^(1/3)), cell list, max_num_neighbors 64 (the 32 of
    inference.py would overflow at water density).  Returns (model, z, pos, batch, L) on dev."""
    from torchmdnet.models.model import create_model
    args = tn_args()
    args.update(max_num_neighbors=64, precision=precision)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    rep_ = model.representation_model
    rep_.static_shapes = static_shapes  # (create_model keeps TensorNet's default True, as the reference's)
    rep_.distance.resize_to_fit = not static_shapes
    g = torch.Generator().manual_seed(7 + seed)
    L = (n / 0.1003) ** (1.0 / 3.0)
    dt = torch.float64 if precision == 64 else torch.float32
    pos = (torch.rand(n, 3, generator=g, dtype=torch.float64) * L).to(dt).to(dev)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3 + 1)[:n].to(dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    d = rep_.distance
    d.box = torch.eye(3, dtype=dt) * L
    d.use_periodic = True
    d.strategy = "cell"
    return model, z, pos, batch, L


def secondary_tn_water_box(a, ws, rank, dev):
    """C5, TensorNet arm: TensorNet-rMD17 architecture on the ~50k-atom periodic water
    box, energy + forces through TorchMD_Net, eager, static_shapes (reference default) and dynamic shapes;
    one system per GPU (replicas)."""
    n = a.roofline_atoms
    steps = max(3, a.steps // 10)
    out = {}
    for static in (True, False):
        model, z, pos, batch, L = tn_water_box_model(n, static, rank, dev)
        el = timed_loop(lambda: model(z, pos, batch), 2, steps, ws, dev)
        d = model.representation_model.distance
        out["static_shapes" if static else "dynamic_shapes"] = {
            "value": round(n * ws * steps / el, 1), "unit": "atoms/s", "ms_per_step": round(1000 * el / steps, 3),
            "edges": int(d.last_num_pairs.item()) if torch.is_tensor(d.last_num_pairs) else d.last_num_pairs}
        del model
    res = out["static_shapes"]
    return {"workload": f"TensorNet (rMD17 arch: 128 ch, 2 layers, 32 RBF, cutoff 4.5, O(3)) water box, {n} atoms, "
                        f"periodic L={L:.1f} A, cell list, energy+forces, eager (C5, benchmarks/inference.py model)",
            "value": res["value"], "unit": "atoms/s", "ms_per_step": res["ms_per_step"], **out}


def secondary_scripted_water_box(a, ws, rank, dev, eager_ms=None):
    """C5 as the MD-engine form: torch.jit.script(model) in eval mode on the same water box -- the whole
    energy + force evaluation as ONE tmdnet::et_energy_forces operator with the large-system forms (Morton
    renumbering, pair rows, planar v, fused-projection layers, x3 GEMMs) issued from C++."""
    from torchmdnet.models.model import create_model
    n = a.roofline_atoms
    args = et_args(a.channels)
    args.update(max_num_neighbors=128)
    torch.manual_seed(0)
    model = create_model(args).to(dev).eval()
    g = torch.Generator().manual_seed(7 + rank)
    L = (n / 0.1003) ** (1.0 / 3.0)
    pos = (torch.rand(n, 3, generator=g, dtype=torch.float64) * L).float().to(dev)
    z = torch.tensor([8, 1, 1], dtype=torch.long).repeat(n // 3 + 1)[:n].to(dev)
    batch = torch.zeros(n, dtype=torch.long, device=dev)
    d = model.representation_model.distance
    d.box = torch.eye(3, dtype=torch.float32) * L
    d.use_periodic = True
    d.strategy = "cell"
    scripted = torch.jit.script(model)
    steps = max(3, a.steps // 10)
    el = timed_loop(lambda: scripted(z, pos, batch), 2, steps, ws, dev)
    ms = 1000 * el / steps
    out = {"workload": f"ET water box, {n} atoms, periodic L={L:.1f} A, energy+forces, torch.jit.script eval "
                       "(tmdnet::et_energy_forces, one operator)",
           "value": round(n * ws * steps / el, 1), "unit": "atoms/s", "ms_per_step": round(ms, 3)}
    if eager_ms:
        out["ratio_to_eager"] = round(ms / eager_ms, 3)
    return out


def secondary_train(a, ws, rank, dev):
    """ET-QM9 training step (E+F MSE with forces via create_graph, backward incl. the double
    backward, one fused RCCL all-reduce of the gradients when ws > 1, AdamW)."""
    from torchmdnet.models.model import create_model
    from torchmdnet.training import LNNPStep
    torch.manual_seed(0)
    model = create_model(et_args(a.channels)).to(dev)
    z, pos, batch = qm9_like(a.batch, gen_seed=1 + rank)
    gy = torch.Generator().manual_seed(100 + rank)
    y_lab = torch.randn(a.batch, 1, generator=gy).to(dev)
    f_lab = torch.randn(z.shape[0], 3, generator=gy).to(dev)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    from torchmdnet.training import GraphedTrainStep
    steps = max(10, a.steps // 2)
    phase("train: eager steps")
    trainer = LNNPStep(model, lr=4e-4)
    el = timed_loop(lambda: trainer.step(z, pos, batch, y_lab, f_lab), max(3, a.warmup // 2), steps, ws, dev)
    res = {"workload": "ET-QM9 training step (E+F MSE, double backward, "
                       + ("fused RCCL all-reduce, " if ws > 1 else "") + "AdamW), eager",
           "value": round(a.batch * ws * steps / el, 2), "unit": "molecules/s",
           "ms_per_step": round(1000 * el / steps, 4), "steps": steps, "parallelism": f"dp{ws}"}
    if a.graphed_train:
        phase("train: graph-captured step")
        del trainer
        try:
            gtr = GraphedTrainStep(model, z, pos, batch, y_lab, f_lab, lr=4e-4)
            el = timed_loop(lambda: gtr.step(), max(3, a.warmup // 2), steps, ws, dev)
            gtr.check_capacity()
            gtr.release()
            res["graphed"] = {
                "value": round(a.batch * ws * steps / el, 2), "unit": "molecules/s",
                "ms_per_step": round(1000 * el / steps, 4), "edge_capacity": gtr.edge_capacity,
                "execution": "fwd + force pass + double backward in one HIP graph; "
                             + ("RCCL all-reduce + " if ws > 1 else "") + "fused AdamW eager"}
        except RuntimeError as exc:  # the eager line above stands on its own
            res["graphed"] = {"error": str(exc)[:300]}
    return res


def secondary_tn_train(a, ws, rank, dev):
    """C3 training: TensorNet-rMD17 (8 x aspirin, O(3), static_shapes) E + F MSE step -- forces by
    create_graph, the double backward through the hand-written second order (tmdnet_tn_node_bwd2, the
    GEMM / message second orders) -- eager and as one HIP-graph replay (GraphedTrainStep) + AdamW."""
    import yaml
    from torchmdnet.models.model import create_model
    from torchmdnet.training import GraphedTrainStep, LNNPStep
    with open(os.path.join(ROOT, "tests", "golden", "configs", "tensornet_rmd17.yaml")) as f:
        args = yaml.safe_load(f)
    args.update(prior_model=None, precision=32, derivative=True)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    n_mol = 8
    z, pos, batch = rmd17_like(n_mol, 1 + rank)
    gy = torch.Generator().manual_seed(300 + rank)
    y_lab = torch.randn(n_mol, 1, generator=gy).to(dev)
    f_lab = torch.randn(z.shape[0], 3, generator=gy).to(dev)
    z, pos, batch = z.to(dev), pos.float().to(dev), batch.to(dev)
    steps = max(10, a.steps // 2)
    trainer = LNNPStep(model, lr=4e-4)
    el = timed_loop(lambda: trainer.step(z, pos, batch, y_lab, f_lab), max(3, a.warmup // 2), steps, ws, dev)
    res = {"workload": "TensorNet-rMD17 training step (C3: 8 x aspirin, E+F MSE, double backward, AdamW), eager",
           "value": round(n_mol * ws * steps / el, 2), "unit": "molecules/s",
           "ms_per_step": round(1000 * el / steps, 4), "steps": steps, "parallelism": f"dp{ws}"}
    if a.graphed_train:
        del trainer
        try:
            gtr = GraphedTrainStep(model, z, pos, batch, y_lab, f_lab, lr=4e-4)
            el = timed_loop(lambda: gtr.step(), max(3, a.warmup // 2), steps, ws, dev)
            gtr.check_capacity()
            gtr.release()
            res["graphed"] = {"value": round(n_mol * ws * steps / el, 2), "unit": "molecules/s",
                              "ms_per_step": round(1000 * el / steps, 4),
                              "execution": "fwd + force pass + double backward in one HIP graph; fused AdamW eager"}
        except RuntimeError as exc:
            res["graphed"] = {"error": str(exc)[:300]}
    return res


def write_custom_dataset(root, n_mol, gen_seed):
    """SURVEY.md 8(d) QM9-like molecules in the reference's Custom npy format (datasets/custom.py:
    one coordinate / embedding / energy / force file per molecule size, frames of that size), with
    random labels: the on-disk input of the fit() line."""
    import numpy as np
    z, pos, batch = qm9_like(n_mol, gen_seed)
    g = torch.Generator().manual_seed(gen_seed + 1000)
    groups = {}
    for m in range(n_mol):
        sel = batch == m
        zi, pi = z[sel], pos[sel].float()
        key = (int(zi.shape[0]), tuple(zi.tolist()))
        groups.setdefault(key, []).append(pi)
    os.makedirs(root, exist_ok=True)
    for i, ((n, zs), frames) in enumerate(sorted(groups.items())):
        c = torch.stack(frames).numpy()
        np.save(os.path.join(root, f"coords_{i:04d}.npy"), c)
        np.save(os.path.join(root, f"embed_{i:04d}.npy"), np.asarray(zs, dtype=np.int64))
        np.save(os.path.join(root, f"energy_{i:04d}.npy"), torch.randn(len(frames), 1, generator=g).numpy())
        np.save(os.path.join(root, f"forces_{i:04d}.npy"), torch.randn(c.shape, generator=g).float().numpy())
    return root


def secondary_fit(a, ws, rank, dev):
    """fit()-style training on the real data path: QM9-like molecules on disk in the
    Custom npy format -> DataModule (splits, FloatCast, per-rank ShardSampler, DataLoader workers) ->
    variable-size batches padded to an atom capacity (training.PaddedBatches, one captured step per
    capacity) -> ONE graph replay per step + fused AdamW.  The timed region includes the host loader
    (sampling, file reads, collation, padding, pinned H2D copy).  Beside it: the loader alone, and the
    fixed-layout graphed step on the same model and batch size (et_train_step.graphed)."""
    import tempfile
    from torchmdnet.data import DataModule
    from torchmdnet.models.model import create_model
    from torchmdnet.module import default_atom_buckets
    from torchmdnet.training import PaddedBatches, PaddedGraphedTrainer
    steps = max(20, a.steps)
    n_mol = a.batch * (a.warmup + steps + 8) * 2
    tmp = tempfile.mkdtemp(prefix="tmd_fit_")
    root = write_custom_dataset(os.path.join(tmp, f"r{rank}"), n_mol, 50 + rank)
    hp = dict(dataset="Custom", coord_files=os.path.join(root, "coords_*.npy"),
              embed_files=os.path.join(root, "embed_*.npy"), energy_files=os.path.join(root, "energy_*.npy"),
              force_files=os.path.join(root, "forces_*.npy"), batch_size=a.batch, inference_batch_size=a.batch,
              train_size=0.95, val_size=0.05, test_size=0, seed=1, num_workers=4, precision=32)
    dm = DataModule(hp, rank=rank, world_size=ws)
    dm.setup()
    torch.manual_seed(0)
    model = create_model(et_args(a.channels)).to(dev)
    buckets = default_atom_buckets(dm.train_dataset, a.batch)
    pb = PaddedBatches(buckets, a.batch, 5.0)
    tr = PaddedGraphedTrainer(model, pb, lr=4e-4, y_weight=0.05, neg_dy_weight=0.95)
    loader = dm.loader("train", pb.collate)
    # the loader alone (host cost per batch, workers prefetching)
    t0 = time.perf_counter()
    nb = 0
    for b in loader:
        nb += 1
        if nb >= steps:
            break
    loader_ms = 1000 * (time.perf_counter() - t0) / nb
    it = iter(loader)

    def step():
        nonlocal it
        try:
            b = next(it)
        except StopIteration:
            it = iter(loader)
            b = next(it)
        tr.step(b)

    # warm-up until no new capacity has been captured for 16 steps (captures are one-time costs of an epoch)
    quiet, n_warm = 0, 0
    while quiet < 16 and n_warm < 200:
        nb0 = len(tr.steps) + tr.recaptures
        step()
        n_warm += 1
        quiet = quiet + 1 if len(tr.steps) + tr.recaptures == nb0 else 0
    el = timed_loop(step, 0, steps, ws, dev)
    tr.finish()
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return {"workload": "ET-QM9 force-matching training through DataModule (Custom npy files, 4 loader workers, "
                        "variable-size batches padded to atom buckets, one graph replay per step, fused AdamW)",
            "value": round(a.batch * ws * steps / el, 2), "unit": "molecules/s",
            "ms_per_step": round(1000 * el / steps, 4), "steps": steps, "loader_ms_per_batch": round(loader_ms, 4),
            "atom_buckets": buckets, "captured_buckets": sorted(tr.steps), "recaptures": tr.recaptures,
            "edge_capacities": {k: v.edge_capacity for k, v in sorted(tr.steps.items())}}


def _time_cpu(fn, seconds, max_calls=200):
    fn()  # warm-up
    n = 0
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= max_calls:
            return n, el


def _cpu_sd(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def cpu_threads(info):
    """the CPU path on ALL physical host cores (torch.set_num_threads(n_phys)), within
    the CPUs this process may use; the OMP_NUM_THREADS share of the box is timed beside it."""
    phys = info["physical_cores_machine"] or info["affinity_cpus"]
    return max(1, min(phys, info["affinity_cpus"]))


def cpu_baseline(model, args, z, pos, batch, seconds):
    """C2 energy + forces with oracle/model_oracle.py on the host cores (the headline CPU line), on all
    physical cores; the same sample at the box's OMP_NUM_THREADS share is recorded beside it."""
    from oracle import model_oracle as O
    info = host_cpu_info()
    cores = cpu_threads(info)
    sd = _cpu_sd(model)
    mols = int(batch.max()) + 1
    share = info["threads_used"]
    run = lambda secs: _time_cpu(lambda: O.energy_forces(sd, dict(args), z, pos, batch, dtype=torch.float32,  # noqa: E731
                                                         create_graph=True), secs)
    torch.set_num_threads(cores)
    n, el = run(seconds)
    all_cores = {"value": round(mols * n / el, 2), "unit": "molecules/s", "cores": cores,
                 "sample": f"{n} calls, {el:.1f} s"}
    share_line = None
    if share != cores:
        torch.set_num_threads(share)
        n_s, el_s = run(seconds / 2)
        share_line = {"value": round(mols * n_s / el_s, 2), "unit": "molecules/s", "cores": share,
                      "sample": f"{n_s} calls, {el_s:.1f} s"}
    # the headline CPU figure is the FASTER of the two thread counts (on a box whose CPU bandwidth is
    # capped below its core count -- cgroup_cpu_quota -- threads on every physical core oversubscribe
    # the share and run slower); both are reported
    best = all_cores if share_line is None or all_cores["value"] >= share_line["value"] else share_line
    torch.set_num_threads(best["cores"])
    return {"value": best["value"], "unit": "molecules/s", "cores": best["cores"], "kind": "port",
            "host": info, "all_physical_cores": all_cores, "omp_share": share_line,
            "calibration": "profiles/r02_cpu_calibration.json (restatement vs the shimmed reference, same "
                           "8 cores of the build container)",
            "sample": f"oracle/model_oracle.py (PyTorch-CPU restatement of the reference ET path), energy+force "
                      f"calls on the same {mols} molecules / weights, float32, timed at {cores} and {share} "
                      f"threads; headline = the faster ({best['cores']} threads, {best['sample']})"}


def cpu_baseline_extra(a, model, args, z, pos, batch):
    """the CPU path on the other configs, each a bounded sample with the same thread
    count: C2 training step, C3 TensorNet-rMD17, C4 ET-SPICE, C5 as a 1500-atom periodic water box
    (the 50k-atom system is CPU-infeasible for the reference: its O(N^2) pair list needs > 62 GB
    above ~2k atoms)."""
    import yaml
    from oracle import model_oracle as O
    from torchmdnet.models.model import create_model
    secs = a.cpu_extra_seconds
    out = {}
    # C2 training step: E+F MSE (forces with create_graph), double backward, AdamW
    sd = _cpu_sd(model)
    pnames = {k for k, _ in model.named_parameters()}
    leaf = {k: (v.clone().requires_grad_(True) if k in pnames else v) for k, v in sd.items()}
    opt = torch.optim.AdamW([leaf[k] for k in sorted(pnames)], lr=4e-4)
    gy = torch.Generator().manual_seed(100)
    nmol = int(batch.max()) + 1
    y_lab = torch.randn(nmol, 1, generator=gy)
    f_lab = torch.randn(z.shape[0], 3, generator=gy)

    def train_step():
        opt.zero_grad()
        y, f = O.energy_forces(leaf, dict(args), z, pos, batch, dtype=torch.float32, create_graph=True)
        loss = torch.nn.functional.mse_loss(y, y_lab) + torch.nn.functional.mse_loss(f, f_lab)
        loss.backward()
        opt.step()
    n, el = _time_cpu(train_step, secs)
    out["c2_train_step"] = {"value": round(nmol * n / el, 2), "unit": "molecules/s",
                            "sample": f"{n} ET-QM9 training steps (E+F MSE, double backward, AdamW), {el:.1f} s"}
    # C3 TensorNet-rMD17, 8 x aspirin (reference CPU semantics: the CPU op never pads)
    with open(os.path.join(ROOT, "tests", "golden", "configs", "tensornet_rmd17.yaml")) as f:
        targs = yaml.safe_load(f)
    targs.update(prior_model=None, precision=32, derivative=True)
    torch.manual_seed(0)
    tm = create_model(targs)
    zt, pt, bt = rmd17_like(8, 1)
    n, el = _time_cpu(lambda: O.energy_forces(_cpu_sd(tm), dict(targs), zt, pt.float(), bt, dtype=torch.float32,
                                              static_shapes=False, create_graph=True), secs)
    out["c3_tensornet_rmd17"] = {"value": round(8 * n / el, 2), "unit": "molecules/s",
                                 "sample": f"{n} energy+force calls, 8 x aspirin, {el:.1f} s"}
    # C4 ET-SPICE, 16 x 40 atoms
    sargs = spice_model_args()
    torch.manual_seed(0)
    sm = create_model(sargs)
    zs, ps, bs = spice_like(16, 1)
    ssd = _cpu_sd(sm)
    n, el = _time_cpu(lambda: O.energy_forces(ssd, dict(sargs), zs, ps.float(), bs, dtype=torch.float32,
                                                    create_graph=True), secs)
    out["c4_et_spice"] = {"value": round(16 * n / el, 2), "unit": "molecules/s",
                          "sample": f"{n} energy+force calls, 16 x 40 atoms, {el:.1f} s"}
    # C5 water box at 1500 atoms (periodic, cutoff 5, ET-QM9 weights of the headline model)
    nb = 1500
    g = torch.Generator().manual_seed(7)
    L = (nb / 0.1003) ** (1.0 / 3.0)
    pw = (torch.rand(nb, 3, generator=g, dtype=torch.float64) * L).float()
    zw = torch.tensor([8, 1, 1], dtype=torch.long).repeat(nb // 3 + 1)[:nb]
    bw = torch.zeros(nb, dtype=torch.long)
    wargs = dict(args, box=[[L, 0, 0], [0, L, 0], [0, 0, L]])
    n, el = _time_cpu(lambda: O.energy_forces(sd, wargs, zw, pw, bw, dtype=torch.float32, create_graph=True),
                      secs)
    out["c5_water_box_1500"] = {"value": round(nb * n / el, 1), "unit": "atoms/s",
                                "sample": f"{n} energy+force calls, {nb}-atom periodic water box L={L:.1f} A, "
                                          f"{el:.1f} s",
                                "c5_50k": "CPU-infeasible for the reference (O(N^2) CPU pair list)"}
    return out


def main():
    a = parse()
    if a.pmc_child:  # profiled child of pmc_counters(): the probe kernels in the PMC_CHILD order
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        launch, _, _ = probe_workload(a.roofline_atoms, a.channels, dev)
        for _ in range(8):
            launch()
        for _ in range(8):
            launch.pairs()
        for _ in range(4):
            launch.bwd(False)
        for _ in range(4):
            launch.bwd(True)
        fp = fused_setup(launch, a.channels, dev)
        if fp is not None:
            for _ in range(8):
                fp.fwd()
            for _ in range(4):
                fp.bwd()
        torch.cuda.synchronize()
        del launch, fp
        tfwd, tbwd, *_ = tn_message_probe_setup(a.roofline_atoms, a.channels, dev)
        for _ in range(8):
            tfwd()
        for _ in range(4):
            tbwd()
        torch.cuda.synchronize()
        return
    maybe_spawn(a)
    ws, rank, dev = setup_dist()
    from torchmdnet import kernels
    from torchmdnet.models.model import create_model
    from torchmdnet.training import LNNPStep

    args = et_args(a.channels)
    torch.manual_seed(0)
    model = create_model(args).to(dev)
    z, pos, batch = qm9_like(a.batch, gen_seed=1 + rank)
    n_atoms = z.shape[0]
    zd, posd, batchd = z.to(dev), pos.float().to(dev), batch.to(dev)

    if a.mode == "train":
        gy = torch.Generator().manual_seed(100 + rank)
        y_lab = torch.randn(a.batch, 1, generator=gy).to(dev)
        f_lab = torch.randn(n_atoms, 3, generator=gy).to(dev)
        trainer = LNNPStep(model, lr=4e-4, group=None)

        def step():
            return trainer.step(zd, posd, batchd, y_lab, f_lab)
    elif a.eager:
        def step():
            y, f = model(zd, posd, batchd)
            return y, f
    else:
        from torchmdnet.graphs import GraphedEnergyForces
        gm = GraphedEnergyForces(model, zd, posd, batchd)
        # fresh coordinates every step (a pool of perturbed geometries resident in HBM): the replay
        # recomputes the neighbour list and everything downstream from the new positions
        gen = torch.Generator(device=dev).manual_seed(11 + rank)
        pool = [posd + 0.02 * torch.randn(posd.shape, device=dev, generator=gen) for _ in range(8)]
        it = [0]

        def step():
            it[0] += 1
            return gm(pool[it[0] % len(pool)])

    phase(f"main: {a.mode} {'eager' if (a.eager or a.mode == 'train') else 'hip-graph'} timing")
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    barrier(ws)
    probe = []
    kernels.EVENT_PROBE = probe
    torch.cuda.synchronize()
    barrier(ws)
    t0 = time.perf_counter()
    last = None
    for _ in range(a.steps):
        last = step()
    torch.cuda.synchronize()
    barrier(ws)
    el = time.perf_counter() - t0
    kernels.EVENT_PROBE = None
    el = max_over_ranks(el, ws, dev)
    if a.dump_outputs:  # (before anything below runs the model again: a replay's outputs are static buffers)
        dump_outputs(a.dump_outputs, {"loss": last} if a.mode == "train" else {"y": last[0], "neg_dy": last[1]}, rank)
    if a.mode == "infer" and not a.eager:
        gm.check_capacity()
        gm.release()
    if a.full and a.mode == "infer" and not a.eager:
        # graph replays run no Python: time the edge kernel live in a short eager pass instead
        probe = []
        kernels.EVENT_PROBE = probe
        for _ in range(10):
            model(zd, posd, batchd)
        torch.cuda.synchronize()
        kernels.EVENT_PROBE = None

    mols = a.batch * ws * a.steps
    out = {
        "metric": "molecules/sec (energy+force) ET-QM9" + (" training step" if a.mode == "train" else ""),
        "value": round(mols / el, 2),
        "unit": "molecules/s",
        "n_gpus": ws,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(1000 * el / a.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic (SURVEY.md 8(d) QM9-like molecules, random-init weights)",
        "config": {"workload": "ET-QM9 energy+forces (TorchMD_Net derivative=True)" if a.mode == "infer"
                   else "ET-QM9 force-matching training step (E+F MSE, double backward, RCCL all-reduce, AdamW)",
                   "model": "equivariant-transformer", "embedding_dimension": a.channels, "num_layers": 8,
                   "num_rbf": 64, "num_heads": 8, "cutoff": 5.0, "molecules_per_gpu": a.batch,
                   "atoms_per_gpu": n_atoms, "global_batch": a.batch * ws, "parallelism": f"dp{ws}",
                   "execution": "eager" if (a.eager or a.mode == "train") else "hip-graph replay"},
    }
    out["distributed"] = dist_info(ws, rank, dev)
    if rank == 0 and probe:
        H = a.channels
        ms = sum(e0.elapsed_time(e1) for e0, e1, *_ in probe) / len(probe)
        E, N = probe[0][2], probe[0][3]
        nbytes = et_algorithmic_bytes(E, N, H)
        gbs = nbytes / (ms * 1e-3) / 1e9
        out["roofline_c2"] = {"kernel": "tmdnet_et_message_fwd (k_fwd<float,4,4,1,false>)",
                              "workload": f"metric batch, N={N}, E={E} (working set fits Infinity Cache; "
                                          f"{'timed-region' if a.eager or a.mode == 'train' else 'eager pass after the graph-timed region'})",
                              "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": None,
                              "bytes_per_launch": nbytes, "ms_per_launch": round(ms, 5),
                              "launches": len(probe)}
    if a.full and a.mode == "infer" and not a.no_secondary:
        phase("secondary: TensorNet C3")
        sec = {"tensornet_c3": secondary_tensornet(a, ws, rank, dev)}
        phase("secondary: ET training step")
        sec["et_train_step"] = secondary_train(a, ws, rank, dev)
        phase("secondary: TensorNet C3 training step")
        sec["tn_train_step_c3"] = secondary_tn_train(a, ws, rank, dev)
        phase("secondary: fit() on the data path")
        sec["et_fit_data_path"] = secondary_fit(a, ws, rank, dev)
        phase("secondary: ET-SPICE C4")
        sec["et_spice_c4"] = secondary_spice(a, ws, rank, dev)
        phase("secondary: TorchScript C2")
        sec["et_scripted_c2"] = secondary_scripted(a, ws, rank, dev)
        phase("secondary: ET C5 water box")
        sec["et_water_box_c5"] = secondary_water_box(a, ws, rank, dev)
        phase("secondary: ET C5 water box, TorchScript")
        sec["et_scripted_c5"] = secondary_scripted_water_box(a, ws, rank, dev, sec["et_water_box_c5"]["ms_per_step"])
        phase("secondary: TensorNet C5 water box")
        sec["tn_water_box_c5"] = secondary_tn_water_box(a, ws, rank, dev)
        if rank == 0:
            out["secondary"] = sec
    if a.full and a.mode == "infer" and a.ddp_train:
        phase("ddp_train: ET-SPICE graphed training step")
        dt = ddp_train(a, ws, rank, dev)
        if rank == 0:
            out["ddp_train"] = dt
    if a.full and rank == 0 and not a.no_roofline:
        phase("roofline probe (C5 water box)")
        # the secondary lines leave tens of GB in the caching allocator's segments: hand them back so
        # the probe's 10+ GB of inputs are laid out as in a fresh process
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        out["roofline"] = roofline_probe(a, dev)
        tn_pmc = out["roofline"].pop("_tn_pmc", None)
        gc.collect()
        torch.cuda.empty_cache()
        phase("roofline probe: TensorNet message (C5 TensorNet graph)")
        tnr = tn_message_probe(a, dev)
        if tn_pmc:
            f = tn_pmc.get("tn_msg_fwd") or {}
            tnr["traffic"] = f.get("traffic")
            tnr["traffic_detail"] = {**f, "source": PMC_SOURCE}
            if f.get("traffic"):
                tnr["traffic_detail"]["traffic_over_bytes"] = round(f["traffic"] / tnr["bytes_per_launch"], 3)
            tnr["backward"]["pmc"] = {k: tn_pmc.get(k) for k in ("tn_msg_bwd_pair", "tn_msg_bwd_src")}
        out["roofline"]["tensornet_message"] = tnr
        phase("MFMA probe (dk/dv projection GEMM)")
        E_c5 = int(out["roofline"]["workload"].split("E=")[1].split(",")[0])
        E_c2, N_c2 = (int(probe[0][2]), int(probe[0][3])) if probe else (12548, 678)
        out["mfma"] = mfma_probe(E_c5, a.roofline_atoms, E_c2, N_c2, a.channels, 64, dev)
    if a.full and rank == 0 and ws == 1 and not a.no_cpu_baseline:
        phase("CPU baseline")
        out["cpu_baseline"] = cpu_baseline(model, args, z, pos, batch, a.cpu_seconds)
        if a.cpu_extra_seconds > 0:
            phase("CPU baseline: other configs")
            out["cpu_baseline"]["other_configs"] = cpu_baseline_extra(a, model, args, z, pos, batch)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if ws > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
