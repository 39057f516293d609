#!/usr/bin/env python
"""bench.py -- corrected Mbase/s of the per-window de Bruijn consensus path on MI355X.

One "step" = one pass of the hot path (trace expansion -> per-window consensus -> pile vote ->
fragments on the host) over one batch of synthetic piles that is already resident in HBM when the
timed region starts.  Workload at N=1 = BASELINE.json configs[1]: synthetic 10k A-reads x 10 kb x 20x
PacBio-like piles, k=14 (the other configs are parity cases: tests/test_gpu_scale.py).

Multi-GPU: ONE data set, sharded over the ranks by A-read range exactly like the reference's
`-J g,G` option (src/daccord.cpp:1156-1183, daccord_amd/shard.py); piles are independent, so there is no
data-path collective, and rank 0 gathers the corrected fragments over RCCL at the end of every step.
  --scaling weak   (default): the data set has N x --reads A-reads (fixed work per GPU)
  --scaling strong          : the data set has --reads A-reads in total
`python bench.py --gpus N` with N > 1 and no torchrun environment re-executes itself under
`python -m torch.distributed.run --nproc-per-node N` (one rank per GPU, backend nccl = RCCL).

Prints ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times --steps steps, writes the
outputs of its last step with --dump-outputs DIR and prints metric, value, unit, higher_is_better, dtype, ms_per_step and the
workload.  Everything else it measures or checks runs with --full only:
  value_end_to_end : a second timed loop of dacc_submit_piles (host plan + upload + kernels + download, --e2e-steps)
  roofline     : algorithmic bytes of the dominant kernel / its HIP-event duration vs the 8 TB/s HBM peak, the HBM
                 traffic and issue-slot counters of the same kernel from the committed PMC passes (profiles/)
  cpu_baseline : the CPU oracle (a port of the reference's algorithm, oracle/) timed on this host's cores on a
                 bounded sample of the same piles, single thread and all cores (N=1, rank 0 only)
  parity       : SHA-256 of the GPU FASTA of every committed stratum of the batch (tests/golden/scale_cfg2*.json: the first
                 1000 piles, the boundaries, middles and quarter points of the eight per-XCD queue ranges) against the digests the oracle
                 produced in the build container (default workload only), the full-batch digest, and the live CPU samples
  value_incl_plan_h2d : the same rate over the FIRST pass, which includes the host plan and the upload of piles / overlaps /
                 trace points ("piles in host RAM" to fragments); `value` is the resident-batch rate the contract asks for
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=10000, help="A-reads (= piles) per GPU (weak) or in total (strong)")
    ap.add_argument("--readlen", type=int, default=10000)
    ap.add_argument("--coverage", type=float, default=20.0)
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the end-to-end loop, roofline / PMC figures, parity digests, "
                         "live oracle samples, the accuracy report and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step returned (fragment fields, per-fragment base checksums, a seeded "
                         "sample of the bases) as DIR/<name>.npy in float64 / float32")
    ap.add_argument("--cpu-seconds", type=float, default=25.0, help="target wall time of each CPU baseline leg")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--ont", action="store_true", help="config 5 error mix (ins/del/sub = 1/3 each)")
    ap.add_argument("--e2e-steps", type=int, default=5,
                    help="steps of the second timed loop (value_end_to_end: dacc_submit_piles per step = host plan + H2D + kernels + D2H); min(--steps, this), 0 = off; with --full")
    ap.add_argument("--live-parity", type=int, default=None,
                    help="piles of rank 0's shard run through oracle/ (and half as many through oracle/_ref) after the timed loop and compared with the "
                         "GPU output (parity.live); default: 16 for every line the committed digests do not cover (N > 1, other shapes), 0 otherwise and with --no-cpu; with --full")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def respawn(args):
    """`python bench.py --gpus N` outside torchrun: start N ranks (one per GPU) and relay rank 0's JSON line."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def pmc_lookup(dom, reads, readlen, coverage, k):
    """What the committed PMC summaries (profiles/*_pmc_summary.json, scripts/gpu_pmc.sh) say about kernel `dom` on this workload and
    THIS build: roofline keys (traffic, issue fractions, diagnostics) or only a pmc_source that says why there are none.  A summary
    counts when its device sources are this build's (csrc_hash) or, failing that, for the kernels whose gfx950 instruction stream is
    identical in this build (kernel_isa); kernels that changed since are left out of the per-kernel numbers."""
    roof = {}
    try:
        import glob
        from daccord_amd import build as _build
        cur = _build.csrc_hash(); isa = None
        for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")), reverse=True):
            pm = json.load(open(fn))
            wl = pm["workload"]
            if (wl["reads"], wl["readlen"], wl["coverage"], wl["k"]) != (reads, readlen, coverage, k) or dom not in pm["kernels"]:
                continue
            same_src = pm.get("csrc_hash") == cur
            if same_src:
                valid = set(pm["kernels"])
            else:
                if isa is None:
                    isa = _build.kernel_isa_hashes()
                valid = set(kn for kn, h in pm.get("kernel_isa", {}).items() if isa.get(kn) == h)
            if dom not in valid:
                continue
            kern = {kn: v for kn, v in pm["kernels"].items() if kn in valid}
            kk = kern[dom]
            roof["traffic"] = int(kk["traffic_bytes_per_launch"])
            for key in ("valu_issue_frac", "salu_issue_frac", "lds_issue_frac", "wait_frac", "resident_waves_per_cu", "pmc_kernel_ms"):
                if key in kk:
                    roof[key] = kk[key]
            dg = kk.get("diagnostics", {})
            # the stated secondary bound (the path is not HBM bound): share of the chip's VALU issue slots the kernel uses
            # -- a wave64 VALU instruction holds a SIMD-32 for 2 cycles, 1024 SIMDs at 2.4 GHz (MI355X_MICROARCH.md) -- and, times
            # the mean share of active lanes, of its integer lane-op peak
            try:
                nv = float(kk["sq"]["SQ_INSTS_VALU"]); ms_ = float(kk["pmc_kernel_ms"])
                roof["valu_issue_util"] = round(nv * 2.0 / (ms_ * 1e-3 * 2.4e9 * 1024.0), 4)
                if "valu_lane_util" in dg:
                    roof["lane_op_frac"] = round(roof["valu_issue_util"] * float(dg["valu_lane_util"]), 4)
                roof["secondary_bound"] = "latency of dependent LDS round trips: VALU issue slots and lanes used (valu_issue_util, lane_op_frac) are what the counters say, not HBM"
            except Exception:
                pass
            for key in ("valu_lane_util", "inflight_share", "tcc_hit_rate", "tcp_tcc_read_latency_cycles", "active_scalar_frac", "lds_bank_conflict"):
                if key in dg:
                    roof[key] = dg[key]
            roof["resident_waves_per_cu_by_kernel"] = {kn: v.get("resident_waves_per_cu") for kn, v in kern.items() if v.get("resident_waves_per_cu")}
            roof["traffic_all_kernels"] = {kn: int(v["traffic_bytes_per_launch"]) for kn, v in kern.items()}
            roof["pmc_source"] = ("NOT measured in this run: constants read from profiles/%s, collected by scripts/gpu_pmc.sh (separate rocprofv3 --pmc "
                                  "passes, traffic = 2*FETCH_SIZE + WRITE_SIZE) on this workload and on %s; "
                                  "lane utilisation / in-flight shares / L2 hit rate from a %s-read slice of the same workload"
                                  % (os.path.basename(fn), ("the very device sources of this build (csrc %s)" % cur) if same_src else
                                     ("kernels whose gfx950 instruction stream is identical in this build (kernel_isa of %s; sources then csrc %s, now %s: "
                                      "kernels that changed since are left out of the per-kernel numbers)" % (", ".join(sorted(valid)), pm.get("csrc_hash"), cur)),
                                     pm.get("diagnostics_workload_reads", "?")))
            break
        else:
            roof["pmc_source"] = "none for this build (csrc %s): traffic is null until scripts/gpu_pmc.sh has run on it" % cur
    except Exception as ex:
        roof["pmc_source"] = "error while reading the PMC summaries: %r" % (ex,)
    return roof


def cgroup_quota():
    """CPUs the cgroup of this process may use (cpu.max), None = no quota."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(float(q) / float(per), 2)
    except Exception:
        return None


def usable_cpus():
    """The CPUs this process can actually get = its affinity mask capped by the cgroup's CPU quota.  On the round-6 GPU box that is 16 of
    256 logical CPUs (cpu.max = 1600000 100000): 256 threads measured 15.6 effective cores and a SLOWER like-for-like leg than 16 threads
    (0.47 vs 0.68 Mbase/s: throttled threads thrash), so the CPU legs run one thread per CPU of the quota and the line reports the host's
    CPU count, the quota and the effective cores (process CPU time / wall time) of every leg beside "cores" (VERDICT r05 task 5c)."""
    n = max(1, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    q = cgroup_quota()
    return max(1, min(n, int(q + 0.999))) if q else n


def live_parity(args, p, d, piles, ovl, frags, bases, nlive, nthr, with_reference=True, budget=45.0):
    """A bounded sample of THIS rank's own shard -- `nlive` piles from its middle -- through oracle/ on `nthr` host threads (and, on the
    rank that asks for it, half as many through oracle/_ref = the reference's own sources), compared with what this rank's GPU returned
    for the same piles.  Test infrastructure on the checking side only: nothing here is timed or shipped."""
    from daccord_amd import engine
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle as _po
        tl0 = time.perf_counter()
        lfirst = len(piles) // 2
        nlive = max(1, min(nlive, len(piles) - lfirst))
        Ol = _po.Oracle(p); Ol.set_error_profile(*d.error_profile()); Ol.load_db(d.bps, d.boff, d.rlen)
        n0 = min(nlive, nthr)
        fo_, bo_ = Ol.run(piles[lfirst:lfirst + n0], ovl, d.trace, nthreads=nthr)
        tfirst_l = time.perf_counter() - tl0
        ndone = n0
        if ndone < nlive and tfirst_l * (nlive / float(n0)) < budget:
            fo_, bo_ = Ol.run(piles[lfirst:lfirst + nlive], ovl, d.trace, nthreads=nthr); ndone = nlive
        lo_l, hi_l = int(piles[lfirst]["aread"]), int(piles[lfirst + ndone - 1]["aread"])
        gl = frags[(frags["aread"] >= lo_l) & (frags["aread"] <= hi_l)]
        live = {"oracle": {"piles": int(ndone), "first_pile_of_this_rank": int(lfirst), "areads": [lo_l, hi_l], "identical": bool(engine.fasta(gl, bases) == _po.fasta(fo_, bo_)),
                           "seconds": round(time.perf_counter() - tl0, 1), "threads": nthr}}
        if with_reference:
            try:
                import pyref as _pr
                if _pr.available(k16=(args.k > 12)) and time.perf_counter() - tl0 < budget:
                    tr0 = time.perf_counter()
                    Rl = _pr.Reference(p); Rl.set_error_profile(*d.error_profile()); Rl.load_db(d.bps, d.boff, d.rlen)
                    rthr_l = max(1, min(nthr, 16 if args.k <= 14 else 2))
                    nrl = max(1, min(ndone // 2, rthr_l))
                    fr2, br2 = Rl.run(piles[lfirst:lfirst + nrl], ovl, d.trace, nthreads=rthr_l)
                    hi_r = int(piles[lfirst + nrl - 1]["aread"])
                    gr = frags[(frags["aread"] >= lo_l) & (frags["aread"] <= hi_r)]
                    live["reference_build"] = {"piles": int(nrl), "identical": bool(engine.fasta(gr, bases) == _po.fasta(fr2, br2)),
                                               "seconds": round(time.perf_counter() - tr0, 1), "threads": rthr_l}
                else:
                    live["reference_build"] = {"skipped": "oracle/_ref not built (needs /root/reference at build time) or no time left"}
            except Exception as ex:
                live["reference_build"] = {"error": repr(ex)[:200]}
        live["identical"] = bool(live["oracle"]["identical"] and live.get("reference_build", {}).get("identical", True))
        return live
    except Exception as ex:
        return {"error": repr(ex)[:200], "identical": False}


def dump_outputs(outdir, frags, bases, budget=64 << 20):
    """What one step returned to its caller -- the fragments and the corrected bases of the whole job -- as float arrays, so that two
    builds can be compared output for output: every field of every fragment (float64; a seeded sample of the fragments where they would
    take more than half of `budget`), per fragment the checksum sum_i (i + 1) * base[i] over its bases (float64, exact), and the bases
    themselves at seeded positions of the base buffer (float32 byte values)."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    fields = ("aread", "first", "last", "len", "seq_off")
    b = np.frombuffer(bases, dtype=np.uint8) if len(bases) else np.zeros(0, np.uint8)
    rng = np.random.default_rng(20261016)
    nf_max = (budget // 2) // (8 * (len(fields) + 1))
    fi = np.arange(len(frags)) if len(frags) <= nf_max else np.sort(rng.choice(len(frags), nf_max, replace=False))
    fs = frags[fi]
    out = {"fragment_" + f: fs[f].astype(np.float64) for f in fields}
    wmax = int(fs["len"].max()) if len(fs) else 0
    w = np.arange(1, wmax + 1, dtype=np.float64)
    ck = np.zeros(len(fs), np.float64)
    for j, (o, n) in enumerate(zip(fs["seq_off"].tolist(), fs["len"].tolist())):
        ck[j] = float(np.dot(b[o:o + n].astype(np.float64), w[:n]))
    out["fragment_base_checksum"] = ck
    if len(fi) < len(frags):
        out["fragment_index"] = fi.astype(np.float64)
    left = budget - sum(a.nbytes for a in out.values())
    nb = min(len(b), left // 4, 1 << 22)
    bi = np.arange(len(b)) if nb == len(b) else np.sort(rng.integers(0, len(b), nb))
    out["bases_sample"] = b[bi].astype(np.float32)
    for name, a in out.items():
        np.save(os.path.join(outdir, name + ".npy"), a)
    return {name: int(a.size) for name, a in out.items()}


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(respawn(args))

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product has no CPU path")
    # test hook (tests/test_gpu_bench_ranks.py): DACC_BENCH_ONE_DEVICE=1 runs every rank on device 0 over gloo, so that the
    # N > 1 code path of this very script can be exercised on a box with a single GPU; never set by the driver
    one_device = os.environ.get("DACC_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    backend = "gloo" if one_device else "nccl"
    gdev = "cpu" if one_device else "cuda"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    from daccord_amd import engine, shard
    from daccord_amd._structs import default_params
    from daccord_amd.synth import SynthData

    # N > 1: one tiny all_gather + point-to-point exchange on the REAL backend before anything expensive (the data set of an 8-rank run
    # takes two minutes to generate): a rank that is missing, sits on the wrong device or cannot send fails here, naming what it saw
    preflight = shard.preflight(gdev, device_index=(local_rank if not one_device else None)) if world > 1 else None

    # one synthetic data set; rank g corrects the -J g,G part of it (A-read range rule of
    # src/daccord.cpp:1156-1183 over [0, total_reads)).  Every rank generates all READS (B reads are arbitrary; the 2-bit
    # store is replicated per GPU) but only the overlaps / piles of ITS A reads: the records are identical to those of the
    # full set (daccord_amd/synth: aread_range), so N ranks do 1/N of the setup each instead of all of it N times.
    total_reads = args.reads * world if args.scaling == "weak" else args.reads
    genome = int(total_reads * args.readlen / args.coverage)
    ncpu = os.cpu_count() or 1
    t0 = time.time()
    skw = dict(ins_frac=1 / 3.0, del_frac=1 / 3.0, sub_frac=1 / 3.0) if args.ont else {}
    arange = shard.shard_range(0, total_reads, rank, world)
    d = SynthData(genome, total_reads, args.readlen, seed=args.seed, nthreads=max(1, usable_cpus() // max(world, 1)),
                  aread_range=(arange if world > 1 else None), **skw)
    ovl, piles = engine.pile_select(d.ovl, d.piles)
    npiles_total = total_reads            # one pile per A read, pile index = A read id
    tgen = time.time() - t0

    p = default_params(k=args.k, device=local_rank)
    E = engine.Engine(p)
    E.set_error_profile(*d.error_profile())
    E.load_db(d.bps, d.boff, d.rlen)                # read store replicated on every GPU (B reads are arbitrary)
    t0 = time.time()
    frags, bases = E(piles, ovl, d.trace)          # H2D + first pass (not timed)
    tfirst = time.time() - t0
    tm0 = E.timing()

    gathered = [None, None]

    def step():
        E.rerun()
        fr, ba = E.collect()
        # the only communication of a step: corrected fragments of all ranks to rank 0 (RCCL gather; no-op at N=1)
        gathered[0], gathered[1] = shard.gather_fragments(fr, ba)      # message buffers where the backend needs them (device for RCCL, host arrays for gloo)

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wsum = tsum = vsum = t0sum = t7sum = t10sum = 0.0
    tsums = [0.0, 0.0, 0.0]
    touts = [0, 0, 0]
    for _ in range(args.steps):
        step()
        t = E.timing()
        wsum += t.window_ms; tsum += t.trace_ms; vsum += t.vote_ms; t0sum += float(getattr(t, "tier0_ms", 0.0)); t7sum += float(getattr(t, "tier7_ms", 0.0)); t10sum += float(getattr(t, "tier10_ms", 0.0))
        for i in range(3):
            tsums[i] += t.tier_ms[i]; touts[i] = int(t.tier_out[i])
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt, tfirst], dtype=torch.float64, device=gdev)
    nb = torch.tensor([float(len(bases))], dtype=torch.float64, device=gdev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(nb, op=dist.ReduceOp.SUM)
    dt = float(tmax[0].item()); tfirst_max = float(tmax[1].item())
    total_bases = float(nb.item())
    dumped = None
    if args.dump_outputs and rank == 0:
        # the last timed step's result as its caller receives it (rank 0: the gathered fragments of every rank), before anything else runs
        dumped = dump_outputs(args.dump_outputs, gathered[0], gathered[1])

    # ---- second clock (VERDICT r05 task 3): BASELINE.md section 3 defines the wall time as "piles + DB in host RAM -> last fragment on
    # host", excluding only the one-off copy of the read DB.  A step here is dacc_submit_piles on the host arrays (planner, upload of
    # piles / overlaps / trace points, every kernel, download, fragment assembly) + the gather; buffers and the hand-over buffer exist
    # (this is not the context's first batch), nothing is resident but the read store.
    e2e_steps = max(0, min(args.steps, args.e2e_steps)) if args.full else 0
    dt_e2e = 0.0
    if e2e_steps:
        def step_e2e():
            fr, ba = E(piles, ovl, d.trace)
            gathered[0], gathered[1] = shard.gather_fragments(fr, ba)
        step_e2e()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(e2e_steps):
            step_e2e()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        te = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=gdev)
        if world > 1:
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
        dt_e2e = float(te.item())
        tm_e2e = E.timing()
    t_post = time.perf_counter()      # rank 0's work behind the timed loops (digests, accuracy, CPU legs) is reported as post_loop_s

    # ---- parity.live on EVERY rank's shard (VERDICT r05 task 5b): a line the committed digests do not cover (N > 1 weak scaling: another
    # genome; other coverages / error mixes) samples piles from the middle of each rank's own shard, runs them through oracle/ on that
    # rank's share of the host cores and compares with what that rank's GPU returned; rank 0 collects the verdicts.
    default_set = (total_reads, args.readlen, args.coverage, args.k, args.seed, args.ont) == (10000, 10000, 20.0, 14, 3, False)
    nlive = args.live_parity
    if nlive is None:
        nlive = 0 if (args.no_cpu or default_set) else (16 if world == 1 else max(2, (64 + world - 1) // world))
    if not args.full:
        nlive = 0
    live_rank = None
    if nlive > 0:
        live_rank = live_parity(args, p, d, piles, ovl, frags, bases, nlive, max(1, usable_cpus() // max(world, 1)), with_reference=(rank == 0))
    live_all = None
    if world > 1 and nlive > 0:
        v = torch.tensor([1.0 if (live_rank and live_rank.get("identical")) else 0.0, float((live_rank or {}).get("oracle", {}).get("piles", 0)), 1.0], dtype=torch.float64, device=gdev)
        vmin = v.clone(); dist.all_reduce(vmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(v, op=dist.ReduceOp.SUM)
        live_all = {"ranks_reporting": int(v[2].item()), "ranks_identical": int(v[0].item()), "piles_total": int(v[1].item()), "identical_on_every_rank": bool(vmin[0].item() == 1.0)}

    if rank == 0:
        t = E.timing()
        allfr, allba = (gathered[0], gathered[1]) if gathered[0] is not None else (frags, bases)
        assert float(len(allba)) == total_bases, "gathered bases do not add up"
        ms_per_step = 1e3 * dt / args.steps
        value = total_bases * args.steps / dt / 1e6
    if rank == 0 and args.full:
        # slots of the window kernels: shallow batches run k_classify + k_window_fast<0> (size classes) and k_window_fast<1> in
        # the first slot and k_window_fast<6> in the second; batches of deep piles k_window_fast<4> and k_window_fast<2>
        deep = int(getattr(t, "first_tier", 1)) == 4
        first_kernel = "k_window_fast<4>" if deep else "k_window_fast<1>"
        second_kernel = "k_window_fast<2>" if deep else "k_window_fast<6>"
        kern = {"k_trace": tsum / args.steps, "k_vote": vsum / args.steps,
                first_kernel: (tsums[0] - t0sum - t7sum) / args.steps, second_kernel: tsums[1] / args.steps,
                "k_window_fast<3>": (tsums[2] - t10sum) / args.steps, "k_window": (wsum - sum(tsums)) / args.steps}
        t10ran = int(getattr(t, "tier10_ran", 0)) == 1; t10out = int(getattr(t, "tier10_out", 0))
        dense_kernel = "k_window_fast<11>" if deep else "k_window_fast<10>"      # the dense tier of deep / shallow batches
        if t10ran:
            kern[dense_kernel] = t10sum / args.steps      # round 6: the dense-graph tier (2 wavefronts per CU) between the second slot's tier and tier 3
        if t0sum > 0:
            kern["k_classify+k_window_fast<0>"] = t0sum / args.steps
        if t7sum > 0:
            kern["k_window_fast<7>"] = t7sum / args.steps      # round 6: the middle size class (7 wavefronts per CU) between tier 0 and tier 1
        dom = max(kern, key=kern.get)
        # algorithmic bytes (every input byte once + corrected bases = 61 B per window at config 2) of the windows the
        # dominant kernel ITSELF ran in a launch / its duration.  (Rounds 1-4 divided the whole batch's bytes by the one kernel's time,
        # 1.6 x too kind since the size classes: VERDICT r04 weak 3.)  The window kernels' shares of the batch:
        # (the second stream's windows run in k_window_long: n1 = the pre-scan's list, which no tier sees, n2 = the windows the first
        # tier found no LDS tier can run -- the first tier did process those)
        nwin = int(t.nwindows); t0in = int(getattr(t, "tier0_in", 0)); t0out = int(getattr(t, "tier0_out", 0)); nlong = int(getattr(t, "long_windows", 0))
        n2 = int(getattr(t, "long_first_tier", 0)); n1 = max(0, nlong - n2)
        t7in = int(getattr(t, "tier7_in", 0)); t7out = int(getattr(t, "tier7_out", 0))
        # tier 7 ran the pre-pass's middle class + tier 0's hand-overs; tier 1 the pre-pass's big class + tier 7's hand-overs (without tier 7: + tier 0's)
        first_in = (nwin - t0in - n1 - (t7in - t0out) + t7out) if t7in else (nwin - t0in - n1 + t0out)
        wins = {"k_trace": nwin, "k_vote": nwin, first_kernel: max(0, first_in), second_kernel: touts[0],
                "k_window_fast<3>": (t10out if t10ran else touts[1]), dense_kernel: (touts[1] if t10ran else 0), "k_window": touts[2], "k_window_long": nlong, "k_classify+k_window_fast<0>": t0in, "k_window_fast<7>": t7in}
        bpw = t.algo_bytes / max(1, nwin)
        dom_bytes = bpw * wins.get(dom, nwin)
        achieved = dom_bytes / (kern[dom] * 1e-3) / 1e9 if kern[dom] > 0 else 0.0
        achieved_step = t.algo_bytes / max(dt / args.steps, 1e-12) / 1e9
        roof = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 4), "peak": 8000.0, "unit": "GB/s",
                "frac": round(achieved / 8000.0, 8), "traffic": None,
                "windows_per_launch": int(wins.get(dom, nwin)), "algo_bytes_per_window": round(bpw, 2),
                "algo_bytes_per_launch": int(dom_bytes), "algo_bytes_batch": int(t.algo_bytes),
                "achieved_step": round(achieved_step, 4), "frac_step": round(achieved_step / 8000.0, 8),
                "windows_by_kernel": {k: int(v) for k, v in wins.items() if k in kern or k == "k_window_long"},
                "kernel_ms": {k: round(v, 3) for k, v in kern.items()},
                "window_ms_all_tiers": round(wsum / args.steps, 3),
                "windows_handed_on": dict({first_kernel: touts[0], second_kernel: touts[1], "k_window_fast<3>_to_generic": touts[2]}, **({dense_kernel: t10out} if t10ran else {})),
                "size_classes": {"windows_sent_to_tier0": int(getattr(t, "tier0_in", 0)), "handed_on_by_tier0": int(getattr(t, "tier0_out", 0)),
                                 "windows_run_by_tier7": t7in, "handed_on_by_tier7": t7out},
                "windows_on_second_stream": int(getattr(t, "long_windows", 0))}
        # HBM traffic and issue counters of the dominant kernel from the PMC passes (rocprofv3 --pmc, separate runs,
        # scripts/gpu_pmc.sh -> profiles/<round>_pmc_summary.json): quoted only when they were collected on this very
        # workload AND on the very kernels this build runs -- never stale counters.  "The very kernels": the device sources are the
        # same (csrc_hash), or the machine code of the kernel is (kernel_isa: instruction-stream hash per kernel, build.kernel_isa_hashes;
        # a change to the generic engine leaves the code of the LDS tiers as it was).  Per-kernel numbers are quoted for unchanged kernels only.
        # (the size classes' entry is two kernels; its counters are those of k_window_fast<0>, the pre-pass is 1 ms of it)
        roof.update(pmc_lookup("k_window_fast<0>" if dom == "k_classify+k_window_fast<0>" else dom, args.reads, args.readlen, args.coverage, args.k))
    if rank == 0:
        res = {
            "metric": "corrected Mbase/s (whole node), synthetic 20x PacBio piles",
            "value": round(value, 3), "unit": "Mbase/s", "n_gpus": world, "ranks": (dist.get_world_size() if world > 1 else 1), "backend": (backend if world > 1 else None),
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "value_incl_plan_h2d": round(total_bases / max(tfirst_max, 1e-9) / 1e6, 3),
            "preflight": preflight,
            "gather": (shard.last_transport if world > 1 else None),
            "dtype": "u64+f64", "data": "synthetic",
            "config": {"workload": "%ssynthetic %d A-reads x %d b x %.0fx%s, 15%% error (%s), k=%d, w=40, a=10, tspace=100"
                       % (("BASELINE.json configs[1] (10k A-reads x 10 kb x 20x, k=14, one MI355X%s): " % (" per rank, weak scaling" if world > 1 else ""))
                          if (args.reads, args.readlen, args.coverage, args.k, args.ont) == (10000, 10000, 20.0, 14, False) and (world == 1 or args.scaling == "weak") else "",
                          total_reads, args.readlen, args.coverage, " (%d per GPU)" % args.reads if args.scaling == "weak" and world > 1 else "",
                          "ins/del/sub 1/3 each" if args.ont else "ins 80/del 13.3/sub 6.7", args.k),
                       "piles_total": int(npiles_total), "piles_rank0": int(len(piles)), "overlaps_rank0": int(len(ovl)), "windows_rank0": int(t.nwindows),
                       "trace_blocks_rank0": int(t.nblocks), "corrected_bases_total": int(total_bases),
                       "k_range": "3..16; k = 17 is rejected by dacc_create (DACC_EINVAL): no reference semantics -- the reference's k-mer instance word is kmer << 32 | pos << 16 | seq "
                                  "(src/DebruijnGraph.hpp:956-961, 1209-1235), a 34 bit k-mer does not fit it",
                       "sharding": "one data set, A-read ranges as -J g,G (daccord.cpp:1156-1183), no data-path collective; RCCL gather of corrected fragments per step"},
            "setup_s": {"generate": round(tgen, 2), "first_pass_incl_plan_h2d": round(tfirst_max, 2), "h2d_ms": round(tm0.h2d_ms, 2)},
        }
        if dumped is not None:
            res["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if rank == 0 and args.full:
        res.update({
            "value_end_to_end": (round(total_bases * e2e_steps / dt_e2e / 1e6, 3) if e2e_steps and dt_e2e > 0 else None),
            "value_definition": "value = resident rate the driver's contract asks for (piles, overlaps, trace points and the plan already in HBM when the timed region starts; "
                                "every kernel, the download and the host fragment assembly run in every step); value_end_to_end = BASELINE.md section 3's clock "
                                "(piles + DB in host RAM -> last fragment on host, excluding only the one-off copy of the read DB): %d step(s) of dacc_submit_piles = host plan + upload of "
                                "piles / overlaps / trace points + the same kernels + download, timed the same way" % e2e_steps,
            "end_to_end": ({"steps": e2e_steps, "ms_per_step": round(1e3 * dt_e2e / e2e_steps, 3), "h2d_ms": round(tm_e2e.h2d_ms, 2), "window_ms": round(tm_e2e.window_ms, 2)} if e2e_steps else None),
            "roofline": roof})
        # ---- parity: full-batch digest, the oracle's committed digest of the first 1000 piles, live oracle sample ----
        def fasta_sha256(fr, ba):
            # digest of the FASTA text record by record (the text of 8 x 10 000 reads would be 0.7 GB in one string)
            h = hashlib.sha256(); well = 0
            for i in range(0, len(fr), 256):
                h.update(engine.fasta(fr[i:i + 256], ba, start_well=well).encode()); well += len(fr[i:i + 256])
            return h.hexdigest()
        par = {"gpu_fasta_sha256_all": fasta_sha256(allfr, allba), "piles_all": int(npiles_total)}
        # The oracle's committed digests (build container, tests/golden/make_golden_scale.py): piles STRATIFIED over the whole
        # batch -- the first 62, 125 around each of the seven interior boundaries of the eight per-XCD window queues, the last
        # 125 (scale_cfg2s.json) -- and, if present, the first 1000 piles (scale_cfg2.json); default workload only.  Other
        # workloads of the same generator: --coverage 54 / --ont against their own fixtures when the shapes match.
        def compare_golden(name):
            gold = os.path.join(ROOT, "tests", "golden", "scale_%s.json" % name)
            if not os.path.exists(gold):
                return None
            GG = json.load(open(gold)); G = GG["runs"][0]; spec = GG["spec"]
            if G.get("params") != {"k": args.k}:      # a fixture of the same data set under other run parameters (window size ...) is not this run's oracle
                return None
            ranges = spec.get("pile_ranges") or [[spec["first"], spec["first"] + spec["npiles"]]]
            idx = np.concatenate([np.arange(a, b) for a, b in ranges])
            areads = idx                 # pile index = A read id in the synthetic sets
            sel = allfr[np.isin(allfr["aread"], areads)]
            h = fasta_sha256(sel, allba)
            out = {"fixture": "tests/golden/scale_%s.json" % name, "piles_compared": int(len(idx)), "pile_ranges": ranges,
                   "gpu_fasta_sha256": h, "oracle_fasta_sha256": G["fasta_sha256"], "identical": h == G["fasta_sha256"]}
            if not out["identical"] and "pile_sha256" in G:
                bad = []
                for j, a in enumerate(areads):
                    f = allfr[allfr["aread"] == a]
                    if hashlib.sha256(engine.fasta(f, allba).encode()).hexdigest()[:12] != G["pile_sha256"][j]:
                        bad.append(int(idx[j]))
                out["piles_that_differ"] = bad[:50]
            return out
        if default_set:
            # every committed stratum of this batch: cfg2s (boundaries of the queue ranges), cfg2t (their middles), cfg2u (their first
            # quarters), cfg2v (three-quarter points), cfg2 (the first 1000 piles)
            import glob
            names = sorted(os.path.basename(f)[len("scale_"):-len(".json")] for f in glob.glob(os.path.join(ROOT, "tests", "golden", "scale_cfg2*.json")))
            cmp_ = [c for c in (compare_golden(n) for n in sorted(names, key=lambda n: (n == "cfg2", n))) if c]
            if cmp_:
                distinct = set()
                for c in cmp_:
                    for a, b in c["pile_ranges"]:
                        distinct.update(range(a, b))
                par.update({"piles_compared": int(sum(c["piles_compared"] for c in cmp_)), "piles_compared_distinct": len(distinct),       # the strata of the first range overlap the first 1000 piles
                            "identical": all(c["identical"] for c in cmp_), "fixtures": cmp_,
                            "oracle_source": "oracle run in the build container (tests/golden/make_golden_scale.py): the first 1000 piles and stratified samples of all eight queue ranges of the batch (boundaries, middles, quarter points); "
                                             "the oracle itself is pinned to the reference's own sources (oracle/_ref, tests/test_oracle_vs_ref.py)"})
        # ---- parity.live: see live_parity() -- rank 0's own sample in full, the other ranks' verdicts collected above
        if live_rank is not None:
            par["live"] = live_rank
            if live_all is not None:
                par["live"]["all_ranks"] = live_all
                par["live"]["identical"] = bool(par["live"].get("identical") and live_all["identical_on_every_rank"])
        res["parity"] = par
        # ---- accuracy against the known truth of the synthetic reads (checkconsensus measurement, README.md:406-472):
        # the only quality figure that does not depend on the oracle ----
        try:
            from daccord_amd import checkconsensus
            nacc = min(npiles_total, 200)
            lim = nacc - 1
            _, acc = checkconsensus.check(allfr[allfr["aread"] <= lim], allba, d.genome, d.truth, d.rlen)
            acc["sample"] = "first %d reads, every fragment aligned to the true sequence of its read interval" % nacc
            acc["raw_read_erate"] = 0.15
            res["accuracy"] = acc
        except Exception as ex:      # the accuracy report must never cost the throughput line
            res["accuracy"] = {"error": str(ex)}
        if world == 1 and not args.no_cpu:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import pyoracle
            pyref_fasta = pyoracle.fasta
            O = pyoracle.Oracle(p)
            O.set_error_profile(*d.error_profile())
            O.load_db(d.bps, d.boff, d.rlen)
            # bounded samples of the same batch (a pile of this workload costs the oracle about 5-10 s on one thread):
            # (a) one thread, (b) all CPUs this process may use (cgroup quota / affinity; the logical CPU count of the
            # host is reported beside it), schedule(dynamic,1) over A-reads like src/daccord.cpp:2109.  (b) runs in two
            # stages so that a host that delivers fewer cores than it shows cannot blow the time budget.  The piles of
            # (b) lie behind the first 1000, which the committed digest covers.
            def mem_available_gib():
                try:
                    for ln in open("/proc/meminfo"):
                        if ln.startswith("MemAvailable:"):
                            return float(ln.split()[1]) / (1 << 20)
                except Exception:
                    pass
                return 64.0
            tc = time.perf_counter()
            f1, b1 = O.run(piles[:1], ovl, d.trace, nthreads=1)
            t1 = time.perf_counter() - tc
            n1 = 1
            if t1 < args.cpu_seconds / 2:
                n1 = max(1, min(len(piles), int(args.cpu_seconds / max(t1, 1e-3))))
                tc = time.perf_counter()
                f1, b1 = O.run(piles[:n1], ovl, d.trace, nthreads=1)
                t1 = time.perf_counter() - tc
            per_pile = t1 / n1
            nthr = usable_cpus()
            quota = cgroup_quota()
            cap_cores = max(1.0, min(float(nthr), quota) if quota else float(nthr))      # for SIZING the samples only: what the host is likely to deliver
            first = min(1000, max(0, len(piles) - 1))
            # stage 1: a probe of at most 32 piles on all threads (bounded even if the host delivers far fewer cores than it shows);
            # stage 2: as many piles as the delivered cores finish in the leg's time budget, at least one per core that can run
            nall = min(len(piles) - first, nthr, 32)
            tc = time.perf_counter(); pc = time.process_time()
            fa, ba = O.run(piles[first:first + nall], ovl, d.trace, nthreads=nthr)
            ta = time.perf_counter() - tc; pa = time.process_time() - pc
            cpu_s_per_pile = pa / max(1, nall)
            more = min(len(piles) - first, int(cap_cores * args.cpu_seconds / max(cpu_s_per_pile, 1e-3)))
            if more > nall and ta < args.cpu_seconds:
                nall = more
                tc = time.perf_counter(); pc = time.process_time()
                fa, ba = O.run(piles[first:first + nall], ovl, d.trace, nthreads=nthr)
                ta = time.perf_counter() - tc; pa = time.process_time() - pc
                cpu_s_per_pile = pa / max(1, nall)
            lo, hi = int(piles[first]["aread"]), int(piles[first + nall - 1]["aread"])
            gsel = frags[(frags["aread"] >= lo) & (frags["aread"] <= hi)]
            same_all = engine.fasta(gsel, bases) == pyoracle.fasta(fa, ba)
            g1 = frags[frags["aread"] <= int(piles[n1 - 1]["aread"])]
            same_1 = engine.fasta(g1, bases) == pyoracle.fasta(f1, b1)
            res["cpu_baseline"] = {
                "value": round(len(ba) / ta / 1e6, 5), "unit": "Mbase/s", "cores": nthr, "kind": "port", "host_logical_cpus": ncpu,
                "effective_cores": round(pa / max(ta, 1e-9), 1), "cgroup_cpu_quota": cgroup_quota(),
                "parallel_speedup_over_single_thread": round((len(ba) / ta) / max(len(b1) / t1, 1e-12), 2),
                "sample": "piles %d..%d of the same batch (%d piles, %d windows each), oracle with %d OpenMP threads schedule(dynamic,1), %.1f s"
                          % (first, first + nall - 1, nall, int(t.nwindows // max(1, len(piles))), nthr, ta),
                "single_thread": {"value": round(len(b1) / t1 / 1e6, 6), "cores": 1, "sample": "first %d pile(s), %.1f s" % (n1, t1)},
                "identical_to_gpu_on_sample": bool(same_all and same_1), "piles_compared_live": int(nall + n1),
                "note": "the oracle follows the reference and recomputes stretches, feasibility and both path enumerations for every "
                        "(first,last) k-mer pair; the GPU path caches them per k-mer, so the ratio is not like for like",
            }
            # like for like: the SAME algorithm as the kernels (cached enumerations, tiers, reachability prune) compiled for the
            # host -- the 1-lane build of the kernel headers that the CPU tests use (tests/emul) -- one context per thread on
            # all usable cores over a bounded sample of the same batch.  GPU / this = what the chip buys for this algorithm.
            try:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import emul_lib
                from concurrent.futures import ThreadPoolExecutor
                lthr = max(1, min(nthr, int(mem_available_gib() / 1.0)))      # an emulation context: its own arenas and images, < 1 GiB
                nl = min(len(piles) - first, max(lthr, lthr * 6))
                chunks = [piles[first + i:first + nl:lthr] for i in range(lthr)]
                def work(ch):
                    if len(ch) == 0:
                        return 0, b""
                    Em = emul_lib.Emul(p); Em.set_error_profile(*d.error_profile()); Em.load_db(d.bps, d.boff, d.rlen)
                    fe, be = Em.run(ch, ovl, d.trace)
                    return len(be), hashlib.sha256(engine.fasta(fe, be).encode()).digest()
                emul_lib.lib(1)
                tc = time.perf_counter()
                pc = time.process_time()
                with ThreadPoolExecutor(lthr) as ex:
                    outs = list(ex.map(work, chunks))
                tl = time.perf_counter() - tc; pl = time.process_time() - pc
                same = True
                for ch, (nbs, dg) in zip(chunks, outs):
                    if len(ch):
                        g = frags[np.isin(frags["aread"], ch["aread"])]
                        same = same and hashlib.sha256(engine.fasta(g, bases).encode()).digest() == dg
                lb = sum(o[0] for o in outs)
                res["cpu_baseline"]["like_for_like"] = {
                    "value": round(lb / tl / 1e6, 5), "unit": "Mbase/s", "cores": lthr, "kind": "port", "effective_cores": round(pl / max(tl, 1e-9), 1),
                    "what": "the kernels' own algorithm (tests/emul: kernel headers compiled as a 1-lane wavefront, g++ -O2), one context per thread",
                    "sample": "%d piles of the same batch behind pile %d, %.1f s" % (nl, first, tl),
                    "identical_to_gpu_on_sample": bool(same), "gpu_over_this": round(value / max(lb / tl / 1e6, 1e-12), 1)}
            except Exception as ex:
                res["cpu_baseline"]["like_for_like"] = {"error": repr(ex)[:200]}
            # the reference's OWN sources (oracle/_ref: /root/reference/src headers compiled in the build container against the
            # libmaus2 stand-in, oracle/ref_shim/; the built library travels, the sources do not) on the same host cores, bounded
            # sample: the CPU figure closest to "reference daccord on this box" that exists without libmaus2.  Its primitives
            # (aligner, heaps, rank / RMQ structures) are plain stand-ins, slower than libmaus2's SIMD code, so the ratio flatters
            # the GPU even more than the oracle's does; what it adds is that the GPU output equals the REFERENCE SOURCE's here.
            try:
                import pyref
                if pyref.available(k16=(args.k > 12)):
                    R = pyref.Reference(p)
                    R.set_error_profile(*d.error_profile()); R.load_db(d.bps, d.boff, d.rlen)
                    # a DebruijnGraph<k> of the reference holds a node cache of 4^k int32 per thread (1 GiB at k = 14, 16 GiB at k = 16): as many
                    # threads as half of the available host memory holds, at most every usable core
                    per_thr_gib = max(0.25, 4.0 * (4.0 ** args.k) / (1 << 30) * 1.25)
                    rthr = max(1, min(nthr, int(0.5 * mem_available_gib() / per_thr_gib)))
                    # sample sized to the leg's time budget on the cores the host delivers (the port leg measured the CPU seconds of a pile;
                    # the reference build needs about 1.6 x that), at least one pile per thread that fits
                    nrp = max(1, min(len(piles) - first, 2 * rthr, max(rthr if rthr <= cap_cores else int(cap_cores), int(cap_cores * args.cpu_seconds / max(1.6 * cpu_s_per_pile, 1e-3)))))
                    tc = time.perf_counter(); pc = time.process_time()
                    fr_, br_ = R.run(piles[first:first + nrp], ovl, d.trace, nthreads=rthr)
                    tr_ = time.perf_counter() - tc; pr_ = time.process_time() - pc
                    lo_, hi_ = int(piles[first]["aread"]), int(piles[first + nrp - 1]["aread"])
                    gs_ = frags[(frags["aread"] >= lo_) & (frags["aread"] <= hi_)]
                    res["cpu_baseline"]["reference_build"] = {
                        "value": round(len(br_) / tr_ / 1e6, 5), "unit": "Mbase/s", "cores": rthr, "kind": "reference",
                        "effective_cores": round(pr_ / max(tr_, 1e-9), 1), "host_logical_cpus": ncpu, "cgroup_cpu_quota": cgroup_quota(),
                        "what": "src/HandleContext.hpp + DebruijnGraph.hpp + OffsetLikely.hpp ... of the reference, unmodified, on the libmaus2 stand-in (oracle/_ref%s)"
                                % (", k <= 16 factory" if args.k > 12 else ""),
                        "sample": "piles %d..%d of the same batch, %.1f s" % (first, first + nrp - 1, tr_),
                        "identical_to_gpu_on_sample": bool(engine.fasta(gs_, bases) == pyref_fasta(fr_, br_))}
                else:
                    res["cpu_baseline"]["reference_build"] = {"error": "oracle/_ref not built (needs /root/reference at build time)"}
            except Exception as ex:
                res["cpu_baseline"]["reference_build"] = {"error": repr(ex)[:200]}
            # top level = the figure north_star names: the reference's own code on this host's cores (kind "reference"); the oracle
            # port, its single thread and the like-for-like leg are nested.  Without oracle/_ref the port stays on top and says so.
            cb = res["cpu_baseline"]; rb = cb.get("reference_build") or {}
            if "value" in rb:
                port = {k_: v_ for k_, v_ in cb.items() if k_ not in ("like_for_like", "reference_build")}
                res["cpu_baseline"] = {"value": rb["value"], "unit": rb["unit"], "cores": rb["cores"], "kind": "reference", "sample": rb["sample"],
                                       "effective_cores": rb.get("effective_cores"), "host_logical_cpus": ncpu, "cgroup_cpu_quota": rb.get("cgroup_cpu_quota"),
                                       "what": rb["what"], "identical_to_gpu_on_sample": rb["identical_to_gpu_on_sample"],
                                       "gpu_over_this": round(value / max(rb["value"], 1e-12), 1),
                                       "port": port, "like_for_like": cb.get("like_for_like")}
            else:
                cb["note_kind"] = "oracle/_ref is not available here: the top-level entry is the oracle port"
    if rank == 0:
        res["post_loop_s"] = round(time.perf_counter() - t_post, 2)
        print(json.dumps(res), flush=True)      # out before any teardown (stdout is block-buffered when it is a file)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
