#!/usr/bin/env python3
"""bench.py — headline benchmark of the FASTQ record-scan path on MI355X.

One "step" = one pass of the hot path (fqh_scan: byte-scan kernel -> tile prefix -> emit/validate ->
summary) over one HBM-resident batch of synthetic 150 bp FASTQ.  N = 1: BASELINE.json configs[1],
16 GiB (17 179 868 970 B = 52 060 209 records).  N > 1: the input is one file of N x 16 GiB cut by
byte range at multiples of 2^34 (cuts fall inside records); every rank scans its own shard, the
ranks exchange 7 words of carry, re-run only the emit step with the true carry, and all-reduce the
counts (and histograms) over RCCL.  value = total bytes of all ranks / max-over-ranks time.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the line
(roofline: k_index, the dominant kernel, measured with HIP events on the launch stream inside the
timed region).  --full adds everything else the benchmark measures or checks, in runs of their own:
other input allocations (best_allocation), roofline traffic from rocprofv3 counters, the read
ceiling, stats (the histogram pass on the same buffer, configs[2]), kilobase reads, the streamed
leg (configs[3]), cpu_baseline (the oracle timed on the host cores, rank 0, N = 1 only), host_api,
the one-rank RCCL protocol check and the sharded host-streamed leg (configs[4]).
--dump-outputs DIR writes what the last timed step computed (record offsets, summary, carry) as .npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

RECLEN = 330
SHARD = 1 << 34

# The contract: rank 0 prints ONE JSON line on stdout.  Libraries under this process write to file descriptor 1 as well (RCCL
# prints a version banner when a communicator is created — the library's own binding makes one even at N = 1 — and C stdio
# flushes it at exit, BEHIND the line).  So the line goes to a private copy of the original stdout and descriptor 1 itself is
# pointed at stderr for everything else.
_LINE_OUT = None


def own_stdout():
    global _LINE_OUT
    if _LINE_OUT is None:
        sys.stdout.flush()
        _LINE_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit_line(obj):
    own_stdout()
    _LINE_OUT.write(json.dumps(obj) + "\n")
    _LINE_OUT.flush()
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bytes", type=int, default=0, help="per-GPU bytes (default 16 GiB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stats", action="store_true")
    ap.add_argument("--cpu-sample-mib", type=int, default=4096)
    ap.add_argument("--shard-stats", action="store_true",
                    help="N > 1 only, after the timed steps: per-position histograms over the shards (every rank "
                         "gets the tail of the previous rank's shard in front of its own, one all_reduce of the "
                         "histograms) and a check of the global totals; one extra JSON line, not part of the metric")
    ap.add_argument("--stream-gib", type=float, default=0.0,
                    help="configs[3] (N = 1) / configs[4] (N > 1): stream this many GiB (in total) from pinned host memory "
                         "through fqh_stream_* (a pinned block is replayed) and report the PCIe-inclusive rate; N > 1: "
                         "byte-range shards, every rank phase-free through its own ring, one exchange + stitch + all_reduce")
    ap.add_argument("--slot-mib", type=int, default=256, help="ring slot size of the streamed modes")
    ap.add_argument("--producer-threads", type=int, default=0,
                    help="threads that fill a ring slot from pageable host memory (0: 1, the reference's one reader thread, AND 8)")
    ap.add_argument("--no-stream", action="store_true", help="skip the configs[3] leg of a --full run")
    ap.add_argument("--no-long-reads", action="store_true", help="skip the kilobase-read histogram leg of a --full run")
    ap.add_argument("--default-stream-gib", type=float, default=256.0,
                    help="size of the configs[3] leg of a --full run (its stated size: 256 GiB, ~5 s at the link's rate; the "
                         "one-thread producer run stops at 8 GiB)")
    ap.add_argument("--numa-pin", choices=["auto", "require", "off"], default="auto",
                    help="streamed legs: run on (and first-touch the pinned ring from) the NUMA node of the GPU.  auto: best effort, "
                         "the JSON line says what happened; require: fail if it did not happen")
    ap.add_argument("--pmc-traffic", choices=["auto", "off"], default="auto",
                    help="roofline.traffic from this run's own rocprofv3 --pmc passes (two short child runs, FETCH_SIZE and WRITE_SIZE "
                         "apart, calibrated on the plain read kernel) when rocprofv3 is on the box; otherwise from the committed profile")
    ap.add_argument("--comm", choices=["auto", "abi", "torch"], default="auto",
                    help="who runs the collectives of the sharded modes: abi = the library's own RCCL binding (fqh_comm_* / fqh_allgather / "
                         "fqh_allreduce_u64 / fqh_allreduce_min_u64, csrc/comm.hip: what a Rust or C++ host without torch uses), torch = "
                         "torch.distributed.  auto: abi when the backend is nccl (or there is one rank), torch under gloo (the one-GPU "
                         "functional mode: RCCL does not put two ranks on one device)")
    ap.add_argument("--default-shard-stream-gib", type=float, default=128.0,
                    help="GiB PER RANK of the configs[4] leg every --full run carries (key `sharded_stream`); 128 gives 1 TiB at 8 ranks")
    ap.add_argument("--no-shard-stream", action="store_true", help="skip the configs[4] leg of a --full run")
    ap.add_argument("--no-host-api", action="store_true", help="skip the timing of the drop-in host API (host/bin/fastq_count) on the configs[0] file")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other measurement and check (input allocation candidates, "
                         "rocprofv3 traffic, read ceiling, histograms, long reads, streamed legs, CPU baseline, host API, RCCL "
                         "protocol check, configs[4]); a plain run measures the headline figure only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (record offsets: all, or a fixed seeded sample of at most 2^21; "
                         "the summary; the carry) as DIR/<name>.npy in float64; bench_outputs/ is git-ignored")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` with no launcher around it: be the launcher (one rank per GPU, the contract's command line)
        sys.exit(self_launch(args.gpus))

    own_stdout()   # (before anything below can write to descriptor 1)
    import numpy as np
    import torch
    import torch.distributed as dist

    import __graft_entry__ as g
    pkg = g.load_package()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = args.gpus
    if world != n_gpus:  # a line that says n_gpus != --gpus would be a wrong record without any error (checked before any rendezvous)
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (plain `python bench.py --gpus N` "
                         "does it by itself)" % (n_gpus, world))
    # FQH_BENCH_BACKEND=gloo + FQH_BENCH_ONE_GPU=1: run the N > 1 protocol with every rank on cuda:0
    # (functional check of the sharded path on a 1-GPU box; the driver's runs use RCCL, one GPU per rank)
    backend = os.environ.get("FQH_BENCH_BACKEND", "nccl")
    one_gpu = os.environ.get("FQH_BENCH_ONE_GPU", "0") == "1"
    dev_index = 0 if (world == 1 or one_gpu) else local_rank
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    # who takes part: world size as the process group sees it, the backend, and the UUID of every rank's device
    my_uuid = str(getattr(torch.cuda.get_device_properties(dev_index), "uuid", "cuda:%d" % dev_index))
    if world > 1:
        uuids = [None] * world
        dist.all_gather_object(uuids, my_uuid)
        rccl = {"ranks": dist.get_world_size(), "backend": dist.get_backend(), "device_uuids": uuids,
                "distinct_devices": len(set(uuids))}
    else:
        rccl = {"ranks": 1, "backend": None, "device_uuids": [my_uuid], "distinct_devices": 1}

    # one real stream for the library's kernels and for the collectives (the device-side exchange is ordered by the
    # stream alone; torch's default stream is the null stream, which the library would replace by a stream of its own)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    via = args.comm if args.comm != "auto" else ("abi" if (backend == "nccl" or world == 1) else "torch")
    if via == "abi" and world > 1 and backend != "nccl":
        raise SystemExit("bench.py: --comm abi needs one GPU per rank (RCCL does not put two ranks on one device); the gloo mode keeps --comm torch")

    if args.stream_gib > 0 and world > 1:
        sctx = pkg.Ctx(dev.index, stream=torch.cuda.current_stream().cuda_stream)
        coll = Coll(pkg, torch, dist, sctx, dev, world, rank, backend, via)
        rccl["via"] = coll.via_text
        j = sharded_stream(args, pkg, torch, dev, sctx, coll, args.stream_gib / world, int(os.environ.get("FQH_BENCH_INJECT", "-1")))
        if rank == 0:
            emit_line(dict(j, mode="sharded-stream", n_gpus=world, backend=backend, rccl=rccl))
        coll.close()
        sctx.close()
        dist.destroy_process_group()
        return
    if args.stream_gib > 0 and not args.bytes:
        args.bytes = (args.slot_mib << 20) + (1 << 20)  # (the streamed mode only needs one slot's worth of synthetic bytes)

    shard = args.bytes if args.bytes else SHARD
    total_records = (world * shard) // RECLEN
    file_len = total_records * RECLEN
    lo = rank * shard
    hi = min((rank + 1) * shard, file_len)
    nbytes = hi - lo

    ctx = pkg.Ctx(dev.index, stream=torch.cuda.current_stream().cuda_stream)
    # (one rank: the timed steps use no collective, but the communicator is made in every run all the same — its device memory
    # is allocated before the input's, and where the input lands decides the byte scan's speed: DESIGN.md 4b)
    coll = Coll(pkg, torch, dist, ctx, dev, world, rank, backend, via)
    rccl["via"] = coll.via_text
    if os.environ.get("FQH_BENCH_PLACE_TRIES"):
        ctx.set_place_tries(int(os.environ["FQH_BENCH_PLACE_TRIES"]))
    # the harness blocks on every step anyway: it opts in to polling the stream at the end of a step (FQH_OPT_SPIN_WAIT; the
    # library's default is to sleep, which wakes up ~15 us late); FQH_BENCH_SPIN_US=0 measures the default
    spin_us = int(os.environ.get("FQH_BENCH_SPIN_US", "20000"))
    ctx.set_spin_wait(spin_us)
    if os.environ.get("FQH_BENCH_ADAPT_LINES"):   # (A/B of the library default, 3; 0 = one line buffer, whatever kind it is for this input)
        ctx.set_adapt_lines(int(os.environ["FQH_BENCH_ADAPT_LINES"]))
    LEAD = 2 * pkg.BUFSIZE  # room in front of the shard for the tail of the previous rank's shard (--shard-stats)
    # Where the driver puts a 16 GiB allocation decides whether the byte scan runs at 2.62-2.66 or at 2.77-2.87 ms on it (DESIGN.md
    # 4b: a property of the PAIR of allocations — the caller's input, the library's line buffer — about one pair in three on the
    # boxes seen; no allocation call, address or offset tells or controls it: profiles/round6_alloc_kind.txt).  `value` is what a
    # caller who owns ONE buffer gets: the timed steps run on the FIRST allocation.  What other allocations would have
    # given is measured as well and reported next to it (config.input_placement; N = 1 only): the harness allocates two more
    # inputs, lets the context settle on each (ten untimed phase-free byte scans) and, if one of them is faster than the first,
    # runs the same warm-up and timed steps on it (--full only).  FQH_BENCH_INPUT_CANDIDATES=1 skips that.
    n_cand = int(os.environ.get("FQH_BENCH_INPUT_CANDIDATES", "3")) if (args.full and world == 1 and nbytes >= (2 << 30) and not args.pmc_child and args.stream_gib == 0) else 1
    cands, cand_ms = [], []
    for k in range(max(1, n_cand)):
        st_k = torch.empty(LEAD + nbytes + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(st_k[LEAD:].data_ptr(), lo, nbytes)
        ms_k = []
        if n_cand > 1:
            for _ in range(10):
                ctx.shard_prescan(st_k[LEAD:].data_ptr(), nbytes)
                ms_k.append(ctx.timing().index_ms)
        cands.append(st_k)
        cand_ms.append(round(min(ms_k[-4:]), 4) if ms_k else None)
    fastest = min(range(len(cands)), key=lambda k: cand_ms[k]) if n_cand > 1 else 0
    store = cands[0]
    input_placement = {"candidates": len(cands), "settled_index_ms": cand_ms, "timed_on": 0, "fastest": fastest,
                       "note": "16 GiB allocations differ (DESIGN.md 4b); `value` is measured on the FIRST allocation, what a caller who "
                               "owns one buffer gets; `best_allocation` (if another candidate's byte scan is more than 1 % faster) is the "
                               "same warm-up and timed steps on that one"} if n_cand > 1 else {"candidates": 1}
    alt_store = cands[fastest] if (n_cand > 1 and fastest != 0 and cand_ms[fastest] < 0.99 * cand_ms[0]) else None
    del cands, st_k
    buf = store[LEAD:]
    cur = {"buf": buf}   # (the buffer the steps run on: the first allocation, later — once — the fastest candidate)
    # FQH_BENCH_INJECT=<file offset of a separator line's '+'> (tests only): that byte becomes '-', and the run must report
    # Parser::each's error for it — "Sequence and quality not separated by +" at record offset // RECLEN — instead of totals
    inject = int(os.environ.get("FQH_BENCH_INJECT", "-1"))
    if inject >= 0:
        assert inject % RECLEN == 177, "FQH_BENCH_INJECT must point at a '+' (offset 177 of a %d-byte record)" % RECLEN
        if lo <= inject < hi and args.stream_gib == 0:
            buf[inject - lo] = ord("-")
    cap = nbytes // 300 + 16
    rec_start = torch.empty(cap, dtype=torch.int64, device=dev)
    is_last = rank == world - 1

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # N > 1: the exchange stays on the device (fqh_shard_prescan_launch / fqh_shard_rescan_launch): the byte scan, an
    # all_gather of 8 words per rank, the fold of the carries + the emit step, an all_reduce of the counts — all
    # enqueued on one stream, one host wait at the end of the step.  If a shard cannot keep the fast path, every rank's
    # finish says so (E_AGAIN) and the step runs the host recipe (prescan, exchange through pinned staging,
    # fqh_carry_combine on the host, rescan).
    W = pkg.SHARD_WORDS
    words = torch.zeros(W, dtype=torch.int64, device=dev)
    all_words = torch.zeros(world * W, dtype=torch.int64, device=dev) if world > 1 else None
    gather_in = torch.zeros(7, dtype=torch.int64, device=dev)
    gather_all = torch.zeros(world * 7, dtype=torch.int64, device=dev) if world > 1 else None
    h_in = torch.zeros(7, dtype=torch.int64).pin_memory() if world > 1 else None
    h_all = torch.zeros(world * 7, dtype=torch.int64).pin_memory() if world > 1 else None
    h_counts = torch.zeros(2, dtype=torch.int64).pin_memory() if world > 1 else None
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    index_ms = []
    host_steps = [0]
    last = {}   # (the carry the last step handed back, for --dump-outputs)

    def step_host():
        # 1) shard-local byte scan (phase-free), 2) carry exchange, 3) emit with the true carry
        host_steps[0] += 1
        nn, ns, back0 = ctx.shard_prescan(cur["buf"].data_ptr(), nbytes)
        index_ms.append(ctx.timing().index_ms)
        h_in[0], h_in[1], h_in[2] = nbytes, nn, ns
        h_in[3], h_in[4], h_in[5], h_in[6] = back0
        gather_in.copy_(h_in, non_blocking=True)
        coll.gather_dev(gather_in, gather_all)
        h_all.copy_(gather_all, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rows = h_all.numpy().reshape(world, 7)
        carry = None
        for r in range(rank):
            carry = pkg.carry_combine(carry, int(rows[r][0]), int(rows[r][1]), int(rows[r][2]),
                                      [int(x) for x in rows[r][3:7]])
        ctx.rescan_launch(is_last, carry, rec_start.data_ptr(), cap)
        s, c, st = ctx.scan_finish()
        last["carry"] = c
        h_counts[0] = s.n_records
        h_counts[1] = 1 if s.parse_status != pkg.OK else 0
        counts.copy_(h_counts, non_blocking=True)
        coll.sum_dev(counts)
        return s

    def step():
        if world == 1:
            s, c, st = ctx.scan(cur["buf"].data_ptr(), nbytes, True, None, rec_start.data_ptr(), cap)
            index_ms.append(ctx.timing().index_ms)
            last["carry"] = c
            return s
        if os.environ.get("FQH_BENCH_HOST_PROTOCOL") == "1":
            return step_host()
        ctx.shard_prescan_launch(cur["buf"].data_ptr(), nbytes, words.data_ptr())
        coll.gather_dev(words, all_words)    # RCCL (fqh_allgather or torch's), enqueued on the step's stream; gloo: two host hops, never a timed configuration
        ctx.shard_rescan_launch(is_last, all_words.data_ptr(), world, rank, rec_start.data_ptr(), cap, counts.data_ptr())
        coll.sum_dev(counts)
        try:
            s, c, st = ctx.scan_finish()
        except pkg.FqhError as e:
            if e.status != pkg.E_AGAIN:
                raise
            if os.environ.get("FQH_BENCH_DEBUG") and host_steps[0] == 0:
                print("rank %d: E_AGAIN, gathered words %s" % (rank, all_words.cpu().numpy().reshape(world, W).tolist()), file=sys.stderr, flush=True)
            return step_host()
        index_ms.append(ctx.timing().index_ms)
        last["carry"] = c
        return s

    if args.stream_gib > 0:
        emit_line(dict(stream_leg(args, pkg, torch, dev, buf, args.stream_gib, args.producer_threads), mode="stream"))
        return
    # FQH_OPT_ADAPT_LINES (default on): the library learns from its first calls on an input which of two line buffers that input
    # runs faster with (calls 1-2 on the first, then one call per alternate tried: DESIGN.md 4b).  A few untimed steps in
    # front of the warm-up let that settle, so that no alternate is allocated or tried inside the timed region.
    import gc

    def timed_steps():
        """settle (untimed, until the context's line buffer for this input is chosen), warm-up, then exactly --steps steps between
        two barriers -> (seconds, last summary, settle steps run)"""
        settle = 0 if args.pmc_child else int(os.environ.get("FQH_BENCH_SETTLE_STEPS", "8"))
        for i in range(settle):
            step()
            if world == 1 and i >= 1 and not ctx.line_buffers()["unsettled"]:   # (N > 1: every rank runs the same number of steps)
                settle = i + 1
                break
        gc.collect()
        gc.disable()   # (the timed region is 20 steps of < 3 ms: one collector pause of the interpreter would be a tenth of it)
        for _ in range(args.warmup):
            step()
        index_ms.clear()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            s_ = step()
        barrier()
        dt_ = time.perf_counter() - t0
        gc.enable()
        return dt_, s_, settle

    dt, s, settle = timed_steps()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, np, torch, rec_start, s, last["carry"], "" if world == 1 else "_rank%d" % rank)
    index_ms_first = list(index_ms)
    best_allocation = None
    if alt_store is not None and inject < 0:
        # the same steps on the fastest of the other candidates: what an allocation of the other kind would have given this run
        cur["buf"] = alt_store[LEAD:]
        dt2, s2, settle2 = timed_steps()
        assert s2.parse_status == pkg.OK and int(s2.n_records) == total_records
        best_allocation = {"candidate": fastest, "ms_per_step": round(dt2 / args.steps * 1e3, 4),
                           "value": round(file_len / 1e9 / (dt2 / args.steps), 2), "index_kernel_ms": round(float(np.mean(index_ms)), 4),
                           "settle_steps": settle2}
        cur["buf"] = buf
        index_ms[:] = index_ms_first
    alt_store = None
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        n_rec_total = int(counts[0].item())
        n_err = int(counts[1].item())
    else:
        n_rec_total = int(s.n_records)
        n_err = 0 if s.parse_status == pkg.OK else 1
    first_error = None
    if inject >= 0:
        # the first error in file order: MIN over the ranks of (failing record, kind) — what Parser::parallel_each returns
        # (src/lib.rs:544-547, 561-564)
        key = ((int(s.err_record) << 3) | int(s.parse_status)) if s.parse_status != pkg.OK else (1 << 62)
        gk = coll.min_key(key)
        first_error = {"status": gk & 7, "n_records": gk >> 3, "expected": {"status": pkg.E_SEP, "n_records": inject // RECLEN}}
        assert n_err >= 1 and (gk & 7, gk >> 3) == (pkg.E_SEP, inject // RECLEN), first_error
    else:
        assert n_err == 0, "scan reported a parse error on valid synthetic input"
        assert n_rec_total == total_records, (n_rec_total, total_records)

    ms_per_step = dt / args.steps * 1e3
    gbs = file_len / 1e9 / (dt / args.steps)
    k_ms = float(np.mean(index_ms))
    achieved = nbytes / 1e9 / (k_ms / 1e3)

    # From the committed rocprofv3 passes of the same command (tools/prof.sh -> profiles/round3_rocprof.json; only valid
    # for the workload they were measured on): HBM bytes per launch of the dominant kernel (PMC), and its duration as
    # rocprofv3 --kernel-trace saw it, next to the HIP-event figure of THIS run.
    traffic = rp = None
    traffic_source = None
    if args.pmc_child:   # (a child of pmc_traffic below: the counters are rocprofv3's business, the line is not looked at)
        emit_line({"pmc_child": True, "kernel_ms": round(k_ms, 4)})
        ctx.read_ceiling(buf.data_ptr(), nbytes)
        return
    if args.full and world == 1 and args.pmc_traffic == "auto":
        live = pmc_traffic(nbytes)
        if live:
            traffic, traffic_source = live["hbm_bytes_per_launch"], live["source"]
    for prof in ("round5_rocprof.json", "round4_rocprof.json", "round3_rocprof.json"):
        try:
            with open(os.path.join(ROOT, "profiles", prof)) as f:
                pj = json.load(f)
            if pj.get("workload_bytes") == nbytes:
                rp = pj["k_index_fast"]
                if traffic is None:
                    traffic = rp.get("hbm_bytes_per_launch")
                    traffic_source = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, a committed run of the same command)" % prof
                break
        except Exception:
            pass
    out = {
        "metric": "GB/s FASTQ parsed (record-offset scan + count, 150 bp synthetic, HBM-resident)",
        "value": round(gbs, 2),
        "unit": "GB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {"workload": "configs[1]: %d x %.3f GiB synthetic 150 bp FASTQ resident in HBM, "
                               "record-offset scan + count + validation" % (world, nbytes / 2**30),
                   "bytes_per_gpu": nbytes, "records_total": total_records,
                   "host_wait": "FQH_OPT_SPIN_WAIT %d us (opt-in of this harness; library default 0)" % spin_us,
                   "line_buffer": "FQH_OPT_ADAPT_LINES (library default): %d untimed steps in front of the warm-up let the context settle "
                                  "which of its line buffers this input takes" % settle,
                   "input_placement": input_placement,
                   "sharding": "byte-range, cuts at multiples of %d" % shard if world > 1 else "none",
                   "exchange": ("on the device: all_gather of 8 words per rank, fold + emit, all_reduce of the counts, one "
                                "host wait per step (%d of %d timed+warmup steps fell back to the host recipe)"
                                % (host_steps[0], args.steps + args.warmup)) if world > 1 else "none"},
        "rccl": rccl,
        "records_per_s": round(total_records / (dt / args.steps), 1),
        "hbm_roofline_frac_whole_step": round(gbs / world / HBM_PEAK_GBS, 4),
        "roofline": {"bound": "hbm", "kernel": "k_index_fast", "achieved": round(achieved, 1),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic, "traffic_source": traffic_source,
                     "kernel_ms": round(k_ms, 4), "kernel_ms_source": "HIP events on the launch stream, this run, mean of the timed steps",
                     "kernel_ms_min": round(float(np.min(index_ms)), 4), "kernel_ms_max": round(float(np.max(index_ms)), 4),
                     "kernel_ms_rocprof_avg": rp.get("avg_ms") if rp else None,
                     "kernel_ms_rocprof_min": rp.get("min_ms") if rp else None,
                     "kernel_ms_rocprof_max": rp.get("max_ms") if rp else None,
                     "algorithmic_bytes_per_launch": nbytes},
    }

    if best_allocation:
        out["best_allocation"] = best_allocation
    out["placement"] = ctx.placement()   # FQH_OPT_PLACE_TRIES (FQH_BENCH_PLACE_TRIES here; default 0 = no search)
    if first_error:
        out["first_error"] = first_error
        if rank == 0:
            emit_line(out)
        return
    if world == 1:
        # what the last timed step left in the caller's array: record k of the synthetic file starts at 330 k (every record of
        # fqh_synth_fill is RECLEN bytes), so the offsets' sum is known in closed form — a figure outside the library's own
        # summary that says the scan wrote what it says it wrote
        got = int(rec_start[:total_records].sum().item())
        exp = RECLEN * total_records * (total_records - 1) // 2
        assert got == exp, ("rec_start checksum", got, exp)
        out["rec_start_checksum"] = {"sum_of_offsets": got, "expected": exp, "records": total_records,
                                     "rule": "record k starts at byte %d k" % RECLEN}
    if rank == 0 and world == 1:
        t = ctx.timing()
        out["stage_ms"] = {"index": round(t.index_ms, 4), "prefix": round(t.prefix_ms, 4),
                           "emit": round(t.emit_ms, 4), "total": round(t.total_ms, 4)}
    if rank == 0 and world == 1 and args.full:
        rc_ms = [ctx.read_ceiling(buf.data_ptr(), nbytes)[1] for _ in range(6)]   # (a ceiling is the fastest launch, not an average)
        out["read_ceiling_gbs"] = round(nbytes / 1e9 / (min(rc_ms) / 1e3), 1)
        out["read_ceiling_ms"] = {"min": round(min(rc_ms), 4), "max": round(max(rc_ms), 4), "launches": len(rc_ms)}
        if not args.no_stats:
            # configs[2]: the histograms, end to end.  A COLD fqh_stats (nothing cached from the scan above: the single pass
            # reads the input once for offsets, validation and histograms), wall time around the blocking call.
            qh = torch.zeros(150 * 256, dtype=torch.int64, device=dev)
            bh = torch.zeros(150 * 8, dtype=torch.int64, device=dev)
            sc = torch.zeros(8, dtype=torch.int64, device=dev)

            def timed(fn, reps=6):
                best = None
                for _ in range(reps):
                    qh.zero_(); bh.zero_(); sc.zero_()
                    ctx.invalidate()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    w = (time.perf_counter() - t1) * 1e3
                    tt = ctx.timing()
                    if best is None or w < best[0]:
                        best = (w, tt.index_ms, tt.total_ms, ctx.last_scan_fast())
                    assert int(sc[0].item()) == total_records
                    assert int(qh.sum().item()) == total_records * 150 and int(bh.sum().item()) == total_records * 150
                return best

            one = timed(lambda: ctx.stats(buf.data_ptr(), nbytes, 150, qh.data_ptr(), bh.data_ptr(), sc.data_ptr()))
            both = timed(lambda: ctx.scan_stats(buf.data_ptr(), nbytes, 150, qh.data_ptr(), bh.data_ptr(), sc.data_ptr(),
                                                d_rec_start=rec_start.data_ptr(), cap=cap))
            # the same call from a host that sizes its arrays for whatever may come (1000 rows over 150-base reads): the pass keeps
            # the rows the READS need (a look at the input's first 64 KiB), lmax only says where the caller's arrays end
            qh_k = torch.zeros(1000 * 256, dtype=torch.int64, device=dev)
            bh_k = torch.zeros(1000 * 8, dtype=torch.int64, device=dev)
            rows_k = None
            for _ in range(3):
                qh_k.zero_(); bh_k.zero_(); sc.zero_()
                ctx.invalidate()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ctx.stats(buf.data_ptr(), nbytes, 1000, qh_k.data_ptr(), bh_k.data_ptr(), sc.data_ptr())
                torch.cuda.synchronize()
                w = (time.perf_counter() - t1) * 1e3
                rows_k = w if rows_k is None else min(rows_k, w)
                assert int(sc[0].item()) == total_records and int(qh_k.sum().item()) == total_records * 150
                assert int(qh_k.view(1000, 256)[150:].sum().item()) == 0 and int(bh_k.sum().item()) == total_records * 150
            rows_k_route = ctx.last_stats_route()
            del qh_k, bh_k
            ctx.set_single_pass(False)
            two = timed(lambda: ctx.stats(buf.data_ptr(), nbytes, 150, qh.data_ptr(), bh.data_ptr(), sc.data_ptr()), reps=2)
            ctx.set_single_pass(True)
            # the same call on input with ANY bytes in seq() / qual() (src/records.rs:19-33, 75-90): one base in a million
            # lower-cased, one quality in a million '~' (outside the kernel's window).  The single pass dumps the batches of eight
            # lines it will not count and k_stats_declined counts them behind it; the scan's result stands, and the plain scan
            # that follows takes the fast path (a count the kernel declines is no doubt about the parse).
            gen = torch.Generator(device=dev)
            gen.manual_seed(20260930)
            nd = max(1, int(total_records * 150 * 1e-6))
            pos_s = torch.unique(torch.randint(0, total_records, (nd,), device=dev, generator=gen) * RECLEN + 26 +
                                 torch.randint(0, 150, (nd,), device=dev, generator=gen))
            pos_q = torch.unique(torch.randint(0, total_records, (nd,), device=dev, generator=gen) * RECLEN + 179 +
                                 torch.randint(0, 150, (nd,), device=dev, generator=gen))
            keep_s, keep_q = buf[pos_s].clone(), buf[pos_q].clone()
            buf[pos_s] = keep_s | 0x20
            buf[pos_q] = 126
            dirty = timed(lambda: ctx.stats(buf.data_ptr(), nbytes, 150, qh.data_ptr(), bh.data_ptr(), sc.data_ptr()), reps=3)
            dirty_route = ctx.last_stats_route()
            assert int(bh.view(150, 8)[:, 5].sum().item()) == pos_s.numel() and int(qh.view(150, 256)[:, 126].sum().item()) == pos_q.numel()
            ds, dc, dst = ctx.scan(buf.data_ptr(), nbytes, True, None, rec_start.data_ptr(), cap)
            dirty_scan_fast = ctx.last_scan_fast()
            assert ds.n_records == total_records and ds.parse_status == pkg.OK
            buf[pos_s] = keep_s
            buf[pos_q] = keep_q
            ctx.invalidate()
            out["stats"] = {
                "workload": "configs[2]: per-position quality + base histograms, same buffer, cold call (fqh_stats)",
                "route": "single pass: k_scan_stats reads the input once for offsets, validation and histograms" if one[3]
                         else "two passes (the single pass was not kept)",
                "kernel": "k_scan_stats", "input_reads": 1 if one[3] else 2,
                "end_to_end_ms": round(one[0], 3), "kernel_ms": round(one[1], 3), "all_kernels_ms": round(one[2], 3),
                "gbs_end_to_end": round(nbytes / 1e6 / one[0], 1),
                "frac_of_hbm_peak_end_to_end": round(nbytes / 1e6 / one[0] / HBM_PEAK_GBS, 4),
                "scan_offsets_and_histograms_end_to_end_ms": round(both[0], 3),
                "two_pass_route_end_to_end_ms": round(two[0], 3),
                "lmax_1000_end_to_end_ms": round(rows_k, 3), "lmax_1000_stats_route": rows_k_route,
                "dirty_input": {"what": "the same cold call with 1e-6 of the bases lower-cased and 1e-6 of the qualities '~' (%d + %d bytes)"
                                        % (pos_s.numel(), pos_q.numel()),
                                "end_to_end_ms": round(dirty[0], 3), "stats_route": dirty_route,
                                "route": {2: "single pass + the declined batches counted behind it (k_stats_declined)",
                                          1: "single pass", 0: "second pass over the input"}[dirty_route],
                                "next_plain_scan_on_fast_path": bool(dirty_scan_fast)},
                "bound": "vector ALU issue, then LDS atomics (DESIGN.md 5b); HBM is read once"}
        if not args.no_stats and not args.no_long_reads:
            out["long_reads"] = long_read_leg(pkg, torch, dev, ctx)
            out["long_reads_varied"] = long_read_leg(pkg, torch, dev, ctx, varied=True)
        if not args.no_stream:
            out["stream"] = stream_leg(args, pkg, torch, dev, buf, args.default_stream_gib, args.producer_threads)
        if not args.no_cpu_baseline:
            from oracle import fqref  # the oracle as timed CPU baseline (kind "port"), never the product
            # SURVEY 8(d) cfg 0: examples/fastq-count.rs on a 2 GiB file on a ramdisk: the oracle's Parser::each reads the
            # file through its 68 KiB Buffer, one read(2) per refill, 1 thread (the reference scan is single-threaded)
            sample = min(nbytes, 2 << 30) // RECLEN * RECLEN
            host = buf[:sample].cpu().numpy()
            path = "/dev/shm/fqh_bench_%d.fastq" % os.getpid()
            best = None
            host_api = None
            try:
                host.tofile(path)
                for _ in range(3):
                    t1 = time.perf_counter()
                    r = fqref.count_file(path)
                    d1 = time.perf_counter() - t1
                    best = d1 if best is None else min(best, d1)
                if not args.no_host_api:
                    exp_hist = torch.zeros(8 + 150 * 264, dtype=torch.int64, device=dev)
                    ctx.stats(buf.data_ptr(), sample, 150, exp_hist[8: 8 + 150 * 256].data_ptr(), exp_hist[8 + 150 * 256:].data_ptr(),
                              exp_hist[:8].data_ptr())
                    host_api = host_api_leg(path, sample, exp_hist.cpu().numpy().astype("uint64"))
            finally:
                if os.path.exists(path):
                    os.remove(path)
            assert r.status == 0 and r.n_records == sample // RECLEN
            model = "unknown"
            try:
                with open("/proc/cpuinfo") as f:
                    model = [l.split(":", 1)[1].strip() for l in f if l.startswith("model name")][0]
            except Exception:
                pass
            out["cpu_baseline"] = {"value": round(sample / 1e9 / best, 3), "unit": "GB/s", "cores": 1,
                                   "kind": "port",
                                   "sample": "configs[0]: the oracle's fastq-count (Parser::each through the 68 KiB Buffer, "
                                             "one read(2) per refill) over a %.2f GiB file of the same synthetic bytes on "
                                             "/dev/shm, best of 3, 1 thread; host: %s, %d logical cores"
                                             % (sample / 2**30, model, os.cpu_count())}
            if host_api is not None:
                out["host_api"] = host_api
            hs = min(sample, 512 << 20) // RECLEN * RECLEN
            t1 = time.perf_counter()
            fqref.stats(host[:hs], 150)
            d1 = time.perf_counter() - t1
            out["cpu_baseline"]["stats_gbs"] = round(hs / 1e9 / d1, 3)
            # the histogram loop the way parallel_each would run it: record-aligned pieces on worker threads
            # (ctypes releases the GIL), all cores
            from concurrent.futures import ThreadPoolExecutor
            nthr = max(1, os.cpu_count() or 1)
            per = (sample // RECLEN + nthr - 1) // nthr * RECLEN
            pieces = [host[i:i + per] for i in range(0, sample, per)]
            with ThreadPoolExecutor(nthr) as ex:
                t1 = time.perf_counter()
                list(ex.map(lambda h: fqref.stats(h, 150), pieces))
                d1 = time.perf_counter() - t1
            out["cpu_baseline"]["stats_parallel_gbs"] = round(sample / 1e9 / d1, 3)
            out["cpu_baseline"]["stats_parallel_threads"] = nthr
    if args.full and world == 1 and coll.comm:
        # the HBM-resident protocol once through the library's own RCCL binding with a communicator of this one rank (untimed):
        # words -> fqh_allgather -> fold + emit -> fqh_allreduce_u64, one host wait — what every step does at N > 1
        w1 = torch.zeros(W, dtype=torch.int64, device=dev)
        ctx.shard_prescan_launch(buf.data_ptr(), nbytes, words.data_ptr())
        coll.gather_dev(words, w1)
        ctx.shard_rescan_launch(True, w1.data_ptr(), 1, 0, rec_start.data_ptr(), cap, counts.data_ptr())
        coll.sum_dev(counts)
        s1, _, _ = ctx.scan_finish()
        assert (s1.parse_status, int(s1.n_records)) == (pkg.OK, total_records) and counts.cpu().tolist() == [total_records, 0]
        out["rccl"]["protocol_check"] = "one HBM-resident sharded step (prescan, fqh_allgather, fold + emit, fqh_allreduce_u64) through a 1-rank fqh_comm: %d records" % total_records
    if args.full and not args.no_shard_stream:
        # configs[4] in every --full line: the sharded, host-streamed leg at this world size next to the same
        # function at world size 1
        inj = int(os.environ.get("FQH_BENCH_INJECT_STREAM", "-1"))   # (tests only)
        if inj >= 0:
            rec = sharded_stream(args, pkg, torch, dev, ctx, coll, args.default_shard_stream_gib, inj)
        else:
            rec = sharded_stream_record(args, pkg, torch, dist, dev, ctx, coll, backend, via, args.default_shard_stream_gib)
        out["sharded_stream"] = rec
    if rank == 0:
        emit_line(out)
    if world > 1 and args.shard_stats:
        # histograms over byte-range shards.  The record that straddles a cut is counted by the
        # rank it ENDS in, which needs its beginning: the last LEAD bytes of every shard are all-gathered
        # (world x 136 KiB) and rank r puts rank r-1's in front of its buffer; then one all_reduce of
        # [scalars, quality histogram, base histogram].
        tails = torch.empty(world * LEAD, dtype=torch.uint8, device=dev)
        coll.gather_dev(buf[nbytes - LEAD: nbytes].contiguous(), tails)
        if rank:
            store[:LEAD].copy_(tails[(rank - 1) * LEAD: rank * LEAD])
        rows = h_all.numpy().reshape(world, 7)
        carry = None
        for r in range(rank):
            carry = pkg.carry_combine(carry, int(rows[r][0]), int(rows[r][1]), int(rows[r][2]),
                                      [int(x) for x in rows[r][3:7]])
        LMAX = 150
        hist = torch.zeros(8 + LMAX * 256 + LMAX * 8, dtype=torch.int64, device=dev)
        sc, qh, bh = hist[:8], hist[8: 8 + LMAX * 256], hist[8 + LMAX * 256:]
        barrier()
        t1 = time.perf_counter()
        ctx.stats_launch_lead(buf.data_ptr(), nbytes, LEAD if rank else 0, LMAX, qh.data_ptr(), bh.data_ptr(),
                              sc.data_ptr(), is_final=is_last, carry=carry)
        s2, _ = ctx.stats_finish()
        coll.sum_dev(hist)
        barrier()
        dts = time.perf_counter() - t1
        assert s2.parse_status == pkg.OK
        tot = hist.cpu().numpy()
        assert int(tot[0]) == total_records, (int(tot[0]), total_records)
        assert int(tot[1]) == int(tot[2]) == total_records * 150
        assert int(tot[8: 8 + LMAX * 256].sum()) == total_records * 150 == int(tot[8 + LMAX * 256:].sum())
        if rank == 0:
            emit_line({"mode": "shard-stats", "n_gpus": world, "records_total": int(tot[0]),
                       "seconds_incl_full_index_and_allreduce": round(dts, 4),
                       "check": "sum over ranks: records, bases, quality and base histogram totals match the "
                                "generator's; every cut-straddling record counted exactly once"})
    coll.close()
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


DUMP_SAMPLE = 1 << 21   # record offsets --dump-outputs writes at most (16 MiB of float64, as much again for their record numbers)


def dump_outputs(d, np, torch, rec_start, s, carry, suffix=""):
    """--dump-outputs DIR: what the last timed step handed its caller, as float64 .npy (offsets < 2^53 are exact).
    rec_start + rec_start_index: the record offsets and their record numbers — all of them up to DUMP_SAMPLE records, else the
    first and last DUMP_SAMPLE / 4 and a fixed seeded sample of the rest; summary: fqh_summary's fields in order (the reserved
    word left out); carry: base_offset, nl_count, back[4]."""
    os.makedirs(d, exist_ok=True)
    n = min(int(s.n_records), rec_start.numel())
    if n <= DUMP_SAMPLE:
        idx = np.arange(n, dtype=np.int64)
    else:
        edge = DUMP_SAMPLE // 4
        mid = np.random.default_rng(20261016).integers(edge, n - edge, DUMP_SAMPLE // 2)
        idx = np.unique(np.concatenate([np.arange(edge), mid, np.arange(n - edge, n)]))
    vals = rec_start[torch.from_numpy(idx).to(rec_start.device)].cpu().numpy()
    summary = [getattr(s, f) for f, _ in s._fields_ if f != "reserved"]
    for name, a in (("rec_start", vals), ("rec_start_index", idx), ("summary", summary),
                    ("carry", [carry.base_offset, carry.nl_count] + list(carry.back))):
        np.save(os.path.join(d, "%s%s.npy" % (name, suffix)), np.asarray(a, dtype=np.float64))


def host_api_leg(path, nbytes, exp_hist):
    """The drop-in surface itself, timed (outside `value`): host/bin/fastq_count — the C++ mirror of the crate's Parser over the
    C ABI; examples/fastq-count.rs:14-23 and, with --threads, examples/fastq-count-thread.rs — on the configs[0] file the
    cpu_baseline leg wrote to /dev/shm, next to the oracle's fastq-count on one core.  Every variant parses the file three times
    in one process (--repeat 3): pass 0 pays the HIP runtime's start-up, the best later pass is the path.  Variants: Parser::each
    / parallel_each(8) with the reference's one reader thread, the same with 8 pread()s side by side per ring slot
    (Options::read_threads) and with a filler thread of the parser's own on top (Options::read_ahead), and the histogram consumer (FQH_STREAM_STATS: the loop over Record::seq()/qual() on the GPU while the file streams)."""
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq-rs_amd", "host", "bin", "fastq_count")
    if not os.path.exists(exe):
        return {"error": "%s is not built (make -C fastq-rs_amd/host)" % exe}
    n_rec = nbytes // RECLEN
    checksum = int((exp_hist * (1 + __import__("numpy").arange(exp_hist.size, dtype="uint64"))).sum(dtype="uint64"))
    one = ["--read-threads", "1"]   # (the reference's one reader; fastq_count's own default is up to eight pread()s per slot)
    variants = [("each", one), ("each_read8", ["--read-threads", "8"]), ("each_read8_ahead", ["--read-threads", "8", "--read-ahead"]),
                ("parallel_each8", ["--threads", "8"] + one), ("parallel_each8_read8", ["--threads", "8", "--read-threads", "8"]),
                ("parallel_each8_read8_ahead", ["--threads", "8", "--read-threads", "8", "--read-ahead"]),
                ("stats150", ["--stats", "150"] + one), ("stats150_read8", ["--stats", "150", "--read-threads", "8"]),
                ("each_default_options", [])]
    res = {"file": "configs[0]: %.2f GiB of the synthetic file on /dev/shm" % (nbytes / 2**30), "binary": "fastq-rs_amd/host/bin/fastq_count",
           "note": "GB/s of the best warm pass of three in one process (pass 0 = cold: HIP start-up, context, ring); one process per "
                   "variant; ring 3-4 x 32 MiB; the oracle's one-core rate is cpu_baseline.value"}
    for name, flags in variants:
        try:
            t0 = time.perf_counter()
            p = subprocess.run([exe, path, "--repeat", "3"] + flags, capture_output=True, text=True, timeout=300)
            wall = time.perf_counter() - t0
        except Exception as e:  # noqa: BLE001
            res[name] = {"error": repr(e)}
            continue
        passes = [float(x) for x in re.findall(r"pass \d+: ([0-9.]+) s", p.stderr)]
        outl = p.stdout.split()
        ok = p.returncode == 0 and len(passes) == 3
        if ok and "--stats" in flags:
            ok = outl[-3:] == [str(n_rec), str(n_rec * 150), str(checksum)]
        elif ok:
            ok = outl[-1:] == [str(n_rec)]
        if not ok:
            res[name] = {"error": "rc %d, stdout %r, stderr %r" % (p.returncode, p.stdout[-200:], p.stderr[-300:])}
            continue
        warm = min(passes[1:])
        res[name] = {"gbs": round(nbytes / 1e9 / warm, 2), "records_per_s": round(n_rec / warm, 1), "seconds_warm": round(warm, 4),
                     "seconds_cold_pass": round(passes[0], 4), "process_wall_seconds": round(wall, 3), "checked": "count" if "--stats" not in flags else "count, bases, histogram checksum"}
    return res


def pmc_traffic(nbytes):
    """HBM bytes per launch of k_index_fast from THIS box's counters: two short child runs of this script under
    `rocprofv3 --pmc` (FETCH_SIZE and WRITE_SIZE do not fit one pass, MI355X_MICROARCH.md), counters in KiB, FETCH_SIZE
    calibrated in the same pass on the plain read kernel k_read_ceiling (on gfx950 it reports half of a 16-byte-per-lane
    stream), as the guide prescribes.  -> dict, or None when rocprofv3 is not there / a pass fails (the caller falls back to
    the committed profile)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if not shutil.which("rocprofv3") or os.environ.get("FQH_BENCH_NO_PMC") == "1":
        return None
    got = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            with tempfile.TemporaryDirectory(dir="/tmp") as d:
                cmd = ["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                       sys.executable, os.path.abspath(__file__), "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-stats",
                       "--no-stream", "--pmc-child", "--bytes", str(nbytes)]
                env = dict(os.environ, TMPDIR="/tmp")
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=150, check=True)
                vals = {}
                for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                    for row in csv.DictReader(open(f)):
                        if row.get("Counter_Name") != counter:
                            continue
                        for k in ("k_index_fast", "k_read_ceiling"):
                            if k in row.get("Kernel_Name", ""):
                                vals.setdefault(k, []).append(float(row["Counter_Value"]))
                for k, v in vals.items():
                    big = [x for x in v if x > 0.5 * max(v)] if max(v) > 0 else v
                    got[(k, counter)] = sum(big) / len(big)
        fetch, write = got[("k_index_fast", "FETCH_SIZE")], got.get(("k_index_fast", "WRITE_SIZE"), 0.0)
        cal = nbytes / (got[("k_read_ceiling", "FETCH_SIZE")] * 1024.0)   # bytes per counted byte of a 16-byte-per-lane stream
        rd, wr = fetch * 1024.0 * cal, write * 1024.0
        return {"hbm_bytes_per_launch": int(rd + wr),
                "source": "this run: rocprofv3 --pmc FETCH_SIZE (%.0f KiB x %.3f, calibrated on k_read_ceiling in the same pass) + "
                          "--pmc WRITE_SIZE (%.0f KiB), two child runs of 2 steps, average over the full-size launches" % (fetch, cal, write)}
    except Exception:
        return None


def long_read_leg(pkg, torch, dev, ctx, read_len=5000, gib=4.0, varied=False):
    """Kilobase reads with PacBio-HiFi-like qualities (80 % '~' = Q93): the reference treats a record of any length up to its
    Buffer alike (src/lib.rs:276-283, src/records.rs:75-90); here they take the exact scan + fqh_index_records + k_stats_long
    (128 quality bins per column in LDS).  varied: the reads' lengths are log-normal around read_len (sigma 0.8,
    200 .. 6 x read_len: a long-read run, not a simulator's output) — the plan k_stats_long follows is made on the device from
    the lengths it finds.  Not part of `value`: evidence that the long-read route has no cliff."""
    import numpy as np
    rng = np.random.default_rng(7)
    nrec = 1024
    max_len = 6 * read_len if varied else read_len
    lens = np.clip(rng.lognormal(np.log(read_len), 0.8, nrec), 200, max_len).astype(np.int64) if varied else np.full(nrec, read_len)
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (nrec, max_len))
    qual = np.where(rng.random((nrec, max_len)) < 0.8, 126, rng.integers(33, 127, (nrec, max_len))).astype(np.uint8)
    block = b"".join(b"@m%06d/ccs\n" % i + seq[i, :lens[i]].tobytes() + b"\n+\n" + qual[i, :lens[i]].tobytes() + b"\n" for i in range(nrec))
    reps = int(gib * (1 << 30)) // len(block)
    n = reps * len(block)
    hb = torch.from_numpy(np.frombuffer(block, dtype=np.uint8).copy()).to(dev)
    d = torch.cat([hb.repeat(reps), torch.zeros(16, dtype=torch.uint8, device=dev)])
    qh = torch.zeros(max_len * 256, dtype=torch.int64, device=dev)
    bh = torch.zeros(max_len * 8, dtype=torch.int64, device=dev)
    sc = torch.zeros(8, dtype=torch.int64, device=dev)
    best = None
    for _ in range(4):
        qh.zero_(); bh.zero_(); sc.zero_()
        ctx.invalidate()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.stats(d.data_ptr(), n, max_len, qh.data_ptr(), bh.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        w = (time.perf_counter() - t1) * 1e3
        tt = ctx.timing()
        if best is None or w < best[0]:
            best = (w, tt.stats_ms)
    # the block's own histograms, counted on the host with numpy, times the repetitions
    exp_q = np.zeros((max_len, 256), dtype=np.int64)
    if varied:
        for i in range(nrec):
            np.add.at(exp_q, (np.arange(lens[i]), qual[i, :lens[i]]), 1)
    else:
        for c in range(0, read_len, 500):
            for v in np.unique(qual[:, c:c + 500]):
                exp_q[c:c + 500, v] = (qual[:, c:c + 500] == v).sum(axis=0)
    got_q = qh.cpu().numpy().reshape(max_len, 256)
    assert int(sc[0].item()) == reps * nrec and np.array_equal(got_q, exp_q * reps), "long-read histograms differ from the host count"
    assert int(bh.sum().item()) == reps * int(lens.sum())
    del d
    what = ("reads of log-normal length (median %d bp, sigma 0.8, %d .. %d bp)" % (read_len, int(lens.min()), int(lens.max()))) if varied \
        else "%d bp reads" % read_len
    return {"workload": "%.2f GiB of %s, 80 %% of the quality bytes '~' (Q93, PacBio HiFi-like), cold fqh_stats" % (n / 2**30, what),
            "route": "exact scan + record index + k_stats_long (128 quality bins per column in LDS; work items cut on the device from the reads' lengths)",
            "end_to_end_ms": round(best[0], 3), "histogram_kernels_ms": round(best[1], 3),
            "gbs_end_to_end": round(n / 1e6 / best[0], 1), "gbs_histograms": round(n / 1e6 / best[1], 1),
            "check": "quality histogram == numpy count of the repeated block x repetitions, bit-exact"}


def stream_leg(args, pkg, torch, dev, buf, gib, threads):
    """configs[3]: pageable host memory -> producer thread(s) -> pinned ring slot -> hipMemcpyAsync (side stream) -> scan, every
    slot scanned while the next one is copied and the one after that is filled (replaces src/thread_reader.rs:131-139: a reader
    thread fills boxes while the consumer parses).  The producer is REAL: every slot of every pass is filled again from a
    pageable source (a record-aligned region replayed) by `threads` threads, memcpy released from the GIL; with 1 thread that is
    the reference's one reader thread, whose memcpy rate — not the link — is then the bound.  -> dict for the JSON line."""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    slot = min(args.slot_mib << 20, (buf.numel() - 16) // RECLEN * RECLEN)
    region = slot // RECLEN * RECLEN      # record-aligned, so replaying it keeps the stream valid FASTQ
    region_recs = region // RECLEN
    numa = numa_pin(torch, dev.index, args.numa_pin)   # (before the pageable source and the pinned ring are first touched)
    host_src = buf[:region].cpu().numpy().copy()   # pageable
    LINK_GBS = 63.0                         # MI355X_MICROARCH.md: PCIe Gen5 x16
    runs = []
    # T = 0: no producer at all — the source region is page-locked where it lies (fqh_host_register) and every slot is DMA'd
    # straight from it (fqh_stream_submit_external, a ring without pinned data slots): what a host does with a resident or
    # mmap'ed file, and the one-reader host's way to the link's rate (1 B of host DRAM traffic per byte instead of 3)
    for T in ([threads] if threads else [1, 8, 0]):
        external = T == 0
        T = max(0 if external else 1, min(T, os.cpu_count() or 1))
        total = int(gib * (1 << 30)) // region * region
        if T == 1:
            total = min(total, (8 << 30) // region * region)   # (one thread fills ~10 GB/s: 8 GiB is second enough)
        n_chunks = max(3, total // region)
        total = n_chunks * region
        sctx = pkg.Ctx(dev.index)
        st = pkg.Stream(sctx, slot, 3, pkg.STREAM_TIMING | (pkg.STREAM_EXTERNAL if external else 0))
        pool = ThreadPoolExecutor(max(1, T))
        piece = (region + max(1, T) - 1) // max(1, T) // 64 * 64 + 64
        src = host_src.ctypes.data
        if external:
            sctx.host_register(src, region)

        def fill(addr):
            jobs = [pool.submit(C.memmove, addr + o, src + o, min(piece, region - o)) for o in range(0, region, piece)]
            for j in jobs:
                j.result()

        sent = got = recs = 0
        fill_s = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while got < n_chunks:
            while sent < n_chunks:
                if external:
                    if sent - got >= 3 or not st.submit_external(src, region, sent + 1 == n_chunks):
                        break
                    sent += 1
                    continue
                a = st.acquire()
                if a is None:
                    break
                t1 = time.perf_counter()
                fill(a[0])
                fill_s += time.perf_counter() - t1
                sent += 1
                st.submit(region, sent == n_chunks)
            c = st.collect()
            assert c.parse_status == pkg.OK
            recs += c.n_records
            got += 1
            st.release()
        dt = time.perf_counter() - t0
        tm = st.timing()
        assert recs == n_chunks * region_recs, (recs, n_chunks * region_recs)
        st.close()
        if external:
            sctx.host_unregister(src)
        sctx.close()
        pool.shutdown()
        runs.append({"producer_threads": T, "source": "registered in place (fqh_stream_submit_external)" if external else "pageable, copied into pinned slots",
                     "gib": round(total / 2**30, 2), "seconds": round(dt, 3),
                     "gbs": round(total / 1e9 / dt, 2), "pcie_frac": round(total / 1e9 / dt / LINK_GBS, 3),
                     "producer_gbs": round(total / 1e9 / fill_s, 2) if fill_s else None,
                     "records_per_s": round(recs / dt, 1),
                     "copy_busy_ms": round(tm.copy_busy_ms, 1), "scan_busy_ms": round(tm.scan_busy_ms, 1),
                     "copy_and_scan_both_busy_ms": round(tm.both_busy_ms, 1),
                     "scan_hidden_behind_copies_frac": round(tm.both_busy_ms / tm.scan_busy_ms, 3) if tm.scan_busy_ms else None,
                     "copy_stream_busy_frac_of_wall": round(tm.copy_busy_ms / (dt * 1e3), 3)})
    copied = [r for r in runs if r["producer_threads"] > 0] or runs
    best = max(copied, key=lambda r: r["gbs"])   # (the leg's `gbs` stays the producer model's: a pageable source copied into the ring)
    reg = [r for r in runs if r["producer_threads"] == 0]
    return {"registered_gbs": reg[0]["gbs"] if reg else None,
            "workload": "configs[3]: synthetic 150 bp FASTQ streamed from PAGEABLE host memory through a 3 x %d MiB pinned ring "
                        "(a %d MiB record-aligned region replayed; every slot of every pass is filled again by the producer "
                        "threads), hipMemcpyAsync on a side stream, scan of slot k enqueued before the host waits for slot k-1"
                        % (slot >> 20, region >> 20),
            "gbs": best["gbs"], "pcie_frac": best["pcie_frac"], "link_gbs": LINK_GBS, "numa": numa, "runs": runs,
            "note": "PCIe- and producer-inclusive: never `value`.  HIP events per slot on both streams (FQH_STREAM_TIMING)"}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start N ranks with torch.distributed.run (the driver's own command line)
    and hand its exit code back.  Refuses when the node has fewer than N GPUs, unless FQH_BENCH_ONE_GPU=1 asks for the
    functional mode (every rank on cuda:0, gloo instead of RCCL: RCCL does not put two ranks on one device)."""
    import socket
    import subprocess
    import torch
    one_gpu = os.environ.get("FQH_BENCH_ONE_GPU", "0") == "1"
    have = torch.cuda.device_count()
    if have < n and not one_gpu:
        print("bench.py: --gpus %d but this node has %d GPU(s); set FQH_BENCH_ONE_GPU=1 for the functional one-GPU mode (gloo)"
              % (n, have), file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    if one_gpu:
        env.setdefault("FQH_BENCH_BACKEND", "gloo")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def numa_pin(torch, dev_index, mode="auto"):
    """Run this process (and first-touch its pinned ring) on the NUMA node of its GPU.  -> {"node", "pinned", "cpus", "why"};
    mode "require": no pinning is an error, said loudly; "off": not attempted."""
    info = {"node": None, "pinned": False, "cpus": None, "why": None}
    if mode == "off":
        info["why"] = "--numa-pin off"
        return info
    try:
        p = torch.cuda.get_device_properties(dev_index)
        bdf = "%04x:%02x:%02x.0" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        with open("/sys/bus/pci/devices/%s/numa_node" % bdf) as f:
            node = int(f.read())
        info["node"] = node
        if node < 0:
            info["why"] = "the device reports no NUMA node (%s: numa_node = %d)" % (bdf, node)
        else:
            with open("/sys/devices/system/node/node%d/cpulist" % node) as f:
                cpus = set()
                for part in f.read().strip().split(","):
                    a, _, b = part.partition("-")
                    cpus.update(range(int(a), int(b or a) + 1))
            allowed = cpus & os.sched_getaffinity(0)
            if not allowed:
                info["why"] = "none of node %d's cpus is in this process's affinity mask" % node
            else:
                os.sched_setaffinity(0, allowed)
                info["pinned"] = True
                info["cpus"] = len(allowed)
    except Exception as e:   # no sysfs entry, no permission
        info["why"] = "%s: %s" % (type(e).__name__, e)
    if mode == "require" and not info["pinned"]:
        raise SystemExit("bench.py: --numa-pin require, but the process could not be pinned: %s" % info["why"])
    return info


class Coll:
    """The collectives of the sharded modes.  via "abi": the library's own RCCL binding (fqh_comm_create with an id that rank 0
    makes and torch's process group only carries to the others; fqh_allgather / fqh_allreduce_u64 / fqh_allreduce_min_u64 on the
    context's stream, csrc/comm.hip) — what fastq::each_sharded and a Rust host use, the gather of parallel_each's results
    (src/lib.rs:553-559) and the parse error it returns (src/lib.rs:544-547, 561-564).  via "torch": torch.distributed (the same
    RCCL under the nccl backend; gloo in the one-GPU functional mode, through host tensors).  The harness's own barrier and
    max-over-ranks timing stay with torch.distributed either way, as the launch contract prescribes."""

    def __init__(self, pkg, torch, dist, ctx, dev, world, rank, backend, via, local=False):
        self.pkg, self.torch, self.dist, self.ctx, self.dev = pkg, torch, dist, ctx, dev
        self.world, self.rank, self.backend, self.comm, self.local = world, rank, backend, None, local
        self.via_text = "torch.distributed (%s)" % backend if world > 1 else "none (one rank)"
        if via != "abi":
            return
        # rank 0 makes the id; the process group's object broadcast is only the messenger.  A rank that cannot bind RCCL says
        # so BEFORE anybody enters ncclCommInitRank (the others would wait there): then every rank stays with torch.
        uid, why = None, None
        if rank == 0 or local:
            try:
                uid = pkg.Comm.unique_id()
            except pkg.FqhError as e:
                why = str(e)
        if world > 1 and not local:
            box = [uid, why]
            dist.broadcast_object_list(box, src=0)
            uid, why = box
        if uid is None:
            self.via_text += "; fqh_comm unavailable: %s" % why
            return
        # Every rank creates its end, runs the three collectives once on known values and says whether they came out right; one
        # torch MIN over those verdicts decides for all: the library's binding, or torch.distributed for every rank (a binding
        # that fails on the first node that ever gives it more than one rank must not cost that node's whole record).
        def agree(ok, why):
            """-> None if every rank says ok, else the first (rank, why); all ranks get the same answer."""
            if world == 1 or local:
                return None if ok else (rank, why)
            verdicts = [None] * world
            dist.all_gather_object(verdicts, (ok, why))
            bad = [(r, w) for r, (o, w) in enumerate(verdicts) if not o]
            return bad[0] if bad else None

        def give_up(bad):
            if self.comm:
                try:
                    self.comm.close()
                except Exception:
                    pass
            self.comm = None
            self.via_text += "; fqh_comm given up: rank %d: %s" % bad

        # Stage 1: every rank creates its end.  Stage 2: the three collectives once, on known values.  After each stage one object
        # gather decides for ALL ranks: the library's binding, or torch.distributed for everybody (a binding that fails on the first
        # node that ever gives it more than one rank must not cost that node's whole record; and no rank may enter a collective
        # of a communicator that another rank has given up).
        ok, why = 1, None
        # (a communicator that never comes up — ncclCommInitRank waiting for a rank that is not coming — must not hold the node
        # until somebody's limit ends the job without a word: after FQH_BENCH_COMM_TIMEOUT seconds, default 300, this rank says what
        # it was waiting for and ends the process; --comm torch is the way around)
        import threading
        limit = float(os.environ.get("FQH_BENCH_COMM_TIMEOUT", "300"))

        def stuck():
            sys.stderr.write("bench.py: rank %d of %d: the library's RCCL binding (fqh_comm_create / its start-up collectives) did not "
                             "finish within %.0f s; giving the job up (run with --comm torch to keep torch.distributed's collectives)\n"
                             % (rank, world, limit))
            sys.stderr.flush()
            os._exit(3)
        watchdog = threading.Timer(limit, stuck) if (world > 1 and not local and limit > 0) else None
        if watchdog:
            watchdog.daemon = True
            watchdog.start()
        try:
            self.comm = pkg.Comm(ctx, world, rank, uid)
        except Exception as e:   # FqhError, or anything the runtime throws
            ok, why = 0, "%s: %s" % (type(e).__name__, e)
        bad = agree(ok, why)
        if bad:
            if watchdog:
                watchdog.cancel()
            return give_up(bad)
        if world > 1 and not local:
            try:
                mine = torch.tensor([rank + 1, 7], dtype=torch.int64, device=dev)
                allv = torch.zeros(2 * world, dtype=torch.int64, device=dev)
                self.comm.allgather(mine.data_ptr(), allv.data_ptr(), 16)
                tot = torch.tensor([rank + 1, 1], dtype=torch.int64, device=dev)
                self.comm.allreduce_u64(tot.data_ptr(), 2)
                low = torch.tensor([1000 + rank], dtype=torch.int64, device=dev)
                self.comm.allreduce_min_u64(low.data_ptr(), 1)
                self.comm.sync()
                want = [x for r in range(world) for x in (r + 1, 7)]
                if allv.cpu().tolist() != want or tot.cpu().tolist() != [world * (world + 1) // 2, world] or int(low.item()) != 1000:
                    ok, why = 0, "start-up check: wrong values (%s, %s, %s)" % (allv.cpu().tolist(), tot.cpu().tolist(), int(low.item()))
            except Exception as e:
                ok, why = 0, "%s: %s" % (type(e).__name__, e)
            bad = agree(ok, why)
            if bad:
                if watchdog:
                    watchdog.cancel()
                return give_up(bad)
        if watchdog:
            watchdog.cancel()
        self.via_text = "fqh_comm (libfastq_hip.so's own RCCL binding, %d rank%s%s)" % (
            world, "" if world == 1 else "s", "" if world == 1 or local else "; its three collectives checked on known values at start-up")

    def close(self):
        if self.comm:
            self.comm.close()
            self.comm = None

    @staticmethod
    def _nbytes(t):
        return t.numel() * t.element_size()

    def gather_dev(self, send, recv):
        """all-gather of a device tensor's bytes, enqueued on the context's (= torch's current) stream."""
        if self.comm:
            self.comm.allgather(send.data_ptr(), recv.data_ptr(), self._nbytes(send))
        elif self.world == 1:
            recv.view(-1)[: send.numel()].copy_(send.view(-1))
        elif self.backend == "nccl":
            self.dist.all_gather_into_tensor(recv, send)
        else:   # gloo gathers host tensors
            ha = self.torch.empty(recv.shape, dtype=recv.dtype)
            self.dist.all_gather_into_tensor(ha, send.cpu())
            recv.copy_(ha)

    def sum_dev(self, t):
        """element-wise SUM of u64 counters (int64 tensors: the same bits), in place, enqueued."""
        if self.comm:
            self.comm.allreduce_u64(t.data_ptr(), t.numel())
        elif self.world == 1:
            pass
        elif self.backend == "nccl":
            self.dist.all_reduce(t)
        else:
            h = t.cpu()
            self.dist.all_reduce(h)
            t.copy_(h)

    def min_key(self, key):
        """MINIMUM over the ranks of one u64 key (the first error in file order)."""
        torch = self.torch
        if self.comm:   # ncclMin over ncclUint64: the u64 bit pattern travels in an int64 tensor
            kt = torch.tensor([key - (1 << 64) if key >= (1 << 63) else key], dtype=torch.int64, device=self.dev)
            self.comm.allreduce_min_u64(kt.data_ptr(), 1)
            self.comm.sync()
            v = int(kt.item())
            return v + (1 << 64) if v < 0 else v
        if self.world == 1:
            return key
        kt = torch.tensor([key - (1 << 63)], dtype=torch.int64,   # (order-preserving map of the u64 key into torch's i64)
                          device=self.dev if self.backend == "nccl" else torch.device("cpu"))
        self.dist.all_reduce(kt, op=self.dist.ReduceOp.MIN)
        return int(kt.item()) + (1 << 63)

    def gather_words(self, words):
        """all-gather of a short list of u64 host words -> [world][len(words)] ints (host)."""
        torch = self.torch
        n = len(words)
        t_in = torch.tensor([x - (1 << 64) if x >= (1 << 63) else x for x in words], dtype=torch.int64, device=self.dev)
        t_all = torch.empty(self.world * n, dtype=torch.int64, device=self.dev)
        self.gather_dev(t_in, t_all)
        if self.comm:
            self.comm.sync()
        return [[int(x) & ((1 << 64) - 1) for x in row] for row in t_all.cpu().numpy().reshape(self.world, n)]

    # ---- the harness's own synchronisation (never the product's): torch.distributed, or nothing for a group of one
    def barrier(self):
        if self.world > 1 and not self.local:
            self.dist.barrier()
        if self.torch.cuda.is_available():
            self.torch.cuda.synchronize()

    def objects(self, obj):
        if self.world == 1 or self.local:
            return [obj]
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out


SHARD_SUB_RUNS = ("producer", "registered", "pinned_replay")


def sharded_stream(args, pkg, torch, dev, ctx, coll, gib_per_rank, inject=-1, sub_runs=SHARD_SUB_RUNS):
    """configs[4]: byte-range sharded AND host-streamed.  The file is the endless repetition of one block (a slot's worth of
    synthetic records), cut at multiples of a shard size that is NOT a multiple of the record size: every cut falls inside a
    record.  Each rank streams its range phase-free (fastq-rs_amd/sharded.py -> fqh_shard_stream_run), then: one all-gather of
    ten words per rank, the true-phase check, the record that straddles each cut parsed by the rank it ends in (through that
    rank's own read callback), one SUM of per-rank record slots + histograms and one MIN of the first-error keys.
    The SAME function runs at every world size (world 1 is the denominator of `ratio_vs_n1`), in three sub-runs:
      producer       the N = 1 leg's producer model (stream_leg): a PAGEABLE source, --producer-threads threads per rank, every
                     slot of every pass filled again — host-side work a real reader has (3 B of host DRAM traffic per byte);
      registered     the source block page-locked where it lies (fqh_host_register) and DMA'd IN PLACE
                     (fqh_shard_stream_run_mapped -> fqh_stream_submit_external): no staging copy, no producer threads, 1 B of
                     host DRAM traffic per byte — what a host does with an mmap'ed / already resident file;
      pinned_replay  no producer: a ring slot that already holds the block at this rotation is submitted as it is (after the
                     first three slots: always) — the link and the kernels alone, labelled as such.
    The ring's pinned slots are created BEFORE the timed region (FQH_OPT_KEEP_RING: the probe ring's memory is what every
    sub-run's ring is made of): a host that streams file after file pins once."""
    import ctypes as C
    import importlib
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    sharded = importlib.import_module("fastq_rs_amd.sharded")
    rank, world = coll.rank, coll.world
    numa = numa_pin(torch, dev.index, args.numa_pin)    # (before the pageable source and the pinned rings are first touched)
    LMAX = 150
    blk = (args.slot_mib << 20) // 2640 * 2640          # multiple of the record size (330) and of 16
    shard = max(blk, int(gib_per_rank * (1 << 30)) // blk * blk) + 997   # cuts inside records
    file_len = world * shard // RECLEN * RECLEN          # (the last rank's range is a few bytes shorter)
    lo, hi = rank * shard, min((rank + 1) * shard, file_len)
    T = args.producer_threads or max(1, min(8, (os.cpu_count() or 1) // max(1, world if not coll.local else 1)))
    # the block, generated on the GPU, and its image in PAGEABLE host memory
    d_blk = torch.empty(blk + 16, dtype=torch.uint8, device=dev)
    ctx.synth_fill(d_blk.data_ptr(), 0, blk)
    h_blk = d_blk[:blk].cpu().numpy().copy()
    src = h_blk.ctypes.data
    pool = ThreadPoolExecutor(T)

    def copy_range(addr, off, n):       # file bytes [off, off + n) -> addr; the file wraps around the block
        done = 0
        while done < n:
            k = min(n - done, blk - (off + done) % blk)
            C.memmove(addr + done, src + (off + done) % blk, k)
            done += k

    def reader(replay):
        filled = {}

        def read_into(addr, off, n):
            if n == 0:
                return
            if replay and filled.get(addr) == (off % blk, n) and not (off <= inject < off + n):
                return                   # pinned replay: the slot already holds these bytes
            if T == 1 or n < (4 << 20):
                copy_range(addr, off, n)
            else:                        # the producer: T threads, memmove outside the GIL
                piece = (n + T - 1) // T // 64 * 64 + 64
                jobs = [pool.submit(copy_range, addr + o, off + o, min(piece, n - o)) for o in range(0, n, piece)]
                for jb in jobs:
                    jb.result()
            filled[addr] = (off % blk, n)
            if off <= inject < off + n:
                C.memset(addr + (inject - off), ord("-"), 1)
                filled.pop(addr, None)
        return read_into

    # what the totals must be: the block's own histograms, times the repetitions, plus the last partial block
    reps, rem = divmod(file_len, blk)
    exp = torch.zeros(8 + LMAX * 264, dtype=torch.int64, device=dev)
    one = torch.zeros_like(exp)
    ctx.stats(d_blk.data_ptr(), blk, LMAX, one[8: 8 + LMAX * 256].data_ptr(), one[8 + LMAX * 256:].data_ptr(), one[:8].data_ptr())
    exp += one * reps
    if rem:
        ctx.stats(d_blk.data_ptr(), rem, LMAX, exp[8: 8 + LMAX * 256].data_ptr(), exp[8 + LMAX * 256:].data_ptr(), exp[:8].data_ptr())
    exp = exp.cpu().numpy()
    ctx.invalidate()

    def map_at(off, want):                # the file's bytes in place: the registered block, up to its end
        return src + off % blk, blk - off % blk

    def once(replay, mapped=False):
        read_into = reader(replay)
        hist = torch.zeros(8 + LMAX * 264, dtype=torch.int64, device=dev)
        sc, qh, bh = hist[:8], hist[8: 8 + LMAX * 256], hist[8 + LMAX * 256:]
        stats = (LMAX, qh.data_ptr(), bh.data_ptr(), sc.data_ptr())
        coll.barrier()
        t0 = time.perf_counter()
        sh = sharded.stream_shard(ctx, read_into, lo, hi, file_len, blk, stats=stats,     # fqh_shard_stream_run[_mapped] (a failure goes into the words)
                                  map_at=map_at if mapped else None)
        t_stream = time.perf_counter() - t0
        # ---- the one exchange: FQH_SHARD_STREAM_WORDS words of every rank (bytes of another rank's range, where a rank needs
        # them, come through its own read callback)
        words = coll.gather_words(sh.words())
        # ---- true-phase check + the gap in front of this rank + its first-error key (fqh_shard_stream_finish), then SUM and MIN
        t1 = time.perf_counter()
        rec, key = sharded.finish(ctx, read_into, file_len, words, rank, blk, stats=stats)
        t_finish = time.perf_counter() - t1
        slots = torch.zeros(world, dtype=torch.int64, device=dev)
        slots[rank] = rec
        both = torch.cat([slots, hist])
        coll.sum_dev(both)
        gkey = coll.min_key(key)
        tot = both.cpu().numpy()
        g_status, g_records, g_err_offset = sharded.outcome([int(x) for x in tot[:world]], gkey)
        coll.barrier()
        dt = time.perf_counter() - t0
        per = coll.objects({"seconds": dt, "stream_seconds": t_stream, "finish_seconds": t_finish, "bytes": hi - lo})
        dt = max(p["seconds"] for p in per)
        r = {"seconds": round(dt, 4), "gbs_aggregate": round(file_len / 1e9 / dt, 2),
             "gbs_per_rank": [round(p["bytes"] / 1e9 / p["stream_seconds"], 2) for p in per],
             "finish_seconds": [round(p["finish_seconds"], 4) for p in per]}
        return r, (g_status, int(g_records), int(g_err_offset), gkey), tot

    # The ring (3 pinned slots + their device twins) is created inside fqh_shard_stream_run.  A host that streams file after file
    # creates it once: FQH_OPT_KEEP_RING parks a destroyed ring's memory with the context and the next ring of the same geometry
    # takes it.  The probe ring below is timed by itself (what a one-shot caller pays on top) and then parked: no sub-run pins
    # memory inside its timed region.
    ctx.set_keep_ring(True)
    t_ring = time.perf_counter()
    probe = pkg.Stream(ctx, blk, 3, pkg.STREAM_STATS)
    probe.close()
    t_ring = time.perf_counter() - t_ring
    out = {"workload": "configs[4]: %.2f GiB in %d byte-range shard%s of %d B (cuts inside records), each streamed from host memory "
                       "through a 3 x %d MiB ring (a %d MiB record-aligned block replayed), phase-free; one all-gather of ten "
                       "words per rank, true-phase check, the record at every cut parsed by the rank it ends in, one SUM and one MIN"
                       % (file_len / 2**30, world, "" if world == 1 else "s", shard, blk >> 20, blk >> 20),
           "ranks": world, "bytes_per_gpu": shard, "comm": coll.via_text, "numa": coll.objects(numa),
           "ring_setup_seconds": [round(x, 4) for x in coll.objects(t_ring)],
           "ring_setup_note": "creating a ring of this size by itself, per rank — OUTSIDE every sub-run's seconds: the ring's memory is "
                              "created once per context (FQH_OPT_KEEP_RING) and every sub-run's ring is made of it"}
    if inject >= 0:
        r, (g_status, g_records, g_err_offset, gkey), tot = once(False)
        exp_err = (pkg.E_SEP, inject // RECLEN, inject // RECLEN * RECLEN)
        assert (g_status, g_records, g_err_offset) == exp_err, ((g_status, g_records, g_err_offset), exp_err)
        out["first_error"] = {"status": g_status, "n_records": g_records, "err_offset": g_err_offset,
                              "key_rank": (gkey >> 3) & 0xFF, "expected": list(exp_err)}
        ctx.set_keep_ring(False)
        pool.shutdown()
        return out
    registered = False
    for name in sub_runs:
        if name == "registered":
            t_reg = time.perf_counter()
            ctx.host_register(src, blk)
            t_reg = time.perf_counter() - t_reg
            registered = True
        r, (g_status, g_records, g_err_offset, gkey), tot = once(name == "pinned_replay", mapped=name == "registered")
        ok_hist = bool((tot[world:] == exp).all())
        assert g_status == pkg.OK, (name, g_status, g_records, g_err_offset)
        assert g_records == file_len // RECLEN, (name, g_records, file_len // RECLEN)
        assert ok_hist, name
        r["records"] = g_records
        r["records_per_s"] = round(g_records / r["seconds"], 1)
        r["check"] = {"records_expected": file_len // RECLEN, "first_error_key": None, "phases_ok": True, "histograms_ok": ok_hist}
        if name == "producer":
            r["producer"] = {"threads_per_rank": T, "host_dram_bytes_per_byte": 3,
                             "source": "pageable host memory; every slot of every pass is filled again "
                                       "(memmove outside the GIL), as in the N = 1 `stream` leg"}
        elif name == "registered":
            r["producer"] = {"threads_per_rank": 0, "host_dram_bytes_per_byte": 1, "register_seconds": round(t_reg, 4),
                             "source": "the pageable source block page-locked where it lies (fqh_host_register, outside the timed "
                                       "region) and DMA'd in place (fqh_shard_stream_run_mapped): no staging copy, no pinned "
                                       "data slots"}
        else:
            r["producer"] = {"threads_per_rank": 0, "host_dram_bytes_per_byte": 1,
                             "source": "none: one pinned block replayed, a slot that already holds its bytes is "
                                       "submitted as it is — link and kernels only, no host-side work"}
        out[name] = r
    if registered:
        ctx.host_unregister(src)
    ctx.set_keep_ring(False)
    pool.shutdown()
    return out


def sharded_stream_record(args, pkg, torch, dist, dev, ctx, coll, backend, via, gib_per_rank):
    """The `sharded_stream` object of the default line: the configs[4] leg at this world size AND — what `ratio_vs_n1` is a
    ratio of — the same function at world size 1, run by rank 0 alone on its GPU while the other ranks wait (nothing else uses
    the host's memory or the links meanwhile).  north_star's ">= 6x at 8 GPUs on the sharded host-streamed path" is
    producer.ratio_vs_n1."""
    world, rank = coll.world, coll.rank
    n1 = None
    if world > 1:
        if rank == 0:
            c1 = Coll(pkg, torch, dist, ctx, dev, 1, 0, backend, via, local=True)
            n1 = sharded_stream(args, pkg, torch, dev, ctx, c1, gib_per_rank)
            c1.close()
        coll.barrier()
    rec = sharded_stream(args, pkg, torch, dev, ctx, coll, gib_per_rank)
    if world == 1:
        n1 = rec
    if rank == 0:
        for name in SHARD_SUB_RUNS:
            rec[name]["n1_gbs"] = n1[name]["gbs_aggregate"]
            rec[name]["ratio_vs_n1"] = round(rec[name]["gbs_aggregate"] / n1[name]["gbs_aggregate"], 3)
        rec["n1"] = ("the same function (sharded_stream) at world size 1: %.2f GiB, run by rank 0 alone while the other ranks wait"
                     % (n1["bytes_per_gpu"] / 2**30)) if world > 1 else "this run"
        rec["gbs_aggregate"] = rec["producer"]["gbs_aggregate"]
        rec["ratio_vs_n1"] = rec["producer"]["ratio_vs_n1"]
    return rec


if __name__ == "__main__":
    main()
