"""Times fqh_align_scores (the per-record Smith-Waterman-Gotoh score against the adapter, examples/alignment_count.rs) on
three HBM-resident inputs and prints one JSON line per input:
  synth16    the 16 GiB BASELINE.json configs[1]-shaped synthetic set (fqh_synth_fill, 150 bp reads)
  ragged     reads of 36..150 bp, uniformly mixed
  kbp5       5 kbp reads
Before timing, a sampled sub-range of records is checked bit-exact against tests/align_model.py.  `ms` is the median of
--steps timed calls (HIP events on the context's stream, --warmup calls excluded); `cells` = sum over records of
len(seq()) * len(query); `frac_valu_bound` = the time the kernel's VALU instructions (per column, from the ISA:
VALU_PER_COLUMN below) need at the VALU issue peak (CUs x 4 SIMDs x 32 lanes x clock) / `ms`.

    python tools/bench_align.py [--steps 10] [--warmup 2] [--bytes N] [--only synth16,ragged,kbp5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# VALU instructions in the column loop of k_align<ROWS> (gfx950 ISA, hipcc -O3)
VALU_PER_COLUMN = {16: 141, 32: 277, 64: 549}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=16 << 30, help="size of the synthetic set")
    ap.add_argument("--other-bytes", type=int, default=1 << 30, help="size of the ragged and 5 kbp inputs")
    ap.add_argument("--only", default="synth16,ragged,kbp5")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--sample", type=int, default=3000, help="records checked against the model before timing")
    a = ap.parse_args()

    import torch
    import __graft_entry__ as g
    import align_model as am

    pkg = g.load_package()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ctx = pkg.Ctx(0, stream=stream.cuda_stream)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    peak = n_cu * 4 * 32 * a.clock_ghz * 1e9
    query = am.ADAPTER
    rows = 16 if len(query) <= 16 else 32 if len(query) <= 32 else 64
    P = am.EXAMPLE

    def tiled(block, nbytes):
        reps = max(1, nbytes // len(block))
        host = np.frombuffer(block, dtype=np.uint8)
        d = torch.empty(reps * len(block) + 64, dtype=torch.uint8, device=dev)
        blk = torch.from_numpy(host.copy()).to(dev)
        d[: reps * len(block)].view(reps, len(block)).copy_(blk.expand(reps, len(block)))
        return d, reps * len(block)

    def record_block(rng, lens):
        out = []
        for i, L in enumerate(lens):
            seq = bytes(rng.choice(list(b"ACGT"), int(L)).astype(np.uint8))
            out.append(b"@r%d\n" % i + seq + b"\n+\n" + b"I" * int(L) + b"\n")
        return b"".join(out)

    def run(name, d, size, truncated_ok):
        s, _, _ = ctx.scan(d.data_ptr(), size, True)
        assert s.parse_status == 0 or (truncated_ok and s.parse_status == pkg.E_TRUNCATED), s.parse_status
        n = s.n_records
        idx = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
        ctx.index_records(idx.data_ptr(), n)
        rowsv = idx.view(torch.int64).view(n, 3)
        hs = rowsv[:, 1].contiguous().view(torch.int32).view(n, 2).to(torch.int64)
        sl = hs[:, 1] - hs[:, 0] - 1
        total_len = int(sl.sum())        # no '\r' in these inputs
        score = torch.zeros(n, dtype=torch.int32, device=dev)
        end = torch.zeros(n, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(c=None):
            ctx.align_scores(d.data_ptr(), size, idx.data_ptr(), n, query, P["match"], P["mismatch"], P["gap_open"],
                             P["gap_extend"], P["threshold"], score.data_ptr(), end.data_ptr(), None,
                             c.data_ptr() if c is not None else None)

        # check a sub-range (its middle) and the last records against the model
        call(count)
        torch.cuda.synchronize()
        k = a.sample if name != "kbp5" else max(1, a.sample // 15)   # the model's cost grows with the read length
        lo = max(0, n // 2 - k // 2)
        sel = np.unique(np.concatenate([np.arange(lo, min(n, lo + k)), np.arange(max(0, n - 20), n)]))
        st = rowsv[torch.from_numpy(sel).to(dev), 0].cpu().numpy()
        hsel = hs[torch.from_numpy(sel).to(dev)].cpu().numpy()
        first = st + hsel[:, 0] + 1
        ln = hsel[:, 1] - hsel[:, 0] - 1
        span_lo, span_hi = int(first.min()), int((first + ln).max())
        window = d[span_lo:span_hi].cpu().numpy().tobytes()
        seqs = [window[int(f) - span_lo: int(f) - span_lo + int(L)] for f, L in zip(first, ln)]
        exp_s, exp_e = am.align_scores(seqs, query, P["match"], P["mismatch"], P["gap_open"], P["gap_extend"])
        ssel = torch.from_numpy(sel).to(dev)
        ok = np.array_equal(score[ssel].cpu().numpy().astype(np.int64), exp_s) and \
            np.array_equal(end[ssel].cpu().numpy().view(np.uint32), exp_e)
        if not ok:
            raise SystemExit("%s: GPU scores differ from the model on the sampled records" % name)
        hits = int(count.cpu()[0])
        assert hits == int((score > P["threshold"]).sum().cpu())
        for _ in range(a.warmup):
            call()
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        cells = total_len * len(query)
        bound_ms = total_len * VALU_PER_COLUMN[rows] / peak * 1e3
        line = {"input": name, "bytes": size, "records": n, "mean_read_len": round(total_len / max(1, n), 2),
                "query_len": len(query), "rows": rows, "ms": round(ms, 3), "ms_min": round(min(times), 3),
                "ms_max": round(max(times), 3), "cells": cells, "gcups": round(cells / ms / 1e6, 1),
                "records_per_s": round(n / ms * 1e3, 1), "fastq_gb_per_s": round(size / ms / 1e6, 1),
                "hits": hits, "valu_bound_ms": round(bound_ms, 3), "frac_valu_bound": round(bound_ms / ms, 3),
                "checked_records": int(len(sel)), "params": P}
        print(json.dumps(line), flush=True)

    only = set(a.only.split(","))
    if "synth16" in only:
        d = torch.empty(a.bytes + 64, dtype=torch.uint8, device=dev)
        ctx.synth_fill(d.data_ptr(), 0, a.bytes)
        run("synth16", d, a.bytes, True)
        del d
        torch.cuda.empty_cache()
    rng = np.random.default_rng(7)
    if "ragged" in only:
        d, size = tiled(record_block(rng, rng.integers(36, 151, 20000)), a.other_bytes)
        run("ragged", d, size, False)
        del d
        torch.cuda.empty_cache()
    if "kbp5" in only:
        d, size = tiled(record_block(rng, [5000] * 200), a.other_bytes)
        run("kbp5", d, size, False)
    ctx.close()


if __name__ == "__main__":
    main()
