#!/usr/bin/env python3
"""trim-relative and merge-graph-with-reference on one MI355X, over the graph of tools/tips_probe.py (synthetic reads with
substituted bases, build-graph k = 27 on the device; about 1.1e8 edges at the defaults):

 * `fused`: goss_gpu_trim_relative at rel = 0.02 and 0.25 and goss_gpu_recount_from against a reference that holds
   every other edge, the whole call between two HIP events and its phases (judge, mirror, compact; for the recount
   lookup and compact) from the library's own events (goss_gpu_relative_timing); median of --reps runs after one
   warm-up; the share of the edges below their threshold and the share removed.
 * `composed`: the same result put together from what the library offered before.  trim-relative: the emitted graph
   opened as an Object, select / node_ranks / multiplicity over every rank, the group sums from a torch prefix sum,
   the comparison in float64, rank of the reverse complements of the edges below.  The merge: Object.rank and
   Object.lookup of every edge in the reference, then a rebuild of the survivors through push_run + finish.  Each
   doubles as an independent check: its survivors (and, for the merge, their counts) must equal the kernel's.
 * `floor`: one streaming pass over the keys and counts (12 bytes an edge) at the 6.29 TB/s a float4 copy reaches on
   this part -- what a pass that only reads the list once cannot beat.  Computed, not measured.

One JSON line per record, appended to profiles/relative/relative_probe.jsonl (--out).  No number is fixed in advance.

usage: python tools/relative_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 5] [--out f.jsonl]
       [--no-composed]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gossamer_amd as g  # noqa: E402
from gossamer_amd import dist as gd  # noqa: E402
from tips_probe import substitute  # noqa: E402

PHASES = ("judge", "mirror", "compact")
HBM_COPY_BYTES_PER_S = 6.29e12


def composed_trim(obj, n, K, rel, dev):
    """keep mask of trim-relative over the Object's graph with batched queries and torch ops; (mask, edges below)"""
    import torch
    ranks = torch.arange(n, dtype=torch.int64, device=dev)
    e = obj.select(ranks)
    c = obj.multiplicity(ranks).to(torch.int64) & 0xFFFFFFFF
    b, end = obj.node_ranks(e >> 2)
    b, end = b.to(torch.int64), end.to(torch.int64)
    pre = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(c, 0, out=pre[1:])
    total = pre[end] - pre[b]
    below = ((end - b) >= 2) & (c.to(torch.float64) < total.to(torch.float64) * rel)
    x = e[below]
    r = torch.zeros_like(x)
    for _ in range(K + 1):
        r = (r << 2) | (3 - (x & 3))
        x = x >> 2
    q, present = obj.rank(r)
    assert bool(present.to(torch.bool).all())
    zap = below.clone()
    zap[q.to(torch.int64)] = True
    return ~zap, int(below.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative", "relative_probe.jsonl"))
    ap.add_argument("--no-composed", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K, L = args.k, args.read_len
    if 2 * (K + 1) > 62:
        raise SystemExit("the composed path handles one-word edge keys: k <= 30")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    def median(v):
        return sorted(v)[len(v) // 2]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), res

    bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.5))
    ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
    torch.cuda.synchronize()
    substitute(bases, args.error, dev)
    torch.cuda.synchronize()
    ctx.push_device(bases.data_ptr(), bases.numel())
    ctx.finish()
    del bases
    torch.cuda.empty_cache()

    kp, cp, n = ctx.result_ptrs()
    keys = gd.device_view(kp, n, torch.int64, dev).clone()
    counts = gd.device_view(cp, n, torch.int32, dev).clone()
    base = {"k": K, "edges": n, "genome": args.genome, "reads": args.reads, "error": args.error}
    floor_ms = n * 12 / HBM_COPY_BYTES_PER_S * 1e3
    emit(dict(base, op="floor", bytes=n * 12, bytes_per_s=HBM_COPY_BYTES_PER_S, ms=round(floor_ms, 4), measured=False))
    obj = None
    if not args.no_composed:
        ctx.emit_device()
        obj = g.Object.from_context(ctx)

    def load():
        ctx.reset()
        ctx.push_run(keys.data_ptr(), counts.data_ptr(), n)
        ctx.finish()
        torch.cuda.synchronize()

    def survivors():
        kp2, cp2, m = ctx.result_ptrs()
        return gd.device_view(kp2, m, torch.int64, dev), gd.device_view(cp2, m, torch.int32, dev)

    # ---- trim-relative
    for rel in (0.02, 0.25):
        def fused():
            load()
            ms, rep = timed(lambda: ctx.trim_relative(rel))
            return ms, ctx.relative_timing(), rep

        fused()                                        # warm-up
        runs = [fused() for _ in range(args.reps)]
        rep = runs[-1][2]
        med_f = median([r[0] for r in runs])
        emit(dict(base, op="fused", cmd="trim-relative", rel=rel, ms_all=[round(r[0], 3) for r in runs], ms=round(med_f, 3),
                  phases_ms={p: round(median([r[1][p] for r in runs]), 3) for p in PHASES},
                  phases_ms_all={p: [round(r[1][p], 3) for r in runs] for p in PHASES},
                  below_share=round(rep["below"] / n, 6), removed_share=round((rep["edges_before"] - rep["edges_after"]) / n, 6),
                  over_floor=round(med_f / floor_ms, 2), report=rep))
        if obj is not None:
            timed(lambda: composed_trim(obj, n, K, rel, dev))
            cruns = [timed(lambda: composed_trim(obj, n, K, rel, dev)) for _ in range(args.reps)]
            keep, below = cruns[-1][1]
            same = bool(torch.equal(survivors()[0], keys[keep])) and bool(torch.equal(survivors()[1], counts[keep]))
            med_c = median([r[0] for r in cruns])
            emit(dict(base, op="composed", cmd="trim-relative", rel=rel, ms_all=[round(r[0], 3) for r in cruns], ms=round(med_c, 3),
                      below=below, survivors_equal=same, composed_over_fused=round(med_c / med_f, 2)))
            if not same or below != rep["below"]:
                raise SystemExit("the composed pass and the kernel disagree")
            del keep
    if obj is not None:
        obj.close()

    # ---- merge-graph-with-reference: the reference holds every other edge, with other multiplicities
    ref_keys = keys[::2].contiguous()
    ref_counts = (counts[::2] + 1).contiguous()
    nref = ref_keys.numel()
    rctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(nref * 64 + (2 << 30)))
    rctx.push_run(ref_keys.data_ptr(), ref_counts.data_ptr(), nref)
    rctx.finish()
    rctx.emit_device()
    ref = g.Object.from_context(rctx)
    rctx.close()

    def fused_merge():
        load()
        ms, rep = timed(lambda: ctx.recount_from(ref))
        return ms, ctx.relative_timing(), rep

    fused_merge()
    runs = [fused_merge() for _ in range(args.reps)]
    rep = runs[-1][2]
    med_f = median([r[0] for r in runs])
    got_keys, got_counts = (t.clone() for t in survivors())
    emit(dict(base, op="fused", cmd="merge-graph-with-reference", ref_edges=nref, ms_all=[round(r[0], 3) for r in runs], ms=round(med_f, 3),
              phases_ms={"lookup": round(median([r[1]["judge"] for r in runs]), 3), "compact": round(median([r[1]["compact"] for r in runs]), 3)},
              kept_share=round(rep["edges_after"] / n, 6), over_floor=round(med_f / floor_ms, 2), report=rep))
    if not args.no_composed:
        def composed_merge():
            _, present = ref.rank(keys)
            keep = present.to(torch.bool)
            k2 = keys[keep].contiguous()
            c2 = ref.lookup(k2).contiguous()
            ctx.reset()
            ctx.push_run(k2.data_ptr(), c2.data_ptr(), k2.numel())
            ctx.finish()
            return k2.numel()

        timed(composed_merge)
        cruns = [timed(composed_merge) for _ in range(args.reps)]
        same = bool(torch.equal(survivors()[0], got_keys)) and bool(torch.equal(survivors()[1], got_counts))
        med_c = median([r[0] for r in cruns])
        emit(dict(base, op="composed", cmd="merge-graph-with-reference", ms_all=[round(r[0], 3) for r in cruns], ms=round(med_c, 3),
                  survivors_equal=same, composed_over_fused=round(med_c / med_f, 2)))
        if not same or cruns[-1][1] != rep["edges_after"]:
            raise SystemExit("the composed merge and the kernel disagree")
    ref.close()
    ctx.close()


if __name__ == "__main__":
    main()
