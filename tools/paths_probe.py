#!/usr/bin/env python3
"""trim-paths and clip-links on one MI355X, over the graph of tools/tips_probe.py (synthetic reads with substituted
bases, build-graph k = 27 on the device; about 1.1e8 edges at the defaults), untrimmed and after trim-graph -C 1:

 * `fused`: goss_gpu_trim_paths / goss_gpu_clip_links on the finished graph, the whole pass between two HIP events and
   its phases (link, flag, gather, walk, compact) from the library's own events (goss_gpu_paths_timing); median of
   --reps runs after one warm-up; the share of the edges that are starts.
 * `composed`: the same removal bitmap put together from what the library offered before -- the emitted graph opened
   as an Object, batched node_ranks / rank / multiplicity with torch index ops, level-synchronous over the starts (one
   round of launches per path step), as tips_probe.py composes its baseline.  It doubles as an independent check: its
   survivor set must equal the kernel's.

One JSON line per record, appended to profiles/paths/paths_probe.jsonl (--out).  No number is fixed in advance.

usage: python tools/paths_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 5] [--out f.jsonl]
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

PHASES = ("link", "flag", "gather", "walk", "compact")


def composed_bitmap(obj, keys, K, cmd):
    """The removal bitmap of one pass over the Object's graph with batched queries and torch index ops.  keys: the sorted
    edges (int64, one word).  Returns (keep mask, {starts, hits, rounds})."""
    import torch
    n = keys.numel()
    node_mask = (1 << (2 * K)) - 1

    def out_range(nodes, incoming=False):
        b, e = obj.node_ranks(nodes, incoming=incoming)
        return b, e - b

    def revcomp(x, length):
        r = torch.zeros_like(x)
        for _ in range(length):
            r = (r << 2) | (3 - (x & 3))
            x = x >> 2
        return r

    def mult(ranks):
        return obj.multiplicity(ranks).to(torch.int64) & 0xFFFFFFFF

    if cmd == "trim":
        _, deg = out_range(keys >> 2, incoming=True)
        beg = torch.nonzero(deg == 0).reshape(-1)
    else:
        _, deg = out_range(keys >> 2)
        beg = torch.nonzero(deg >= 2).reshape(-1)
    cur = beg.clone()
    length = torch.ones_like(beg)
    active = torch.ones_like(beg, dtype=torch.bool)
    too_long = torch.zeros_like(active)
    rounds = 0
    while bool(active.any()):
        rounds += 1
        idx = torch.nonzero(active).reshape(-1)
        to = keys[cur[idx]] & node_mask
        b, od = out_range(to)
        _, idg = out_range(to, incoming=True)
        go = (od == 1) & (idg == 1) & (b != beg[idx])
        cur[idx] = torch.where(go, b, cur[idx])
        length[idx] += go.to(length.dtype)
        over = go & (length[idx] > 2 * K)
        too_long[idx] |= over
        active[idx] = go & ~over
    goes = ~too_long
    if cmd == "clip":
        def minor(member_first, size, c, through_rc):
            s = torch.zeros_like(c)
            for j in range(4):
                have = size > j
                r = torch.where(have, member_first + j, member_first)
                if through_rc:
                    r, _ = obj.rank(revcomp(keys[r], K + 1))
                s += torch.where(have, mult(r), torch.zeros_like(c))
            s &= 0xFFFFFFFF
            return (s != 0) & (3 * c < s)

        ob, on = out_range(keys[beg] >> 2)
        goes &= minor(ob, on, mult(beg), False)
        ib, inn = out_range(revcomp(keys[cur] & node_mask, K))
        goes &= minor(ib, inn, mult(cur), True)
    zap = torch.zeros(n, dtype=torch.bool, device=keys.device)
    at = beg[goes].clone()
    left = length[goes].clone()
    while at.numel():
        e = keys[at]
        zap[at] = True
        r, present = obj.rank(revcomp(e, K + 1))
        assert bool(present.all())
        zap[r] = True
        left -= 1
        on = left > 0
        b, _ = out_range(e[on] & node_mask)
        at, left = b, left[on]
    return ~zap, dict(starts=int(beg.numel()), hits=int(goes.sum()), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths", "paths_probe.jsonl"))
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

    bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.7))
    ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
    torch.cuda.synchronize()
    substitute(bases, args.error, dev)
    torch.cuda.synchronize()
    ctx.push_device(bases.data_ptr(), bases.numel())
    ctx.finish()
    del bases
    torch.cuda.empty_cache()

    for graph in ("untrimmed", "trimmed"):
        if graph == "trimmed":
            ctx.select_counts(2, 0xFFFFFFFF)
        kp, cp, n = ctx.result_ptrs()
        keys = gd.device_view(kp, n, torch.int64, dev).clone()
        counts = gd.device_view(cp, n, torch.int32, dev).clone()
        obj = None
        if not args.no_composed:
            ctx.emit_device()
            obj = g.Object.from_context(ctx)
        base = {"k": K, "graph": graph, "edges": n, "genome": args.genome, "reads": args.reads, "error": args.error}

        def load():
            ctx.reset()
            ctx.push_run(keys.data_ptr(), counts.data_ptr(), n)
            ctx.finish()
            torch.cuda.synchronize()

        for cmd in ("trim", "clip"):
            def fused():
                load()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rep = ctx.trim_paths() if cmd == "trim" else ctx.clip_links()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), ctx.paths_timing(), rep

            fused()                                    # warm-up
            runs = [fused() for _ in range(args.reps)]
            rep = runs[-1][2]
            emit(dict(base, op="fused", cmd=cmd, ms_all=[round(r[0], 3) for r in runs], ms=round(median([r[0] for r in runs]), 3),
                      phases_ms={p: round(median([r[1][p] for r in runs]), 3) for p in PHASES},
                      start_share=round(rep["candidates"] / n, 5), report=rep))
            if obj is not None:
                def composed():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    keep, crep = composed_bitmap(obj, keys, K, cmd)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1), keep, crep

                composed()
                cruns = [composed() for _ in range(args.reps)]
                _, keep, crep = cruns[-1]
                kp2, _, m = ctx.result_ptrs()
                same = bool(torch.equal(gd.device_view(kp2, m, torch.int64, dev), keys[keep]))
                med_c, med_f = median([r[0] for r in cruns]), median([r[0] for r in runs])
                emit(dict(base, op="composed", cmd=cmd, ms_all=[round(r[0], 3) for r in cruns], ms=round(med_c, 3), rounds=crep["rounds"],
                          starts=crep["starts"], hits=crep["hits"], survivors_equal=same, composed_over_fused=round(med_c / med_f, 2)))
                if not same or crep["starts"] != rep["candidates"]:
                    raise SystemExit("the composed pass and the kernel disagree")
        if obj is not None:
            obj.close()
        # (the next graph is made from this one: back to the whole list)
        load()
    ctx.close()


if __name__ == "__main__":
    main()
