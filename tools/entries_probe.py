#!/usr/bin/env python3
"""build-entry-edge-set on one MI355X: goss_gpu_entries_build on two shapes of graph, k = 27.

 * `fragmented`: synthetic reads with substituted bases (the 1.1 x 10^8-edge graph of tools/contigs_probe.py), as built;
 * `long`: error-free reads over the same genome: one path of 10^7 edges per strand.

Per shape: one warm-up, --reps timed calls of Context.entries_build; the host clock around the call (it ends in a
stream synchronise), and beside it the HIP-event times of its four parts (link pass / ranking / records / images) as
the call reports them.  One JSON line per record, appended to profiles/entries/entries_probe.jsonl.

 * `composed`: the same columns put together from what the library offered before -- Context.linear_segments (one
   path of every mirror pair, its figures from a sort by (path, position)), the table copied to the host side of torch,
   and the compaction there: the mirror starts by a search of the reverse complements of the end edges, the merge of the
   two halves, the numbering.  It needs the multiplicities of an edge and of its reverse complement to be equal, which
   holds for a graph as built.  It is timed without the images and doubles as an independent check of the kernel's
   columns (read back through an Object: select / multiplicity / length / end_rank over all entries).

usage: python tools/entries_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 3]
       [--shapes fragmented,long] [--no-composed] [--out profiles/entries/entries_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gossamer_amd as g  # noqa: E402
from gossamer_amd import dist as gd  # noqa: E402
from tips_probe import substitute  # noqa: E402


def composed_columns(ctx, keys, K, dev):
    """(starts, cnt, len, ends) of every entry, in rank order, from the linear segments and torch"""
    import torch
    table, _, _ = ctx.linear_segments()
    col = lambda f: torch.from_numpy(table[f].astype("int64")).to(dev)
    first, end, m, s = col("first_rank"), col("end_rank"), col("edges"), col("s")
    x = keys[end]
    rc = torch.zeros_like(x)
    for _ in range(K + 1):
        rc = (rc << 2) | (3 - (x & 3))
        x = x >> 2
    mirror = torch.searchsorted(keys, rc)
    other = mirror != first                              # (a path that is its own mirror image is one entry)
    starts = torch.cat([first, mirror[other]])
    partner = torch.cat([mirror, first[other]])
    length = torch.cat([m, m[other]])
    total = torch.cat([s, s[other]])
    order = torch.argsort(starts)
    starts, partner, length, total = starts[order], partner[order], length[order], total[order]
    cnt = (2 * total + length) // (2 * length)           # round half away from zero, exactly
    ends = torch.searchsorted(starts, partner)
    return starts, cnt, length, ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="fragmented,long")
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entries", "entries_probe.jsonl"))
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

    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.7))

    def build(error):
        bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
        ctx.reset()
        ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
        torch.cuda.synchronize()
        if error:
            substitute(bases, error, dev)
            torch.cuda.synchronize()
        ctx.push_device(bases.data_ptr(), bases.numel())
        ctx.finish()
        del bases
        torch.cuda.empty_cache()

    def measure(shape):
        kp, _, n = ctx.result_ptrs()
        keys = gd.device_view(kp, n, torch.int64, dev).clone()
        base = {"k": K, "shape": shape, "edges": n, "genome": args.genome, "reads": args.reads}
        ctx.entries_build()
        ctx.entries_release()                            # warm-up
        ts, infos = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            info = ctx.entries_build()
            ts.append(time.perf_counter() - t)
            infos.append(info)
            ctx.entries_release()
        order = sorted(range(len(ts)), key=ts.__getitem__)
        med = order[len(ts) // 2]
        info = infos[med]
        emit(dict(base, op="entries_build", ms_all=[round(x * 1e3, 3) for x in ts], ms=round(ts[med] * 1e3, 3),
                  edges_per_s=round(n / ts[med]), rounds=info["rounds"], walk=info["walk_steps"],
                  ms_link=round(info["ms_link"], 3), ms_rank=round(info["ms_rank"], 3),
                  ms_paths=round(info["ms_paths"], 3), ms_emit=round(info["ms_emit"], 3),
                  entries=info["entries"], cycle_edges=info["cycle_edges"], longest_path=info["longest_path"],
                  hist_size=info["hist_size"]))
        if args.no_composed:
            return
        composed_columns(ctx, keys, K, dev)              # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = composed_columns(ctx, keys, K, dev)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        ts.sort()
        ctx.entries_build()
        with g.Object.from_context(ctx) as obj:
            ctx.entries_release()
            ranks = torch.arange(obj.count, dtype=torch.int64, device=dev)
            want = (torch.searchsorted(keys, obj.select(ranks).reshape(-1)), obj.multiplicity(ranks).to(torch.int64) & 0xFFFFFFFF,
                    obj.length(ranks).to(torch.int64) & 0xFFFFFFFF, obj.end_rank(ranks))
        same = all(a.numel() == b.numel() and bool(torch.equal(a, b)) for a, b in zip(got, want))
        emit(dict(base, op="composed", ms_all=[round(x * 1e3, 3) for x in ts], ms=round(ts[len(ts) // 2] * 1e3, 3),
                  entries=int(got[0].numel()), columns_equal=same))
        if not same:
            raise SystemExit("the composed columns and the kernel's disagree")

    shapes = args.shapes.split(",")
    if "fragmented" in shapes:
        build(args.error)
        measure("fragmented")
    if "long" in shapes:
        build(0.0)
        measure("long")
    ctx.close()


if __name__ == "__main__":
    main()
