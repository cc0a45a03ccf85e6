#!/usr/bin/env python3
"""print-contigs (linear segments) on one MI355X: goss_gpu_segments_build on two shapes of graph, k = 27.

 * `fragmented`: synthetic reads with substituted bases (the graph of tools/tips_probe.py), as built and after
   trim -C 1 + five prune-tips iterations;
 * `long`: error-free reads over the same genome: a handful of paths of millions of edges.

Per shape and per setting of GOSS_GPU_CONTIGS_WALK (1 = pointer doubling alone; 16, 64, 256 = a bounded walk of that many
pointers per lane, then doubling): one warm-up, --reps timed calls; the host clock around the call (it ends in a
stream synchronise), and beside it the HIP-event times of its four parts (link pass / ranking / figures / text) as
the call reports them.  One JSON line per record.

 * `composed` (fragmented shape as built only): the same table put together from what the library offered before --
   the emitted graph opened as an Object, batched node_ranks / rank / multiplicity with torch index ops,
   level-synchronous over all starts: one round of launches per path step.  It produces the figures of every taken
   path (not the text) and doubles as an independent check of the kernel's table.  On the other shapes the number of
   rounds is the longest path (10^5 .. 10^7): not run.

usage: python tools/contigs_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 3]
       [--shapes fragmented,cleaned,long] [--walks 1,16,64,256] [--no-composed] [--out f.jsonl]"""
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


def composed_table(obj, keys, K, max_rounds):
    """(first_rank, edges, min, max, s) of every taken path, in rank order, by batched queries; rounds"""
    import torch
    node_mask = (1 << (2 * K)) - 1

    def degree(nodes, incoming=False):
        b, e = obj.node_ranks(nodes, incoming=incoming)
        return b, e - b

    def revcomp(x, length):
        r = torch.zeros_like(x)
        for _ in range(length):
            r = (r << 2) | (3 - (x & 3))
            x = x >> 2
        return r

    frm = keys >> 2
    _, od = degree(frm)
    _, idg = degree(frm, incoming=True)
    beg = torch.nonzero(~((od == 1) & (idg == 1))).reshape(-1)
    del frm, od, idg
    cur = beg.clone()
    c0 = obj.multiplicity(cur).to(torch.int64) & 0xFFFFFFFF
    m = torch.ones_like(beg)
    mn, mx, s = c0.clone(), c0.clone(), c0.clone()
    idx = torch.arange(beg.numel(), device=keys.device)
    rounds = 0
    while idx.numel():
        rounds += 1
        if rounds > max_rounds:
            return None, rounds
        to = keys[cur[idx]] & node_mask
        b, o = degree(to)
        _, i = degree(to, incoming=True)
        go = (o == 1) & (i == 1)
        idx, b = idx[go], b[go]
        cur[idx] = b
        c = obj.multiplicity(b).to(torch.int64) & 0xFFFFFFFF
        m[idx] += 1
        mn[idx] = torch.minimum(mn[idx], c)
        mx[idx] = torch.maximum(mx[idx], c)
        s[idx] += c
    r, present = obj.rank(revcomp(keys[cur], K + 1))
    assert bool(present.all())
    taken = beg <= r
    return (beg[taken], m[taken], mn[taken], mx[taken], s[taken]), rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="fragmented,cleaned,long")
    ap.add_argument("--walks", default="1,16,64,256")
    ap.add_argument("--max-rounds", type=int, default=20000)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K, L = args.k, args.read_len
    if 2 * (K + 1) > 62:
        raise SystemExit("the composed path handles one-word edge keys: k <= 30")
    out = open(args.out, "a") if args.out else None
    shapes = args.shapes.split(",")
    walks = [int(w) for w in args.walks.split(",")]

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if out:
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

    def snapshot():
        kp, cp, n = ctx.result_ptrs()
        return gd.device_view(kp, n, torch.int64, dev).clone(), gd.device_view(cp, n, torch.int32, dev).clone(), n

    def load(keys, counts, n):
        ctx.reset()
        ctx.push_run(keys.data_ptr(), counts.data_ptr(), n)
        ctx.finish()
        torch.cuda.synchronize()

    def measure(shape, keys, counts, n):
        base = {"k": K, "shape": shape, "edges": n, "genome": args.genome, "reads": args.reads}
        load(keys, counts, n)
        table = None
        for w in walks:
            os.environ["GOSS_GPU_CONTIGS_WALK"] = str(w)
            ctx.segments_build()
            ctx.segments_release()                       # warm-up
            ts, infos = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                info = ctx.segments_build()
                ts.append(time.perf_counter() - t)
                infos.append(info)
                if table is None:
                    table = ctx.segments_table(0, info["segments"])
                ctx.segments_release()
            order = sorted(range(len(ts)), key=ts.__getitem__)
            med = order[len(ts) // 2]
            info = infos[med]
            emit(dict(base, op="segments_build", walk=w, ms_all=[round(x * 1e3, 3) for x in ts], ms=round(ts[med] * 1e3, 3),
                      edges_per_s=round(n / ts[med]), rounds=info["rounds"],
                      ms_link=round(info["ms_link"], 3), ms_rank=round(info["ms_rank"], 3),
                      ms_figures=round(info["ms_figures"], 3), ms_text=round(info["ms_text"], 3),
                      link_share=round(info["ms_link"] / (ts[med] * 1e3), 3),
                      text_bytes=info["text_bytes"],
                      text_gb_per_s=round(info["text_bytes"] / max(info["ms_text"], 1e-3) / 1e6, 2),
                      segments=info["segments"], paths=info["paths"], taken_paths=info["taken_paths"],
                      cycle_edges=info["cycle_edges"], longest_path=info["longest_path"]))
        os.environ.pop("GOSS_GPU_CONTIGS_WALK", None)
        return base, table

    if "fragmented" in shapes or "cleaned" in shapes:
        build(args.error)
        keys, counts, n = snapshot()
        if "fragmented" in shapes:
            base, table = measure("fragmented", keys, counts, n)
            if not args.no_composed:
                load(keys, counts, n)
                ctx.emit_device()
                obj = g.Object.from_context(ctx)
                torch.cuda.synchronize()
                t = time.perf_counter()
                got, rounds = composed_table(obj, keys, K, args.max_rounds)
                torch.cuda.synchronize()
                s = time.perf_counter() - t
                rec = dict(base, op="composed", ms=round(s * 1e3, 3), rounds=rounds, finished=got is not None)
                if got is not None:
                    same = all(bool(torch.equal(a.cpu(), torch.from_numpy(table[f].astype("int64"))))
                               for a, f in zip(got, ("first_rank", "edges", "min", "max", "s")))
                    rec.update(paths=int(got[0].numel()), table_equal=same)
                emit(rec)
                obj.close()
                if got is not None and not same:
                    raise SystemExit("the composed walk and the kernel disagree")
        if "cleaned" in shapes:
            load(keys, counts, n)
            ctx.select_counts(2, 0xFFFFFFFF)
            ctx.prune_tips(5)
            ck, cc, cn = snapshot()
            measure("cleaned", ck, cc, cn)
            del ck, cc
        del keys, counts
        torch.cuda.empty_cache()
    if "long" in shapes:
        build(0.0)
        keys, counts, n = snapshot()
        measure("long", keys, counts, n)
    ctx.close()


if __name__ == "__main__":
    main()
