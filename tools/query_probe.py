#!/usr/bin/env python3
"""Query throughput on one MI355X: a graph built on the device from goss_gpu_synth_reads (k = 27 over a 100 Mbp genome
by default), opened with goss_gpu_object_open_emitted, then batched queries against it -- lookup of 10^8 edges (half
present, drawn by select, half random) in random and in sorted order, and rank, select, multiplicity and node ranks
on their own.  One JSON line per operation: queries/s, object bytes, order.

usage: python tools/query_probe.py [--k 27] [--genome 100000000] [--reads 20000000] [--queries 100000000] [--reps 3]
Times are host clocks around the calls, each of which ends in a synchronise of the object's stream; one warm-up call
of every operation precedes the timed ones."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gossamer_amd as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    k, L = args.k, args.read_len
    if 2 * (k + 1) > 62:
        raise SystemExit("the probe draws one-word edge keys: k <= 30")

    t0 = time.perf_counter()
    bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
    free_b, _ = torch.cuda.mem_get_info(dev)
    with g.Context(k, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.85)) as ctx:
        ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
        ctx.push_device(bases.data_ptr(), bases.numel())
        ctx.finish()
        ctx.emit_device()
        obj = g.Object.from_context(ctx)
    del bases
    torch.cuda.empty_cache()
    build_s = time.perf_counter() - t0
    info = obj.info()
    n = args.queries
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    half = n // 2
    ranks = torch.randint(0, info["count"], (n,), device=dev, generator=gen)
    present = obj.select(ranks[:half])
    rand = torch.randint(0, 4 ** (k + 1), (n - half,), device=dev, generator=gen)
    keys = torch.cat([present.reshape(-1), rand])[torch.randperm(n, device=dev, generator=gen)]
    skeys, _ = torch.sort(keys)
    nodes = torch.bitwise_right_shift(keys, 2)
    torch.cuda.synchronize()

    base = {"k": k, "edges": info["count"], "object_bytes": info["resident_bytes"], "D": info["D"],
            "genome": args.genome, "reads": args.reads, "build_s": round(build_s, 2)}
    out = open(args.out, "a") if args.out else None

    def timed(op, order, f, queries):
        f()                                        # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t)
        ms = sorted(ts)[len(ts) // 2] * 1e3
        rec = dict(base, op=op, order=order, queries=queries, ms=round(ms, 3), queries_per_s=round(queries / ms * 1e3),
                   ms_all=[round(x * 1e3, 3) for x in ts])
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    timed("lookup", "random", lambda: obj.lookup(keys), n)
    timed("lookup", "sorted", lambda: obj.lookup(skeys), n)

    def sort_then_lookup():                        # (c): sorting first, its own cost and the scatter back included
        s, perm = torch.sort(keys)
        c = obj.lookup(s)
        res = torch.empty_like(c)
        res[perm] = c
        return res
    timed("lookup+sort", "random", sort_then_lookup, n)
    timed("rank", "random", lambda: obj.rank(keys), n)
    timed("select", "random", lambda: obj.select(ranks), n)
    timed("multiplicity", "random", lambda: obj.multiplicity(ranks), n)
    timed("node_ranks", "random", lambda: obj.node_ranks(nodes), n)
    # the answers of the orders agree
    a = obj.lookup(keys)
    s, perm = torch.sort(keys)
    b = torch.empty_like(a)
    b[perm] = obj.lookup(s)
    assert torch.equal(a, b)
    hit = int((a != 0).sum())
    print(json.dumps(dict(base, op="check", present=hit, queries=n)), flush=True)
    obj.close()


if __name__ == "__main__":
    main()
