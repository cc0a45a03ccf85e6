#!/usr/bin/env python3
"""build-subgraph on one MI355X: goss_gpu_components_grow / _keep_marked on the 1.1 x 10^8-edge graph of
tools/components_probe.py (synthetic reads with substituted bases, k = 27) under the marks of a tenth of its reads
(3 x 10^7 read bytes).

Per mode (nodes, linear paths) and radius (1, 4, 16), one warm-up and --reps timed calls of Context.grow_marks on
freshly taken marks: the host clock around the call (it ends in a stream synchronise) and beside it the HIP-event
times of its parts as it reports them -- the link pass, the segment labels, the passes -- with the passes' time per
pass, what every pass added and the launches.  Then `keep_marked`, once, on the marks of radius 4.

 * `composed`: the node-mode growth of radius 16 put together from what the library offered before -- the graph emitted
   and opened as an Object, Object.node_ranks of every to-node and Object.rank of every reverse complement, the answers
   pulled to the host and the passes run there over index arrays (numpy).  Its first 1 and 4 passes are the smaller
   radii.  It doubles as an independent check of the kernels' marks and per-pass figures.

One JSON line per record, appended to profiles/subgraph/subgraph_probe.jsonl.

usage: python tools/subgraph_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 3]
       [--radii 1,4,16] [--no-composed] [--out profiles/subgraph/subgraph_probe.jsonl]"""
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


def composed_grow(obj, keys, K, marked, radius):
    """(marks after the last pass, [edges added per pass], seconds of the queries, [seconds per pass]): node mode"""
    import numpy as np
    import torch
    t0 = time.perf_counter()
    x = keys.clone()
    rc = torch.zeros_like(x)
    for _ in range(K + 1):
        rc = (rc << 2) | (3 - (x & 3))
        x = x >> 2
    rcr, _ = obj.rank(rc)
    begin, end = obj.node_ranks(keys & ((1 << (2 * K)) - 1))
    rcr, begin, end = rcr.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy()
    t_queries = time.perf_counter() - t0
    I = marked.copy()
    I[rcr[np.flatnonzero(marked)]] = True
    P = np.flatnonzero(I)
    added, t_pass = [], []
    for _ in range(radius):
        t0 = time.perf_counter()
        found = []
        for backwards in (False, True):
            at = rcr[P] if backwards else P
            b, e = begin[at], end[at]
            for j in range(4):
                t = (b + j)[b + j < e]
                found.append(rcr[t] if backwards else t)
        F = np.unique(np.concatenate(found))
        F = F[~I[F]]
        I[F] = True
        P = F
        added.append(int(F.size))
        t_pass.append(time.perf_counter() - t0)
    return I, added, t_queries, t_pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--radii", default="1,4,16")
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph", "subgraph_probe.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    K, L = args.k, args.read_len
    radii = [int(r) for r in args.radii.split(",")]
    if 2 * (K + 1) > 62:
        raise SystemExit("the composed path handles one-word edge keys: k <= 30")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.6))
    mark_dev = ctx._L.goss_gpu_components_mark_device
    mark_dev.argtypes = [g.binding.C.c_void_p, g.binding.C.c_void_p, g.binding.C.c_uint64, g.binding.C.POINTER(g.binding.MarkInfo)]

    def build():
        bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
        ctx.reset()
        ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
        torch.cuda.synchronize()
        substitute(bases, args.error, dev)
        torch.cuda.synchronize()
        ctx.push_device(bases.data_ptr(), bases.numel())
        ctx.finish()
        part = bases[:(args.reads // 10) * (L + 1)].clone()
        del bases
        torch.cuda.empty_cache()
        return part

    def mark(part):
        inf = g.binding.MarkInfo()
        ctx._check(mark_dev(ctx._h, part.data_ptr(), part.numel(), g.binding.C.byref(inf)))
        return inf.marked_total

    part = build()
    kp, _, n = ctx.result_ptrs()
    base = {"k": K, "edges": n, "genome": args.genome, "reads": args.reads, "mark_bytes": part.numel()}
    node_marks = node_added = None
    for linear in (False, True):
        for radius in radii:
            ts, infos = [], []
            for rep in range(args.reps + 1):                # (the first is the warm-up)
                ctx.components_release()
                forward = mark(part)
                torch.cuda.synchronize()
                t = time.perf_counter()
                info, added = ctx.grow_marks(radius, linear_paths=linear)
                dt = time.perf_counter() - t
                if rep:
                    ts.append(dt)
                    infos.append((info, added))
            order = sorted(range(len(ts)), key=ts.__getitem__)
            info, added = infos[order[len(ts) // 2]]
            ms = round(ts[order[len(ts) // 2]] * 1e3, 3)
            emit(dict(base, op="grow", mode="linear-paths" if linear else "nodes", radius=radius, ms_all=[round(x * 1e3, 3) for x in ts], ms=ms,
                      marked_forward=forward, mirrored=info["mirrored"], marked_total=info["marked_total"], passes_run=info["passes_run"],
                      launches=info["launches"], ms_link=round(info["ms_link"], 3), ms_label=round(info["ms_label"], 3),
                      ms_grow=round(info["ms_grow"], 3), ms_per_pass=round(info["ms_grow"] / max(info["passes_run"], 1), 3), added=added))
            if not linear and radius == max(radii):
                node_marks, node_added = ctx.marks(), added
    ctx.components_release()
    if not args.no_composed:
        mark(part)
        marked = ctx.marks()
        ctx.components_release()
        keys = gd.device_view(kp, n, torch.int64, dev).clone()
        ctx.emit()
        with g.Object.from_context(ctx) as obj:
            torch.cuda.synchronize()
            t = time.perf_counter()
            got, added, t_queries, t_pass = composed_grow(obj, keys, K, marked, max(radii))
            dt = time.perf_counter() - t
        same = bool(np.array_equal(got, node_marks)) and added == node_added
        emit(dict(base, op="composed", mode="nodes", radius=max(radii), ms=round(dt * 1e3, 3), ms_queries=round(t_queries * 1e3, 3),
                  ms_passes=[round(x * 1e3, 3) for x in t_pass], added=added, marks_equal=same))
        if not same:
            raise SystemExit("the composed marks and the kernels' disagree")
        del keys
        part = build()
    mark(part)
    ctx.grow_marks(4 if 4 in radii else radii[0])
    torch.cuda.synchronize()
    t = time.perf_counter()
    kept = ctx.keep_marked()
    dt = time.perf_counter() - t
    emit(dict(base, op="keep_marked", ms=round(dt * 1e3, 3), kept=kept))
    ctx.close()


if __name__ == "__main__":
    main()
