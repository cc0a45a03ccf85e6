#!/usr/bin/env python3
"""count-components on one MI355X: the goss_gpu_components_* entry points on two shapes of graph, k = 27.

 * `fragmented`: synthetic reads with substituted bases (the 1.1 x 10^8-edge graph of tools/contigs_probe.py), as built;
 * `long`: error-free reads over the same genome: one path of 10^7 edges per strand.

Per shape, one warm-up and --reps timed calls each of
 * `build_all`:    Context.components() over every edge,
 * `mark`:         Context marks from a tenth of the reads (goss_gpu_components_mark_device),
 * `build_marked`: Context.components(marked=True) over those marks,
 * `keep`:         Context.keep_component(start of the first component), once, on the graph as built;
the host clock around the call (it ends in a stream synchronise) and beside it the HIP-event times of the call's
parts as it reports them.  One JSON line per record, appended to profiles/components/components_probe.jsonl.

 * `composed`: the same labels put together from what the library offered before -- the graph emitted and opened as an
   Object, Object.node_ranks of every to-node and Object.rank of every reverse complement, the answers pulled to the
   host, and a host union-find there (scipy.sparse.csgraph.connected_components over the same three hooks per edge).
   It doubles as an independent check of the kernel's labels.

usage: python tools/components_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 3]
       [--shapes fragmented,long] [--no-composed] [--out profiles/components/components_probe.jsonl]"""
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


def composed_labels(obj, keys, K):
    """np.uint32 component index per edge, numbered by smallest rank, from Object queries and a host union-find"""
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = keys.numel()
    x = keys.clone()
    rc = torch.zeros_like(x)
    for _ in range(K + 1):
        rc = (rc << 2) | (3 - (x & 3))
        x = x >> 2
    rcr, _ = obj.rank(rc)
    begin, end = obj.node_ranks(keys & ((1 << (2 * K)) - 1))
    frm = (keys >> 2).cpu().numpy()
    rcr, begin, end = rcr.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy()
    idx = np.arange(n, dtype=np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = frm[1:] != frm[:-1]
    group = np.maximum.accumulate(np.where(first, idx, 0))           # the first edge of every from-group
    has_out = end > begin
    rows = np.concatenate([idx, idx, idx[has_out]])
    cols = np.concatenate([group, rcr[group[rcr]], begin[has_out]])
    adj = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n, n))
    _, lab = connected_components(adj, directed=False)
    _, start = np.unique(lab, return_index=True)
    number = np.empty(start.size, dtype=np.uint32)
    number[np.argsort(start)] = np.arange(start.size, dtype=np.uint32)
    return number[lab]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components", "components_probe.jsonl"))
    args = ap.parse_args()
    import numpy as np
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
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.6))
    mark_dev = ctx._L.goss_gpu_components_mark_device
    mark_dev.argtypes = [g.binding.C.c_void_p, g.binding.C.c_void_p, g.binding.C.c_uint64, g.binding.C.POINTER(g.binding.MarkInfo)]

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
        part = bases[:(args.reads // 10) * (L + 1)].clone()
        del bases
        torch.cuda.empty_cache()
        return part

    def timed(fn, after=None):
        fn()
        if after:
            after()
        ts, infos = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            infos.append(fn())
            ts.append(time.perf_counter() - t)
            if after:
                after()
        order = sorted(range(len(ts)), key=ts.__getitem__)
        med = order[len(ts) // 2]
        return [round(x * 1e3, 3) for x in ts], round(ts[med] * 1e3, 3), infos[med]

    def mark(part):
        inf = g.binding.MarkInfo()
        ctx._check(mark_dev(ctx._h, part.data_ptr(), part.numel(), g.binding.C.byref(inf)))
        return {name: getattr(inf, name) for name, _ in g.binding.MARK_INFO_FIELDS}

    def measure(shape, part):
        kp, _, n = ctx.result_ptrs()
        base = {"k": K, "shape": shape, "edges": n, "genome": args.genome, "reads": args.reads}

        def figures(info):
            return dict(components=info["components"], marked_edges=info["marked_edges"], largest=info["largest"], launches=info["launches"],
                        ms_link=round(info["ms_link"], 3), ms_label=round(info["ms_label"], 3), ms_figures=round(info["ms_figures"], 3))

        ms_all, ms, (info, table) = timed(lambda: ctx.components(), ctx.components_release)
        emit(dict(base, op="build_all", ms_all=ms_all, ms=ms, edges_per_s=round(n / (ms * 1e-3)), **figures(info)))
        build_all_ms = ms
        ms_all, ms, minfo = timed(lambda: mark(part), ctx.components_release)
        emit(dict(base, op="mark", ms_all=ms_all, ms=ms, bytes=part.numel(), windows=minfo["windows"], hits=minfo["hits"],
                  marked_total=minfo["marked_total"], ms_kernels=round(minfo["ms"], 3)))
        mark(part)
        ms_all, ms, (info, _) = timed(lambda: ctx.components(marked=True))
        emit(dict(base, op="build_marked", ms_all=ms_all, ms=ms, **figures(info)))
        ctx.components_release()
        _, table = ctx.components()
        labels = ctx.component_labels()
        ctx.components_release()
        if not args.no_composed:
            keys = gd.device_view(kp, n, torch.int64, dev).clone()
            ctx.emit()
            with g.Object.from_context(ctx) as obj:
                torch.cuda.synchronize()
                t = time.perf_counter()
                got = composed_labels(obj, keys, K)
                dt = time.perf_counter() - t
            same = bool(np.array_equal(got, labels))
            emit(dict(base, op="composed", ms=round(dt * 1e3, 3), components=int(got.max()) + 1 if n else 0, labels_equal=same,
                      ratio_to_build_all=round(dt * 1e3 / build_all_ms, 1)))
            if not same:
                raise SystemExit("the composed labels and the kernel's disagree")
            return None
        return int(table[0]["start"]) if len(table) else None

    def keep(shape, start):
        n = ctx.result_ptrs()[2]
        torch.cuda.synchronize()
        t = time.perf_counter()
        kept = ctx.keep_component(start)
        dt = time.perf_counter() - t
        emit({"k": K, "shape": shape, "edges": n, "op": "keep", "ms": round(dt * 1e3, 3), "kept": kept})

    for shape, error in (("fragmented", args.error), ("long", 0.0)):
        if shape not in args.shapes.split(","):
            continue
        part = build(error)
        start = measure(shape, part)
        if start is None:                                 # (the composed path emitted the graph: build it again)
            del part
            part = build(error)
            _, table = ctx.components()
            start = int(table[0]["start"])
        keep(shape, start)
        del part
    ctx.close()


if __name__ == "__main__":
    main()
