#!/usr/bin/env python3
"""read links on one MI355X: the goss_gpu_read_links_* entry points on the 1.1 x 10^8-edge graph of the other graph
probes (k = 27, synthetic reads with substituted bases) and 10^6 of its reads of 150 bases, from the host.

 * `begin`: goss_gpu_read_links_begin, its parts by HIP events (link pass, list ranking, segment table);
 * per mode (carry, exact) and share of unique segments (all, half, none), one warm-up and --reps timed calls of
   goss_gpu_read_links_add_host over the whole batch and of goss_gpu_read_links_finish: the host clock around each call
   (both end in a stream synchronise; the add includes the copy of the batch from pageable host memory) and beside it
   the HIP-event times of the parts as the calls report them -- windows, scans (the recurrences; about nothing in
   exact mode), compaction (hits, links and the records), sort, reduce.  All --reps times are kept; `ms` is their median.
 * `device_ms` is the sum of those parts per call (HIP events only, no copy), median of the --reps with all of them kept;
 * the table of the batch in one piece is held against the table of the same batch cut in ten (equal rows asserted);
 * `composed`: the same table, both modes, every segment unique, over the first --baseline-reads reads, put together
   from what the library offered before: the resident keys, Object.node_ranks of every from- and to-node and of their
   in-degrees (starts, successors), pointer jumping to every edge's path head, the entry edge set opened as
   an Object and Object.rank of the heads (the segment of every edge), the windows' keys and Object.rank of them, and
   the aligner and the linker as a state machine in numpy (composed_table).  Equal rows asserted against the device's
   table of the same reads, whose add and finish are timed beside it.  The graph is emitted for it, so it runs last.

Not measured here: two-word keys, and reads longer than a tile at scale.  One JSON line per record, appended to
profiles/links/links_probe.jsonl.

usage: python tools/links_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--link-reads 1000000]
       [--baseline-reads 100000] [--reps 5] [--out profiles/links/links_probe.jsonl]"""
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


def composed_table(keys, rank, present, read_id, seg_of, out_from, K, carry):
    """The link table of one batch from per-window arrays, in numpy: keys (uint64, one-word edges), rank / present of
    every window among the edges, the read every window lies in, seg_of per edge (0xFFFFFFFF: none) and the out-degree
    of every edge's from-node.  Returns rows (a, b, count, gap_sum) ascending, every segment unique."""
    import numpy as np
    n = len(keys)
    if n == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    idx = np.arange(n, dtype=np.int64)
    r = np.where(present, rank, 0).astype(np.int64)
    fresh = np.where(present, seg_of[r].astype(np.int64), 0xFFFFFFFF)
    F = fresh != 0xFFFFFFFF
    if carry:
        node_mask = np.uint64((1 << (2 * K)) - 1)
        A = np.zeros(n, dtype=bool)
        A[1:] = (present[1:] & (read_id[1:] == read_id[:-1]) & ((keys[1:] >> np.uint64(2)) == (keys[:-1] & node_mask))
                 & (out_from[r[1:]] == 1))
        # a chain: a window without A and the windows with A behind it; the first window of a chain that a lookup
        # aligns gives its segment to every window of the chain from there on
        head = np.flatnonzero(~A)
        first = np.minimum.reduceat(np.where(F, idx, n), head)
        src = first[np.cumsum(~A) - 1]
        valid = src <= idx
        seg = np.where(valid, fresh[np.minimum(src, n - 1)], 0xFFFFFFFF)
    else:
        valid, seg = F, fresh
    nh = np.cumsum(~valid)                                   # (every segment unique: a hit is an aligned window)
    h = np.flatnonzero(valid)
    if len(h) == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    hs, hr, hn = seg[h], read_id[h], nh[h]
    first_of_read = np.ones(len(h), dtype=bool)
    first_of_read[1:] = hr[1:] != hr[:-1]
    reset = first_of_read.copy()
    reset[1:] |= hs[1:] != hs[:-1]
    emit = reset & ~first_of_read
    at = np.flatnonzero(reset)
    e = np.flatnonzero(emit)
    prev_reset = at[np.cumsum(reset)[e] - 2]                 # (the reset before the one at e: the same read's)
    gap = hn[e] - hn[prev_reset]
    key = (hs[e - 1].astype(np.uint64) << np.uint64(32)) | hs[e].astype(np.uint64)
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    gaps = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(gaps, inv, gap)
    return np.stack([uniq >> np.uint64(32), uniq & np.uint64(0xFFFFFFFF), cnt.astype(np.uint64), gaps.astype(np.uint64)], axis=1)


def composed_inputs(obj, eobj, keys, batch, K, dev):
    """the arrays composed_table takes, from Object queries and torch plumbing on the device, pulled to the host"""
    import numpy as np
    import torch
    L = K + 1
    n = keys.numel()
    node_mask = (1 << (2 * K)) - 1

    def degree(nodes, incoming=False):
        begin, end = obj.node_ranks(nodes, incoming=incoming)
        return begin, end - begin

    frm, to = keys >> 2, keys & node_mask
    _, out_from = degree(frm)
    _, in_from = degree(frm, incoming=True)
    nxt, out_to = degree(to)
    _, in_to = degree(to, incoming=True)
    start = ~((out_from == 1) & (in_from == 1))
    succ = (out_to == 1) & (in_to == 1)
    ptr = torch.arange(n, dtype=torch.int64, device=dev)
    e = torch.nonzero(succ).reshape(-1)
    ptr[nxt[e].to(torch.int64)] = e                          # (the only predecessor of an edge that is no start)
    for _ in range(48):
        nptr = ptr[ptr]
        if bool(torch.equal(nptr, ptr)):
            break
        ptr = nptr
    hrank, hpresent = eobj.rank(keys[ptr])
    seg_of = torch.where(start[ptr] & hpresent, hrank.to(torch.int64), torch.full_like(ptr, 0xFFFFFFFF))
    # the windows
    b = torch.from_numpy(np.frombuffer(batch, dtype=np.uint8).copy()).to(dev)
    code = torch.full((256,), 4, dtype=torch.int64, device=dev)
    for ch, c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
        code[ch] = c
    c = code[b.to(torch.int64)]
    bad = torch.cumsum((c == 4).to(torch.int64), 0)
    m = b.numel() - L + 1
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), bad[:m - 1]])
    ok = (bad[L - 1:] - before) == 0
    wkey = torch.zeros(m, dtype=torch.int64, device=dev)
    for j in range(L):
        wkey = (wkey << 2) | (c[j:j + m] & 3)
    lines = torch.cumsum((b == 10).to(torch.int64), 0)[:m]
    at = torch.nonzero(ok).reshape(-1)
    wkey, read_id = wkey[at], lines[at]
    rank, present = obj.rank(wkey)
    host = lambda t: t.cpu().numpy()
    return (host(wkey).view(np.uint64), host(rank.to(torch.int64)), host(present), host(read_id),
            host(seg_of).astype(np.uint32), host(out_from.to(torch.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--link-reads", type=int, default=1_000_000)
    ap.add_argument("--baseline-reads", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links", "links_probe.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    K, L = args.k, args.read_len
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.6))
    bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
    ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
    torch.cuda.synchronize()
    if args.error:
        substitute(bases, args.error, dev)
        torch.cuda.synchronize()
    ctx.push_device(bases.data_ptr(), bases.numel())
    ctx.finish()
    batch = bases[:args.link_reads * (L + 1)].cpu().numpy().tobytes()
    del bases
    torch.cuda.empty_cache()
    n = ctx.result_ptrs()[2]
    base = {"k": K, "edges": n, "genome": args.genome, "reads": args.link_reads, "read_len": L, "bytes": len(batch)}

    def timed(fn, before=None):
        ts, infos = [], []
        for rep in range(args.reps + 1):
            if before:
                before()
            torch.cuda.synchronize()
            t = time.perf_counter()
            info = fn()
            dt = time.perf_counter() - t
            if rep:                                          # (the first call is the warm-up)
                ts.append(dt)
                infos.append(info)
        order = sorted(range(len(ts)), key=ts.__getitem__)
        med = order[len(ts) // 2]
        return [round(x * 1e3, 3) for x in ts], round(ts[med] * 1e3, 3), infos[med], infos

    ms_all, ms, info, _ = timed(lambda: ctx.read_links_begin(carry=True), ctx.read_links_release)
    entries = info["entries"]
    emit(dict(base, op="begin", ms_all=ms_all, ms=ms, entries=entries, edges_without_segment=info["edges_without_segment"],
              ms_link=round(info["ms_link"], 3), ms_rank=round(info["ms_rank"], 3), ms_segments=round(info["ms_segments"], 3)))
    ctx.read_links_release()
    begin_ms = ms

    rng = np.random.default_rng(1)
    half = rng.random(entries) < 0.5
    shares = (("all", None), ("half", half), ("none", np.zeros(entries, dtype=bool)))
    cut = [batch[i * (len(batch) // 10 // (L + 1)) * (L + 1):(i + 1) * (len(batch) // 10 // (L + 1)) * (L + 1)] for i in range(10)]
    cut.append(batch[10 * (len(batch) // 10 // (L + 1)) * (L + 1):])
    for carry in (True, False):
        for share, unique in shares:
            def fresh():
                ctx.read_links_release()
                ctx.read_links_begin(unique, carry)
            add_all, add_ms, ainfo, ainfos = timed(lambda: ctx.read_links_add(batch), fresh)
            fin_all, fin_ms, (table, tinfo), tinfos = timed(lambda: ctx.read_links_table())
            dev_all = sorted(round(a["ms_windows"] + a["ms_scans"] + a["ms_compact"] + t[1]["ms_sort"] + t[1]["ms_reduce"], 3)
                             for a, t in zip(ainfos, tinfos))
            emit(dict(base, op="read_links", mode="carry" if carry else "exact", unique=share,
                      add_ms_all=add_all, add_ms=add_ms, finish_ms_all=fin_all, finish_ms=fin_ms, whole_ms=round(add_ms + fin_ms, 3),
                      reads_per_s=round(args.link_reads / ((add_ms + fin_ms) * 1e-3)),
                      device_ms_all=dev_all, device_ms=dev_all[len(dev_all) // 2],
                      ms_windows=round(ainfo["ms_windows"], 3), ms_scans=round(ainfo["ms_scans"], 3), ms_compact=round(ainfo["ms_compact"], 3),
                      ms_sort=round(tinfo["ms_sort"], 3), ms_reduce=round(tinfo["ms_reduce"], 3),
                      windows=ainfo["windows"], misses=ainfo["misses"], carried=ainfo["carried"], hits=ainfo["hits"],
                      records=ainfo["records"], rows=int(tinfo["rows"])))
            ctx.read_links_release()
            if share != "none":
                pieces = ctx.read_links(cut, unique, carry)
                same = bool(np.array_equal(pieces, table))
                emit(dict(base, op="cut_in_ten", mode="carry" if carry else "exact", unique=share, rows=len(pieces), rows_equal=same))
                if not same:
                    raise SystemExit("the table of the batch cut in ten differs from the table of the batch in one piece")
    # ---- the composed baseline, over the first reads of the batch
    if args.baseline_reads and 2 * (K + 1) <= 62:
        part = batch[:args.baseline_reads * (L + 1)]
        mine = {}
        for carry in (True, False):
            def fresh():
                ctx.read_links_release()
                ctx.read_links_begin(None, carry)
            add_all, add_ms, ainfo, _ = timed(lambda: ctx.read_links_add(part), fresh)
            fin_all, fin_ms, (table, tinfo), _ = timed(lambda: ctx.read_links_table())
            mine[carry] = (table, add_all, add_ms, fin_ms,
                           round(ainfo["ms_windows"] + ainfo["ms_scans"] + ainfo["ms_compact"] + tinfo["ms_sort"] + tinfo["ms_reduce"], 3))
            ctx.read_links_release()
        kp = ctx.result_ptrs()[0]
        keys = gd.device_view(kp, n, torch.int64, dev).clone()
        files, _ = ctx.entry_edge_set()
        ctx.emit()
        with g.Object.from_context(ctx) as obj, \
                g.Object.open({"x" + nm: data for nm, data in files.items()}, "x-entries", g.OBJECT_ENTRY_EDGE_SET) as eobj:
            torch.cuda.synchronize()
            t = time.perf_counter()
            arrays = composed_inputs(obj, eobj, keys, part, K, dev)
            torch.cuda.synchronize()
            gather_ms = (time.perf_counter() - t) * 1e3
            for carry in (True, False):
                t = time.perf_counter()
                got = composed_table(*arrays, K, carry)
                numpy_ms = (time.perf_counter() - t) * 1e3
                table, add_all, add_ms, fin_ms, dev_ms = mine[carry]
                want = np.stack([table["a"].astype(np.uint64), table["b"].astype(np.uint64), table["count"], table["gap_sum"]], axis=1)
                same = bool(np.array_equal(got, want))
                whole = begin_ms + add_ms + fin_ms
                emit(dict(base, op="composed", mode="carry" if carry else "exact", unique="all", reads=args.baseline_reads, bytes=len(part),
                          windows=int(len(arrays[0])), rows=int(len(got)), rows_equal=same,
                          composed_gather_ms=round(gather_ms, 3), composed_numpy_ms=round(numpy_ms, 3), composed_ms=round(gather_ms + numpy_ms, 3),
                          device_begin_ms=begin_ms, device_add_ms_all=add_all, device_add_ms=add_ms, device_finish_ms=fin_ms,
                          device_events_ms=dev_ms, device_whole_ms=round(whole, 3),
                          ratio_composed_to_device_whole=round((gather_ms + numpy_ms) / whole, 2),
                          ratio_composed_to_device_batch=round((gather_ms + numpy_ms) / (add_ms + fin_ms), 2)))
                if not same:
                    raise SystemExit("the composed table and the device's disagree")
    ctx.close()


if __name__ == "__main__":
    main()
