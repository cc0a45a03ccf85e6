#!/usr/bin/env python3
"""match_reads throughput on one MI355X, against the graph tools/query_probe.py uses (k = 27 over a 100 Mbp synthetic
genome, about 2 x 10^8 edges, built on the device and opened with goss_gpu_object_open_emitted).

Input: 10^7 synthetic 150-base reads resident in HBM -- half drawn from the graph's genome (goss_gpu_synth_reads with
the build's seed), half from another genome, interleaved at random -- plus an all-matching and a none-matching set of
the same size.  Recorded, one JSON line each: count mode, any mode, any mode on the all-matching reads, any mode on the
none-matching reads, and the baseline.

The baseline is the composed path a caller had before match_reads: the same windows' keys already extracted and
resident in HBM (8 bytes per window, read order), goss_gpu_object_rank for their presence, and a torch segmented sum
per read.  Extraction and upload of the keys are left out of its time.

Times: the library's HIP events around its kernels (info ms) and a host clock around each call, which ends in a
synchronise; one warm-up call, then --reps timed ones: median, and all of them for the spread.

usage: python tools/match_probe.py [--reads 10000000] [--graph-reads 20000000] [--reps 5] [--out profiles/match/match_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gossamer_amd as g  # noqa: E402


def window_keys(torch, bases, nreads, L, W, chunk=500_000):
    """keys of every valid W-window in read order (torch, on the device) and the windows per read"""
    keys, per_read = [], []
    for r0 in range(0, nreads, chunk):
        rows = bases[r0 * (L + 1):min(nreads, r0 + chunk) * (L + 1)].view(-1, L + 1)[:, :L]
        low = rows | 0x20
        code = torch.zeros_like(rows, dtype=torch.int64)
        code[low == ord("c")] = 1
        code[low == ord("g")] = 2
        code[low == ord("t")] = 3
        bad = ~((low == ord("a")) | (low == ord("c")) | (low == ord("g")) | (low == ord("t")))
        nw = L - W + 1
        k = torch.zeros((rows.shape[0], nw), dtype=torch.int64, device=rows.device)
        nb = torch.zeros((rows.shape[0], nw), dtype=torch.int32, device=rows.device)
        for i in range(W):
            k |= code[:, i:i + nw] << (2 * (W - 1 - i))
            nb += bad[:, i:i + nw].to(torch.int32)
        valid = nb == 0
        keys.append(k[valid])
        per_read.append(valid.sum(1))
    return torch.cat(keys), torch.cat(per_read)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--graph-reads", type=int, default=20_000_000)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    k, L, n = args.k, args.read_len, args.reads
    W = k + 1
    if 2 * W > 62:
        raise SystemExit("the baseline's keys are one word: k <= 30")

    bases = torch.empty(args.graph_reads * (L + 1), dtype=torch.uint8, device=dev)
    # the reads to match: other reads of the same genome (first_read beyond the build's), and reads of another genome
    same = torch.empty(n * (L + 1), dtype=torch.uint8, device=dev)
    none = torch.empty(n * (L + 1), dtype=torch.uint8, device=dev)
    free_b, _ = torch.cuda.mem_get_info(dev)
    with g.Context(k, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.6)) as ctx:
        ctx.synth_reads(bases.data_ptr(), args.graph_reads, L, args.genome, seed=1)
        ctx.synth_reads(same.data_ptr(), n, L, args.genome, seed=1, first_read=args.graph_reads)
        ctx.synth_reads(none.data_ptr(), n, L, args.genome, seed=2)
        ctx.push_device(bases.data_ptr(), bases.numel())
        ctx.finish()
        ctx.emit_device()
        obj = g.Object.from_context(ctx)
    del bases
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    half = n // 2
    rows = torch.cat([same.view(n, L + 1)[:half], none.view(n, L + 1)[:n - half]])
    mixed = rows[torch.randperm(n, device=dev, generator=gen)].reshape(-1).contiguous()
    del rows
    torch.cuda.synchronize()

    info = obj.info()
    base = {"k": k, "edges": info["count"], "object_bytes": info["resident_bytes"], "reads": n, "read_len": L,
            "input_bytes": mixed.numel()}
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    def timed(op, f, windows, extra=None):
        f()                                        # warm-up
        torch.cuda.synchronize()
        host, devms, last = [], [], None
        for _ in range(args.reps):
            t = time.perf_counter()
            last = f()
            host.append((time.perf_counter() - t) * 1e3)
            if isinstance(last, tuple) and isinstance(last[-1], dict):
                devms.append(last[-1]["ms"])
        ms = sorted(devms or host)[len(host) // 2]
        rec = dict(base, op=op, windows=windows, ms=round(ms, 3), windows_per_s=round(windows / ms * 1e3),
                   clock="hip events" if devms else "host", host_ms_all=[round(x, 3) for x in host],
                   kernel_ms_all=[round(x, 3) for x in devms])
        rec.update(extra or {})
        if isinstance(last, tuple) and isinstance(last[-1], dict):
            rec.update({x: last[-1][x] for x in ("hits", "matched_reads")})
        emit(rec)
        return last

    # the new path
    windows = obj.match_reads(mixed)[2]["windows"]
    w, h, _ = timed("match count", lambda: obj.match_reads(mixed), windows)
    _, h_any, _ = timed("match any", lambda: obj.match_reads(mixed, any=True), windows)
    timed("match any, all reads match", lambda: obj.match_reads(same, any=True), windows)
    timed("match any, no read matches", lambda: obj.match_reads(none, any=True), windows)
    assert torch.equal(h_any, (h != 0).to(h_any.dtype))

    # the baseline: keys in HBM, rank (presence only), segmented sum
    keys, per_read = window_keys(torch, mixed, n, L, W)
    assert keys.numel() == windows and torch.equal(per_read.to(torch.int32), w)
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(per_read, 0)
    torch.cuda.synchronize()

    def rank_only():
        return obj.rank(keys)[1]

    def composed():
        present = obj.rank(keys)[1]
        cs = torch.zeros(windows + 1, dtype=torch.int64, device=dev)
        cs[1:] = torch.cumsum(present, 0)
        hits = cs[offs[1:]] - cs[offs[:-1]]
        torch.cuda.synchronize()
        return hits

    timed("baseline: rank of resident keys", rank_only, windows, {"key_bytes": keys.numel() * 8})
    hits = timed("baseline: rank + segmented sum", composed, windows, {"key_bytes": keys.numel() * 8})
    assert torch.equal(hits.to(torch.int32), h)
    emit(dict(base, op="check", agree=True, matched_reads=int((h != 0).sum())))
    obj.close()


if __name__ == "__main__":
    main()
