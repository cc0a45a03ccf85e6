#!/usr/bin/env python3
"""prune-tips on one MI355X: synthetic reads with substituted bases (the reads of tools/error_probe.py), build-graph
k = 27 on the device, then

 * `fused`: goss_gpu_prune_tips, one iteration, on the finished graph (link pass + candidate pass + walk + compaction);
 * `composed`: the same iteration put together from what the library offered before -- the emitted graph opened as an
   Object, batched node_ranks / multiplicity / rank with torch index ops, level-synchronous over the candidates
   (one round of launches per path step, up to 2K + 1 rounds).  It doubles as an independent check: its survivor set
   must equal the kernel's.

The two alternate in one process, --reps times each after one warm-up; then five iterations of the fused path run
on (their reports and times are recorded), and the link pass's bucket table is compared with a plain binary search
(GOSS_GPU_TIPS_BUCKET_BITS=0).  One JSON line per record.  Times are host clocks around calls that end in a
synchronise.

usage: python tools/tips_probe.py [--k 27] [--genome 10000000] [--reads 2000000] [--error 0.01] [--reps 3] [--out f.jsonl]
       [--no-composed]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gossamer_amd as g  # noqa: E402
from gossamer_amd import dist as gd  # noqa: E402


def substitute(bases, rate, dev):
    import torch
    lut = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    step = 1 << 28
    for at in range(0, bases.numel(), step):
        v = bases[at:at + step]
        hit = torch.rand(v.numel(), device=dev, generator=gen) < rate
        sub = lut[torch.randint(0, 4, (v.numel(),), device=dev, generator=gen)]
        nl = v == 10
        v[hit & ~nl] = sub[hit & ~nl]
        del hit, sub, nl


def composed_iteration(obj, keys, K):
    """One prune-tips iteration over the Object's graph with batched queries and torch index ops.  keys: the sorted
    edges (int64, one word).  Returns (keep mask, report dict)."""
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

    _, indeg = out_range(keys >> 2, incoming=True)
    beg = torch.nonzero(indeg == 0).reshape(-1)
    rep = dict(candidates=int(beg.numel()))
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
        nxt = torch.where(go, b, cur[idx])
        cur[idx] = nxt
        length[idx] += go.to(length.dtype)
        over = go & (length[idx] > 2 * K)
        too_long[idx] |= over
        active[idx] = go & ~over
    end = cur
    _, beg_out = out_range(keys[beg] >> 2)
    end_to = keys[end] & node_mask
    _, end_out = out_range(end_to)
    sib_end_b, end_in = out_range(end_to, incoming=True)
    beg_con = beg_out > 1
    end_con = (end_in > 1) | (end_out > 0)
    ok = ~too_long
    both = ok & beg_con & end_con
    none = ok & ~beg_con & ~end_con
    one = ok & (beg_con ^ end_con)
    sib_beg_b, _ = out_range(keys[beg] >> 2)
    at_b = torch.where(end_con, sib_end_b, sib_beg_b)
    at_n = torch.where(end_con, end_in, beg_out)
    c = obj.multiplicity(torch.where(end_con, end, beg)).to(torch.int64) & 0xFFFFFFFF
    weaker = torch.zeros_like(one)
    for j in range(4):
        have = at_n > j
        m = obj.multiplicity(torch.where(have, at_b + j, at_b)).to(torch.int64) & 0xFFFFFFFF
        weaker |= have & (m < c)
    tip = one & ~weaker
    rep.update(too_long=int(too_long.sum()), both_joined=int(both.sum()), isolated=int(none.sum()),
               outweighed=int((one & weaker).sum()), tips=int(tip.sum()), zapped=int(2 * length[tip].sum()),
               joined_at_begin=int((tip & beg_con).sum()), joined_at_end=int((tip & end_con).sum()), rounds=rounds)
    # the second walk marks the paths of the tips and their reverse complements
    zap = torch.zeros(n, dtype=torch.bool, device=keys.device)
    cur = beg[tip].clone()
    left = length[tip].clone()
    while cur.numel():
        e = keys[cur]
        zap[cur] = True
        r, present = obj.rank(revcomp(e, K + 1))
        assert bool(present.all())
        zap[r] = True
        left -= 1
        on = left > 0
        b, _ = out_range(e[on] & node_mask)
        cur, left = b, left[on]
    rep.update(edges_before=n, edges_after=int(n - zap.sum()))
    return ~zap, rep


def bucket_bits(n, length):
    bits = 0
    while bits < 26 and (2 << bits) <= n:
        bits += 1
    return min(bits, 2 * length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-composed", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K, L = args.k, args.read_len
    if 2 * (K + 1) > 62:
        raise SystemExit("the composed path handles one-word edge keys: k <= 30")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    bases = torch.empty(args.reads * (L + 1), dtype=torch.uint8, device=dev)
    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_GRAPH, device=0, hbm_budget=int(free_b * 0.7))
    ctx.synth_reads(bases.data_ptr(), args.reads, L, args.genome, seed=1)
    torch.cuda.synchronize()
    substitute(bases, args.error, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.push_device(bases.data_ptr(), bases.numel())
    ctx.finish()
    build_s = time.perf_counter() - t0
    kp, cp, n = ctx.result_ptrs()
    keys = gd.device_view(kp, n, torch.int64, dev).clone()
    counts = gd.device_view(cp, n, torch.int32, dev).clone()
    obj = None
    if not args.no_composed:
        ctx.emit_device()
        obj = g.Object.from_context(ctx)
    del bases
    torch.cuda.empty_cache()
    bits = bucket_bits(n, K + 1)
    base = {"k": K, "edges": n, "genome": args.genome, "reads": args.reads, "error": args.error, "build_s": round(build_s, 2),
            "bucket_bits": bits}

    def load():
        ctx.reset()
        ctx.push_run(keys.data_ptr(), counts.data_ptr(), n)
        ctx.finish()
        torch.cuda.synchronize()

    def fused():
        load()
        t = time.perf_counter()
        rep = ctx.prune_tips(1)[0]
        return time.perf_counter() - t, rep

    def composed():
        torch.cuda.synchronize()
        t = time.perf_counter()
        keep, rep = composed_iteration(obj, keys, K)
        torch.cuda.synchronize()
        return time.perf_counter() - t, keep, rep

    fused()                                            # warm-up
    tf, tc = [], []
    if obj is not None:
        composed()
    for _ in range(args.reps):
        s, rep = fused()
        tf.append(s)
        if obj is not None:
            s, keep, crep = composed()
            tc.append(s)
    ncand = rep["candidates"]
    work = 9 * n + 2 * ((n + 7) // 8) + 4 * ((1 << bits) + 1) + 4 * ncand
    rec = dict(base, op="fused", iteration=1, ms_all=[round(x * 1e3, 3) for x in tf], ms=round(sorted(tf)[len(tf) // 2] * 1e3, 3),
               edges_per_s=round(n / sorted(tf)[len(tf) // 2]), work_bytes_per_edge=round(work / n, 2), report=rep)
    emit(rec)
    if obj is not None:
        kp2, _, m = ctx.result_ptrs()
        same = bool(torch.equal(gd.device_view(kp2, m, torch.int64, dev), keys[keep]))
        fields = [f for f in crep if f in rep]
        agree = same and all(crep[f] == rep[f] for f in fields)
        med_f, med_c = sorted(tf)[len(tf) // 2], sorted(tc)[len(tc) // 2]
        emit(dict(base, op="composed", iteration=1, ms_all=[round(x * 1e3, 3) for x in tc], ms=round(med_c * 1e3, 3),
                  edges_per_s=round(n / med_c), rounds=crep["rounds"], report={f: crep[f] for f in fields},
                  survivors_equal=same, reports_equal=agree, composed_over_fused=round(med_c / med_f, 2)))
        if not agree:
            raise SystemExit("the composed iteration and the kernel disagree")
    # five iterations on end (the context holds the survivors of iteration 1 of the last repeat)
    for it in range(2, 6):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = ctx.prune_tips(1)[0]
        s = time.perf_counter() - t
        emit(dict(base, op="fused", iteration=it, ms=round(s * 1e3, 3), edges_per_s=round(r["edges_before"] / s) if s else 0, report=r))
    # the link pass: bucket table against a plain binary search over the whole list (everything else is the same)
    for label, env in (("bucket_table", None), ("binary_search", "0")):
        if env is None:
            os.environ.pop("GOSS_GPU_TIPS_BUCKET_BITS", None)
        else:
            os.environ["GOSS_GPU_TIPS_BUCKET_BITS"] = env
        fused()
        ts = [fused()[0] for _ in range(args.reps)]
        emit(dict(base, op="link_ab", search=label, ms_all=[round(x * 1e3, 3) for x in ts], ms=round(sorted(ts)[len(ts) // 2] * 1e3, 3),
                  searches=2 * n))
    os.environ.pop("GOSS_GPU_TIPS_BUCKET_BITS", None)
    if obj is not None:
        obj.close()
    ctx.close()


if __name__ == "__main__":
    main()
