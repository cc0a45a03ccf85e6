#!/usr/bin/env python3
"""compute-near-kmers on one MI355X: two synthetic genomes that share most of their sequence (B is A with a share of its
bases substituted; 100 Mbp and 1 % by default), their canonical k-mers (k = 25) counted on the device, merged with
weights 1 and 2 as merge-and-annotate-kmer-sets does, the union opened with goss_gpu_object_open_emitted and the two
membership bitmaps packed from the merged counts.  Then, for each of the four combinations of GOSS_NEAR_WHOLE_BASES and
GOSS_NEAR_NORMALIZE:

  fused     Object.near_kmers on the device bitmaps (goss_gpu_object_near_kmers): one kernel
  composed  the same result from what existed before it: Object.select of the candidates, then per distinct mask
            x ^ mask with torch, Object.rank(normalize=...) of those still looking, gathers of the old bits at the ranks
            found, and the new bitmaps packed with torch

and checks that both give the same words and the same gray count.  One JSON line per measurement, appended to
profiles/near/near_probe.jsonl.

usage: python tools/near_probe.py [--k 25] [--genome 100000000] [--rate 0.01] [--reps 3] [--no-composed]
Times are host clocks around the calls, each of which ends in a synchronise; one warm-up call of the fused form precedes
the timed ones; the composed form is run twice and the second run is the figure."""
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

LINE = 1000             # bases per line handed to the counter; consecutive lines overlap by k - 1 bases


def distinct_masks(K, whole_bases):
    if whole_bases:
        return [b << (2 * j) for j in range(K) for b in (1, 2, 3)]
    return [1 << t for t in range(K + 1)] + [3 << j for j in range(K)]


def pack(bits):
    """bool [n] -> WordyBitVector words as int64 [(n + 63) // 64]"""
    import torch
    n = bits.numel()
    pad = torch.zeros((n + 63) // 64 * 64, dtype=torch.int64, device=bits.device)
    pad[:n] = bits
    w = torch.ones(64, dtype=torch.int64, device=bits.device) << torch.arange(64, device=bits.device)
    return (pad.reshape(-1, 64) * w).sum(dim=1)


def composed(obj, K, lbit, rbit, whole_bases, normalize):
    """-> (lhs words, rhs words, gray, rank queries made)"""
    import torch
    cand = torch.nonzero(lbit != rbit).reshape(-1)
    x = obj.select(cand).reshape(-1)
    mine = lbit[cand]
    gray = torch.zeros(cand.numel(), dtype=torch.bool, device=cand.device)
    alive = torch.arange(cand.numel(), device=cand.device)
    queries = 0
    for m in distinct_masks(K, whole_bases):
        if alive.numel() == 0:
            break
        r, p = obj.rank(x[alive] ^ m, normalize=normalize)
        queries += alive.numel()
        r = torch.where(p, r, torch.zeros_like(r))
        hit = p & (lbit[r] != rbit[r]) & (lbit[r] != mine[alive])
        gray[alive[hit]] = True
        alive = alive[~hit]
    keep = torch.ones_like(lbit)
    keep[cand[gray]] = False
    return pack(lbit & keep), pack(rbit & keep), int(gray.sum()), queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near", "near_probe.jsonl"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K = args.k
    if 2 * K > 62:
        raise SystemExit("the composed path handles one-word keys: k <= 31")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    t0 = time.perf_counter()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    lut = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    genome_a = lut[torch.randint(0, 4, (args.genome,), device=dev, generator=gen)]
    genome_b = genome_a.clone()
    substitute(genome_b, args.rate, dev)
    differing = int((genome_a != genome_b).sum())

    def lines(genome):
        stride = LINE - (K - 1)
        n = (genome.numel() - LINE) // stride + 1
        t = torch.empty((n, LINE + 1), dtype=torch.uint8, device=dev)
        t[:, :LINE] = genome.as_strided((n, LINE), (stride, 1))
        t[:, LINE] = 10
        return t.reshape(-1)

    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_KMER_SET, device=0, hbm_budget=int(free_b * 0.6))
    sets = []
    for genome in (genome_a, genome_b):
        text = lines(genome)
        ctx.reset()
        ctx.push_device(text.data_ptr(), text.numel())
        ctx.finish()
        kp, _, m = ctx.result_ptrs()
        sets.append(gd.device_view(kp, m, torch.int64, dev).clone())
        del text
    del genome_a, genome_b
    torch.cuda.empty_cache()
    # merge-and-annotate-kmer-sets: weights 1 and 2, the sides of a k-mer are the bits of its merged count
    ctx.reset()
    for keys, weight in zip(sets, (1, 2)):
        w = torch.full((keys.numel(),), weight, dtype=torch.int32, device=dev)
        ctx.push_run(keys.data_ptr(), w.data_ptr(), keys.numel())
    ctx.finish()
    _, cp, n = ctx.result_ptrs()
    counts = gd.device_view(cp, n, torch.int32, dev).clone()
    ctx.emit_device()
    obj = g.Object.from_context(ctx)
    sizes = [s.numel() for s in sets]
    del sets
    ctx.close()
    torch.cuda.empty_cache()
    lbit, rbit = (counts & 1) != 0, (counts & 2) != 0
    lhs, rhs = pack(lbit), pack(rbit)
    candidates = int((lbit != rbit).sum())
    torch.cuda.synchronize()
    base = {"k": K, "genome": args.genome, "rate": args.rate, "differing_bases": differing, "lhs_kmers": sizes[0], "rhs_kmers": sizes[1],
            "kmers": n, "candidates": candidates, "object_bytes": obj.resident_bytes, "setup_s": round(time.perf_counter() - t0, 2)}

    for wb in (False, True):
        for nz in (False, True):
            flags = {"whole_bases": wb, "normalize": nz, "masks": len(distinct_masks(K, wb))}
            ts = []
            for rep in range(args.reps + 1):                # (the first is the warm-up)
                torch.cuda.synchronize()
                t = time.perf_counter()
                fl, fr, gray = obj.near_kmers(lhs, rhs, whole_bases=wb, normalize=nz)
                dt = time.perf_counter() - t
                if rep:
                    ts.append(dt)
            ms = sorted(ts)[len(ts) // 2] * 1e3
            emit(dict(base, op="fused", **flags, gray=gray, ms=round(ms, 3), ms_all=[round(x * 1e3, 3) for x in ts],
                      kmers_per_s=round(n / ms * 1e3), candidates_per_s=round(candidates / ms * 1e3)))
            if args.no_composed:
                continue
            cts = []
            for rep in range(2):                            # (the first is the warm-up: torch loads its kernels and grows its pool)
                torch.cuda.synchronize()
                t = time.perf_counter()
                cl, cr, cgray, queries = composed(obj, K, lbit, rbit, wb, nz)
                torch.cuda.synchronize()
                cts.append(time.perf_counter() - t)
            dt = cts[-1]
            same = bool(torch.equal(cl, fl)) and bool(torch.equal(cr, fr)) and cgray == gray
            emit(dict(base, op="composed", **flags, gray=cgray, ms=round(dt * 1e3, 3), ms_warm_up=round(cts[0] * 1e3, 3), rank_queries=queries,
                      equal_to_fused=same, fused_ms=round(ms, 3), ratio=round(dt * 1e3 / ms, 2)))
            if not same:
                raise SystemExit("the composed result and the kernel's disagree")
            del cl, cr
    obj.close()


if __name__ == "__main__":
    main()
