#!/usr/bin/env python3
"""classify_reads on one MI355X, on the index tools/near_probe.py builds: two 100 Mbp synthetic genomes that differ in
about 0.75 % of their bases, their canonical k-mers (k = 25) counted on the device and merged with weights 1 and 2, the
union opened with goss_gpu_object_open_emitted, the two bitmaps packed from the merged counts and finished with
Object.near_kmers -- what `xenome index` leaves.

Input: four sets of 10^6 reads of 150 bases resident in HBM, drawn from the left genome, from the right genome, from
both (alternating) and from neither (random bases).  Recorded per set, one JSON line each:

  classify   Object.classify_reads with the kept bitmaps (the library's HIP events around its kernels)
  match      Object.match_reads(normalize=True) in count mode on the same object and bytes: the same walk without the
             bits -- the yardstick; classify adds two 8-byte loads per hit and four ballots per run
  composed   what a caller had before: the windows' keys resident in HBM (tools/match_probe.py's baseline),
             Object.rank(normalize=True), a gather of the two bits at the ranks found, and a segmented OR per read in
             place of the sum (host clock; extraction of the keys is left out of its time)

and a summary line per set: classify - match against the spread of the match timings, and composed / classify.  The
classes of the composed form must equal the kernel's.

usage: python tools/classify_probe.py [--k 25] [--genome 100000000] [--rate 0.01] [--reads 1000000] [--reps 5]
                                      [--out profiles/classify/classify_probe.jsonl]"""
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
from match_probe import window_keys  # noqa: E402
from near_probe import LINE, pack  # noqa: E402
from tips_probe import substitute  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify", "classify_probe.jsonl"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K, L, n = args.k, args.read_len, args.reads
    if 2 * K > 62:
        raise SystemExit("the composed path handles one-word keys: k <= 31")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    lut = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    genome_a = lut[torch.randint(0, 4, (args.genome,), device=dev, generator=gen)]
    genome_b = genome_a.clone()
    substitute(genome_b, args.rate, dev)
    differing = int((genome_a != genome_b).sum())

    def draw(sources):
        """n reads of L bases and their '\\n', read i from sources[i % len(sources)] at a random place"""
        t = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
        t[:, L] = 10
        at = torch.randint(0, args.genome - L, (n,), device=dev, generator=gen)
        idx = at[:, None] + torch.arange(L, device=dev)[None, :]
        for s, src in enumerate(sources):
            t[s::len(sources), :L] = src[idx[s::len(sources)]]
        return t.reshape(-1)

    other = lut[torch.randint(0, 4, (args.genome,), device=dev, generator=gen)]
    sets = [("left", draw([genome_a])), ("right", draw([genome_b])), ("both", draw([genome_a, genome_b])), ("neither", draw([other]))]
    del other

    def lines(genome):
        stride = LINE - (K - 1)
        m = (genome.numel() - LINE) // stride + 1
        t = torch.empty((m, LINE + 1), dtype=torch.uint8, device=dev)
        t[:, :LINE] = genome.as_strided((m, LINE), (stride, 1))
        t[:, LINE] = 10
        return t.reshape(-1)

    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_KMER_SET, device=0, hbm_budget=int(free_b * 0.6))
    sides = []
    for genome in (genome_a, genome_b):
        text = lines(genome)
        ctx.reset()
        ctx.push_device(text.data_ptr(), text.numel())
        ctx.finish()
        kp, _, m = ctx.result_ptrs()
        sides.append(gd.device_view(kp, m, torch.int64, dev).clone())
        del text
    del genome_a, genome_b
    torch.cuda.empty_cache()
    ctx.reset()
    for keys, weight in zip(sides, (1, 2)):
        w = torch.full((keys.numel(),), weight, dtype=torch.int32, device=dev)
        ctx.push_run(keys.data_ptr(), w.data_ptr(), keys.numel())
    ctx.finish()
    _, cp, count = ctx.result_ptrs()
    counts = gd.device_view(cp, count, torch.int32, dev).clone()
    ctx.emit_device()
    obj = g.Object.from_context(ctx)
    del sides
    ctx.close()
    torch.cuda.empty_cache()
    lhs, rhs, gray = obj.near_kmers(pack((counts & 1) != 0), pack((counts & 2) != 0))
    obj.classify_bits(lhs.cpu().numpy().view("uint64"), rhs.cpu().numpy().view("uint64"))
    shifts = torch.arange(64, device=dev)
    lbit = ((lhs[:, None] >> shifts[None, :]) & 1).reshape(-1)[:count].to(torch.int64)
    rbit = ((rhs[:, None] >> shifts[None, :]) & 1).reshape(-1)[:count].to(torch.int64)
    torch.cuda.synchronize()
    base = {"k": K, "genome": args.genome, "rate": args.rate, "differing_bases": differing, "kmers": count, "gray": gray,
            "object_bytes": obj.resident_bytes, "reads": n, "read_len": L}

    def median(v):
        return sorted(v)[len(v) // 2]

    def kernel_times(f):
        f()                                        # warm-up
        return [f()[-1]["ms"] for _ in range(args.reps)]

    for name, bases in sets:
        rec = dict(base, set=name, input_bytes=bases.numel())
        classes, windows, info = obj.classify_reads(bases)
        a = kernel_times(lambda: obj.classify_reads(bases))
        emit(dict(rec, op="classify", clock="hip events", ms=round(median(a), 3), ms_all=[round(x, 3) for x in a], windows=info["windows"],
                  counts=info["counts"], windows_per_s=round(info["windows"] / median(a) * 1e3)))
        b = kernel_times(lambda: obj.match_reads(bases, normalize=True))
        emit(dict(rec, op="match", clock="hip events", ms=round(median(b), 3), ms_all=[round(x, 3) for x in b]))

        keys, per_read = window_keys(torch, bases, n, L, K)
        offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offs[1:] = torch.cumsum(per_read, 0)
        torch.cuda.synchronize()

        def composed():
            r, p = obj.rank(keys, normalize=True)
            r = torch.where(p, r, torch.zeros_like(r))
            c = torch.where(p, (lbit[r] << 1) | rbit[r], torch.full_like(r, -1))
            mask = torch.zeros(n, dtype=torch.int32, device=dev)
            cs = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=dev)
            for j in range(4):                      # a segmented OR: per class, is there one between the read's offsets
                cs[1:] = torch.cumsum(c == j, 0)
                mask |= ((cs[offs[1:]] - cs[offs[:-1]]) > 0).to(torch.int32) << j
            torch.cuda.synchronize()
            return mask

        composed()                                  # warm-up
        cts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            mask = composed()
            cts.append((time.perf_counter() - t) * 1e3)
        same = bool(torch.equal(mask, classes))
        emit(dict(rec, op="composed", clock="host", ms=round(median(cts), 3), ms_all=[round(x, 3) for x in cts], key_bytes=keys.numel() * 8,
                  equal_to_classify=same))
        if not same:
            raise SystemExit("the composed classes and the kernel's disagree")
        emit(dict(rec, op="summary", classify_ms=round(median(a), 3), match_ms=round(median(b), 3), excess_ms=round(median(a) - median(b), 3),
                  match_spread_ms=round(max(b) - min(b), 3), excess_within_spread=abs(median(a) - median(b)) <= max(b) - min(b),
                  composed_over_classify=round(median(cts) / median(a), 2)))
        del keys, per_read, offs
    obj.close()


if __name__ == "__main__":
    main()
