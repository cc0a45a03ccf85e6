#!/usr/bin/env python3
"""colour_reads on one MI355X, on the index tools/classify_probe.py builds: two 100 Mbp synthetic genomes that differ in
about 0.75 % of their bases, their canonical k-mers (k = 25) counted on the device and merged with weights 1 and 2, the
union opened with goss_gpu_object_open_emitted.  For S = 2 the colour word of a k-mer is its merged count (bit 0: the left
genome holds it, bit 1: the right); for S > 2 the words are drawn at random over the same union.

Input: four sets of 10^6 reads of 150 bases resident in HBM, drawn from the left genome, from the right genome, from
both (alternating) and from neither (random bases).  Recorded per S and set, one JSON line each:

  colour     (a) Object.colour_reads (the library's HIP events around its kernels)
  match      (b) Object.match_reads(normalize=True) in count mode on the same object and bytes: the same walk without the
             word -- the floor; colour adds one 8-byte load per hit and the 64-bit OR per run
  passes     (c) what a caller had before: one k-mer set per reference (the union's k-mers with that bit), S passes of
             Object.match_reads(any=True), one per set, and the OR of the answers in torch; its time is the sum of the
             passes' medians (HIP events) plus the OR (torch events); the words must equal (a)'s
  classify   S = 2 only: Object.classify_reads with the pair of bitmaps packed from the same counts: two dependent bitmap
             loads per hit where colour has one

and a summary line: (a) - (b) against the spread of (b), (c) / (a), and for S = 2 classify - colour.

usage: python tools/elect_probe.py [--k 25] [--genome 100000000] [--rate 0.01] [--reads 1000000] [--reps 5] [--S 2,8,64]
                                   [--out profiles/elect/elect_probe.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gossamer_amd as g  # noqa: E402
from gossamer_amd import dist as gd  # noqa: E402
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
    ap.add_argument("--S", default="2,8,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elect", "elect_probe.jsonl"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    K, L, n = args.k, args.read_len, args.reads
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
    ctx = g.Context(K, g.MODE_KMER_SET, device=0, hbm_budget=int(free_b * 0.5))
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
    kp, cp, count = ctx.result_ptrs()
    union = gd.device_view(kp, count, torch.int64, dev).clone()
    counts = gd.device_view(cp, count, torch.int32, dev).clone()
    ctx.emit_device()
    obj = g.Object.from_context(ctx)
    del sides
    torch.cuda.empty_cache()
    obj.classify_bits(pack((counts & 1) != 0).cpu().numpy().view("uint64"), pack((counts & 2) != 0).cpu().numpy().view("uint64"))
    base = {"k": K, "genome": args.genome, "rate": args.rate, "differing_bases": differing, "kmers": count,
            "object_bytes": obj.resident_bytes, "reads": n, "read_len": L}

    def median(v):
        return sorted(v)[len(v) // 2]

    def kernel_times(f):
        f()                                        # warm-up
        return [f()[-1]["ms"] for _ in range(args.reps)]

    def reference_set(colours, i):
        """the k-mers of the union whose word has bit i, as an object of their own"""
        keys = union[((colours >> i) & 1) != 0].contiguous()
        w = torch.ones(keys.numel(), dtype=torch.int32, device=dev)
        ctx.reset()
        ctx.push_run(keys.data_ptr(), w.data_ptr(), keys.numel())
        ctx.finish()
        ctx.emit_device()
        return g.Object.from_context(ctx)

    for S in [int(x) for x in args.S.split(",")]:
        if S == 2:
            colours = (counts & 3).to(torch.int64)
        elif S == 64:
            colours = torch.randint(-(1 << 63), (1 << 63) - 1, (count,), dtype=torch.int64, device=dev, generator=gen)
        else:
            colours = torch.randint(0, 1 << S, (count,), dtype=torch.int64, device=dev, generator=gen)
        obj.colours(colours.cpu().numpy().view("uint64"), S)
        words, a_ms, b_all = {}, {}, {}
        for name, bases in sets:
            rec = dict(base, S=S, set=name, input_bytes=bases.numel())
            words[name], _, info = obj.colour_reads(bases)
            a = kernel_times(lambda: obj.colour_reads(bases))
            emit(dict(rec, op="colour", clock="hip events", ms=round(median(a), 3), ms_all=[round(x, 3) for x in a], windows=info["windows"],
                      by_count=[x for x in info["by_count"] if x][:8], windows_per_s=round(info["windows"] / median(a) * 1e3)))
            b = kernel_times(lambda: obj.match_reads(bases, normalize=True))
            emit(dict(rec, op="match", clock="hip events", ms=round(median(b), 3), ms_all=[round(x, 3) for x in b]))
            a_ms[name], b_all[name] = median(a), b
            if S == 2:
                c = kernel_times(lambda: obj.classify_reads(bases))
                emit(dict(rec, op="classify", clock="hip events", ms=round(median(c), 3), ms_all=[round(x, 3) for x in c],
                          classify_minus_colour_ms=round(median(c) - median(a), 3)))
        # (c): one object per reference, a pass per object and set
        acc = {name: torch.zeros(n, dtype=torch.int64, device=dev) for name, _ in sets}
        pass_ms = {name: [] for name, _ in sets}
        or_ms = {name: 0.0 for name, _ in sets}
        for i in range(S):
            ref = reference_set(colours, i)
            for name, bases in sets:
                hits = ref.match_reads(bases, normalize=True, any=True)[1]
                t = kernel_times(lambda: ref.match_reads(bases, normalize=True, any=True))
                pass_ms[name].append(median(t))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                acc[name] |= hits.to(torch.int64) << i
                e1.record()
                torch.cuda.synchronize()
                or_ms[name] += e0.elapsed_time(e1)
            ref.close()
        for name, bases in sets:
            rec = dict(base, S=S, set=name, input_bytes=bases.numel())
            same = bool(torch.equal(acc[name], words[name]))
            total = sum(pass_ms[name]) + or_ms[name]
            emit(dict(rec, op="passes", clock="hip events, torch events for the OR", ms=round(total, 3), passes_ms=[round(x, 3) for x in pass_ms[name]],
                      or_ms=round(or_ms[name], 3), equal_to_colour=same))
            if not same:
                raise SystemExit("the S passes and the kernel disagree")
            b = b_all[name]
            emit(dict(rec, op="summary", colour_ms=round(a_ms[name], 3), match_ms=round(median(b), 3), excess_ms=round(a_ms[name] - median(b), 3),
                      match_spread_ms=round(max(b) - min(b), 3), excess_within_spread=abs(a_ms[name] - median(b)) <= max(b) - min(b),
                      passes_over_colour=round(total / a_ms[name], 2)))
        del colours, acc
    obj.close()
    ctx.close()


if __name__ == "__main__":
    main()
