#!/usr/bin/env python3
"""annotate-kmers and classify-reads on one MI355X, on the k-mer set tools/near_probe.py builds: two 100 Mbp synthetic
genomes that differ in about 0.75 % of their bases, the union of their canonical k-mers (k = 25) opened with
goss_gpu_object_open_emitted.

The tree is a complete binary tree of 1 023 nodes with scattered ids; genome A is the first leaf, genome B the last, so
a k-mer of both lifts to the root.  The annotation is made by annotating the probe's own genomes.  Recorded, one JSON
line each (HIP events around the library's kernels unless said otherwise, median of --reps):

  annotate_new      Object.taxo_annotate of genome A's lines on an untouched annotation: every hit is a first touch
  annotate_settled  the same lines again: every hit finds its class there and writes nothing
  match             Object.match_reads(normalize=True) in count mode on the same bytes: the same walk, the floor
  taxon             Object.taxo_classify_reads on 10^6 reads of 150 bases from genome A (one leaf), reads whose halves
                    come from A and from B (two subtrees) and random reads (nothing), each beside its `match` floor
  composed          what a caller had before, for the same reads: the windows' keys resident in HBM, Object.rank
                    (normalize=True), a gather of the annotation's classes and a segmented reduce in torch -- the
                    largest pre-order number per read, then "is every class an ancestor of it" (host clock; extraction
                    of the keys is left out of its time); its results must equal the kernel's
  tally             Object.taxo_tally over the 10^6 results and over `count` values drawn like the annotation (host
                    clock: the call reports no kernel time)

usage: python tools/taxo_probe.py [--k 25] [--genome 100000000] [--rate 0.01] [--reads 1000000] [--reps 5]
                                  [--out profiles/taxo/taxo_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gossamer_amd as g  # noqa: E402
from match_probe import window_keys  # noqa: E402
from near_probe import LINE  # noqa: E402
from tips_probe import substitute  # noqa: E402

NODES = 1023


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taxo", "taxo_probe.jsonl"))
    args = ap.parse_args()
    import numpy as np
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

    def median(v):
        return sorted(v)[len(v) // 2]

    def fig(v):
        return {"ms": round(median(v), 3), "ms_all": [round(x, 3) for x in v]}

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    lut = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    genome_a = lut[torch.randint(0, 4, (args.genome,), device=dev, generator=gen)]
    genome_b = genome_a.clone()
    substitute(genome_b, args.rate, dev)

    def lines(genome):
        stride = LINE - (K - 1)
        m = (genome.numel() - LINE) // stride + 1
        t = torch.empty((m, LINE + 1), dtype=torch.uint8, device=dev)
        t[:, :LINE] = genome.as_strided((m, LINE), (stride, 1))
        t[:, LINE] = 10
        return t.reshape(-1), m

    def draw(first, second):
        """n reads of L bases and their '\\n': the first half of read i from `first`, the second from `second`"""
        t = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
        t[:, L] = 10
        h = L // 2
        for src, lo, hi in ((first, 0, h), (second, h, L)):
            at = torch.randint(0, args.genome - L, (n,), device=dev, generator=gen)
            t[:, lo:hi] = src[at[:, None] + torch.arange(lo, hi, device=dev)[None, :]]
        return t.reshape(-1)

    def draw_one(src):
        t = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
        t[:, L] = 10
        at = torch.randint(0, args.genome - L, (n,), device=dev, generator=gen)
        t[:, :L] = src[at[:, None] + torch.arange(L, device=dev)[None, :]]
        return t.reshape(-1)

    other = lut[torch.randint(0, 4, (args.genome,), device=dev, generator=gen)]
    sets = [("one_leaf", draw_one(genome_a)), ("two_subtrees", draw(genome_a, genome_b)), ("nothing", draw_one(other))]
    del other

    # the union of both genomes' k-mers as one object
    free_b, _ = torch.cuda.mem_get_info(dev)
    ctx = g.Context(K, g.MODE_KMER_SET, device=0, hbm_budget=int(free_b * 0.5))
    text_a, reads_a = lines(genome_a)
    text_b, reads_b = lines(genome_b)
    del genome_a, genome_b
    ctx.push_device(text_a.data_ptr(), text_a.numel())
    ctx.push_device(text_b.data_ptr(), text_b.numel())
    ctx.finish()
    ctx.emit_device()
    obj = g.Object.from_context(ctx)
    ctx.close()
    torch.cuda.empty_cache()
    count = obj.count

    # the tree: node i's parent is (i - 1) // 2; scattered ids; pre-order numbers for the composed form
    rng = np.random.default_rng(3)
    ids = rng.permutation(np.unique(rng.integers(1, 1 << 31, 2 * NODES)))[:NODES].astype(np.uint32)
    parent = np.array([0] + [(i - 1) // 2 for i in range(1, NODES)], dtype=np.uint32)
    obj.taxo_tree(ids, parent)
    pre, last, order, stack = np.zeros(NODES, dtype=np.int64), np.zeros(NODES, dtype=np.int64), 0, [(0, False)]
    while stack:
        v, done = stack.pop()
        if done:
            last[v] = order - 1
            continue
        pre[v] = order
        order += 1
        stack.append((v, True))
        stack += [(c, False) for c in (2 * v + 2, 2 * v + 1) if c < NODES]
    leaf_a, leaf_b = (NODES - 1) // 2, NODES - 1
    base = {"k": K, "genome": args.genome, "rate": args.rate, "kmers": count, "object_bytes": obj.resident_bytes, "nodes": NODES,
            "reads": n, "read_len": L}

    def ms_of(f):
        f()                                        # warm-up
        return [f()[-1]["ms"] for _ in range(args.reps)]

    # annotate: new, then settled; the match floor on the same bytes
    nodes_a = torch.full((reads_a,), int(ids[leaf_a]), dtype=torch.int64, device=dev).to(torch.int32)
    nodes_b = torch.full((reads_b,), int(ids[leaf_b]), dtype=torch.int64, device=dev).to(torch.int32)
    new = []
    for _ in range(args.reps + 1):
        obj.taxo_annotation(None)
        _, info = obj.taxo_annotate(text_a, nodes_a)
        new.append(info["ms"])
    emit(dict(base, op="annotate_new", input_bytes=text_a.numel(), windows=info["windows"], hits=info["hits"], **fig(new[1:])))
    settled = ms_of(lambda: obj.taxo_annotate(text_a, nodes_a))
    emit(dict(base, op="annotate_settled", input_bytes=text_a.numel(), **fig(settled)))
    floor = ms_of(lambda: obj.match_reads(text_a, normalize=True))
    emit(dict(base, op="match", set="genome_a_lines", input_bytes=text_a.numel(), **fig(floor)))
    emit(dict(base, op="summary", set="annotate", new_over_match=round(median(new[1:]) / median(floor), 2),
              settled_over_match=round(median(settled) / median(floor), 2), match_spread_ms=round(max(floor) - min(floor), 3)))
    obj.taxo_annotate(text_b, nodes_b)
    del text_a, text_b, nodes_a, nodes_b
    torch.cuda.empty_cache()
    ann, counts = obj.taxo_read_annotation()
    emit(dict(base, op="annotation", untouched=int((ann == g.TAXO_NONE).sum()), at_root=int(counts[0]), at_leaf_a=int(counts[leaf_a]),
              at_leaf_b=int(counts[leaf_b])))
    # the annotation as pre-order numbers on the device, -1 where untouched (the composed form's gather)
    by_id = {int(x): int(pre[i]) for i, x in enumerate(ids)}
    by_id[g.TAXO_NONE] = -1
    uniq, inv = np.unique(ann, return_inverse=True)
    ann_pre = torch.from_numpy(np.array([by_id[int(x)] for x in uniq], dtype=np.int64)[inv]).to(dev)
    id_of_pre = np.zeros(NODES, dtype=np.int64)
    id_of_pre[pre] = ids
    id_of_pre_t = torch.from_numpy(id_of_pre).to(dev)
    last_of_pre = np.zeros(NODES, dtype=np.int64)
    last_of_pre[pre] = last
    last_t = torch.from_numpy(last_of_pre).to(dev)
    del ann

    results = None
    for name, bases in sets:
        rec = dict(base, set=name, input_bytes=bases.numel())
        res, _, info = obj.taxo_classify_reads(bases)
        a = ms_of(lambda: obj.taxo_classify_reads(bases))
        emit(dict(rec, op="taxon", windows=info["windows"], none=info["none"], many=info["many"], unannotated=info["unannotated"], **fig(a)))
        b = ms_of(lambda: obj.match_reads(bases, normalize=True))
        emit(dict(rec, op="match", **fig(b)))
        keys, per_read = window_keys(torch, bases, n, L, K)
        seg = torch.repeat_interleave(torch.arange(n, device=dev), per_read)
        torch.cuda.synchronize()

        def composed():
            r, p = obj.rank(keys, normalize=True)
            c = torch.where(p, ann_pre[torch.where(p, r, torch.zeros_like(r))], torch.full_like(r, -1))
            deepest = torch.full((n,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, seg, c, "amax")
            m = deepest[seg]
            off = (c >= 0) & ~((c <= m) & (m <= last_t[c.clamp(min=0)]))       # a class that is no ancestor of the largest
            many = torch.zeros(n, dtype=torch.int64, device=dev).scatter_reduce(0, seg, off.to(torch.int64), "amax")
            out_ids = torch.where(deepest < 0, torch.full_like(deepest, g.TAXO_NONE), id_of_pre_t[deepest.clamp(min=0)])
            out_ids = torch.where(many > 0, torch.full_like(out_ids, g.TAXO_MANY), out_ids)
            torch.cuda.synchronize()
            return out_ids

        composed()                                  # warm-up
        cts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            mine = composed()
            cts.append((time.perf_counter() - t) * 1e3)
        same = bool(torch.equal(mine, res.to(torch.int64) & 0xFFFFFFFF))
        emit(dict(rec, op="composed", clock="host", key_bytes=keys.numel() * 8, equal_to_taxon=same, **fig(cts)))
        if not same:
            raise SystemExit("the composed results and the kernel's disagree")
        emit(dict(rec, op="summary", taxon_ms=round(median(a), 3), match_ms=round(median(b), 3), excess_ms=round(median(a) - median(b), 3),
                  match_spread_ms=round(max(b) - min(b), 3), composed_over_taxon=round(median(cts) / median(a), 2)))
        if results is None:
            results = res
        del keys, per_read, seg

    def host_ms(f):
        f()
        v = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            v.append((time.perf_counter() - t) * 1e3)
        return v
    emit(dict(base, op="tally", values=n, clock="host", **fig(host_ms(lambda: obj.taxo_tally(results)))))
    weights = torch.from_numpy(np.concatenate([counts.astype(np.float64), [0.0]]) + 1e-9).to(dev)
    big = torch.from_numpy(ids.astype(np.int64)).to(dev)[torch.multinomial(weights[:NODES], count, replacement=True)].to(torch.int32)
    emit(dict(base, op="tally", values=count, clock="host", **fig(host_ms(lambda: obj.taxo_tally(big)))))
    obj.close()


if __name__ == "__main__":
    main()
