#!/usr/bin/env python3
"""pool-samples on one MI355X: random membership masks made on the device (z = 10^8 k-mers by default), S = 32 samples
at density 1/8 and S = 256 at density 1/64 (4 * 10^8 positions either way; rows and pairs do not depend on the density),
through Context.pool_*.  Per shape, HIP-event time (the context's timing
classes, median of five after one warm-up) of

  pool_rows       goss_gpu_pool_add_masks: masks -> bit rows (S / 32 calls)
  pool_pairs      goss_gpu_pool_intersections: rows -> common k-mers of every pair, with the achieved word-pair rate
                  S (S + 1) / 2 * W per second (in whole tiles: what the kernel computes) beside the VALU bound
  pool_positions  rows -> positions (pool_ones_kernel, the scan, pool_positions_kernel)
  index           the SparseArray images of the positions (goss_gpu_emit_sparse_array's passes)

and a check of sizes and of some pairs against torch.  Then

  baseline        what a caller could do before: the same common counts for S = 8 from 28 pairwise merges of two runs
                  through Context (|A| + |B| - |A u B|), host clock around calls that end in a synchronise, beside the
                  pool's rows + pairs for the same eight samples
  command         `goss pool-samples` end to end on 32 k-mer sets of 10^7 k-mers (drawn from 2 * 10^7), wall clock, with the
                  budgets it works out for itself and with --hbm-budget 16

One JSON line per measurement, appended to profiles/pool/pool_probe.jsonl.

usage: python tools/pool_probe.py [--z 100000000] [--reps 5] [--out FILE] [--no-command] [--set-kmers 10000000]

The VALU bound: a word pair is two v_and_b32 and two v_bcnt_u32_b32 (the add is the instruction's third operand): four
lane-operations; 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 * 10^12 lane-operations / s, so 9.8 * 10^12 word pairs / s."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gossamer_amd as g  # noqa: E402
from gossamer_amd import binding as gb  # noqa: E402

VALU_WORD_PAIRS_PER_S = 256 * 4 * 16 * 2.4e9 / 4
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def random_masks(torch, dev, gen, z, density_log2):
    m = torch.randint(-2 ** 31, 2 ** 31, (z,), dtype=torch.int32, device=dev, generator=gen)
    for _ in range(density_log2 - 1):
        m &= torch.randint(-2 ** 31, 2 ** 31, (z,), dtype=torch.int32, device=dev, generator=gen)
    return m


def class_ms(ctx, name):
    return ctx.timing().ms[gb.T_NAMES.index(name)]


def pool_once(ctx, slabs, nsets, z, index=True):
    """one whole pool; -> (ms of rows, pairs, positions, index images), sizes, inter"""
    ctx.pool_begin(nsets, z)
    ctx.timing(reset=True)
    for i, m in enumerate(slabs):
        ctx.pool_add_masks(32 * i, min(32, nsets - 32 * i), m.data_ptr(), z)
    rows = class_ms(ctx, "reduce")
    ctx.timing(reset=True)
    inter = ctx.pool_intersections()
    pairs = class_ms(ctx, "reduce")
    sizes = ctx.pool_sizes()
    pos = img = 0.0
    if index:
        ctx.timing(reset=True)
        ctx._check(ctx._L.goss_gpu_pool_emit_index(ctx._h))          # (the images stay on the device)
        pos, img = class_ms(ctx, "reduce"), class_ms(ctx, "emit")
    ctx.pool_release()
    return (rows, pairs, pos, img), sizes, inter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--set-kmers", type=int, default=10_000_000)
    ap.add_argument("--no-command", action="store_true")
    ap.add_argument("--only-command", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool", "pool_probe.jsonl"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    z = args.z
    W = (z + 63) // 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    ctx = g.Context(25, g.MODE_KMER_SET, device=0)
    ctx._L.goss_gpu_pool_emit_index.argtypes = [gb.C.c_void_p]

    def bit(m, i):
        return (m >> i) & 1

    # ---- the kernels, S = 32 and S = 256 ----
    for nsets, dlog in (() if args.only_command else ((32, 3), (256, 6))):
        slabs = [random_masks(torch, dev, gen, z, dlog) for _ in range(nsets // 32)]
        torch.cuda.synchronize()
        ts = []
        for rep in range(args.reps + 1):                            # (the first is the warm-up)
            t, sizes, inter = pool_once(ctx, slabs, nsets, z)
            if rep:
                ts.append(t)
        checks = [(0, 0), (0, 1), (3, 17), (31, nsets - 1), (nsets - 2, nsets - 1)]
        ok = True
        for i, j in checks:
            want = int((bit(slabs[i // 32], i % 32) & bit(slabs[j // 32], j % 32)).sum())
            ok = ok and inter[i][j] == want and inter[j][i] == want
        ok = ok and all(sizes[i] == inter[i][i] for i in range(nsets))
        ntiles = (nsets + gb.POOL_TILE - 1) // gb.POOL_TILE
        rows, pairs, pos, img = (median([t[k] for t in ts]) for k in range(4))
        word_pairs = nsets * (nsets + 1) // 2 * W
        tile_word_pairs = ntiles * (ntiles + 1) // 2 * gb.POOL_TILE ** 2 * W
        emit({"op": "kernels", "z": z, "nsets": nsets, "density": 2.0 ** -dlog, "row_bytes": nsets * W * 8, "positions": sum(sizes),
              "pool_rows_ms": round(rows, 3), "pool_pairs_ms": round(pairs, 3), "pool_positions_ms": round(pos, 3), "index_images_ms": round(img, 3),
              "all_ms": [[round(x, 3) for x in t] for t in ts],
              "masks_per_s": round(z * (nsets // 32) / rows * 1e3), "word_pairs": word_pairs, "word_pairs_per_s": round(word_pairs / pairs * 1e3),
              "tile_word_pairs_per_s": round(tile_word_pairs / pairs * 1e3), "valu_bound_word_pairs_per_s": round(VALU_WORD_PAIRS_PER_S),
              "share_of_valu_bound": round(tile_word_pairs / pairs * 1e3 / VALU_WORD_PAIRS_PER_S, 4),
              "positions_per_s": round(sum(sizes) / pos * 1e3), "equal_to_torch": ok})
        if not ok:
            raise SystemExit("the pool's counts and torch's disagree")
        del slabs
        torch.cuda.empty_cache()

    # ---- the baseline: S = 8 by pairwise merges ----
    if not args.only_command:
        baseline(torch, dev, gen, ctx, z, bit, emit)

    # ---- the command, end to end ----
    if not args.no_command:
        command(torch, dev, gen, ctx, args, emit)
    ctx.close()


def baseline(torch, dev, gen, ctx, z, bit, emit):
    masks = random_masks(torch, dev, gen, z, 1)
    keys = torch.arange(z, dtype=torch.int64, device=dev)
    sets = [keys[bit(masks, i) == 1] for i in range(8)]
    ones = torch.ones(z, dtype=torch.int32, device=dev)
    del keys
    ctx.pool_begin(8, z)
    ctx.timing(reset=True)
    ctx.pool_add_masks(0, 8, masks.data_ptr(), z)
    inter = ctx.pool_intersections()
    pool_ms = class_ms(ctx, "reduce")
    ctx.pool_release()
    per_pair, same = [], True
    for rnd in range(2):                                            # (the first round is the warm-up)
        per_pair = []
        for i in range(8):
            for j in range(i + 1, 8):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ctx.reset()
                ctx.push_run(sets[i].data_ptr(), ones.data_ptr(), sets[i].numel())
                ctx.push_run(sets[j].data_ptr(), ones.data_ptr(), sets[j].numel())
                ctx.finish()
                union = ctx.result_ptrs()[2]
                per_pair.append((time.perf_counter() - t) * 1e3)
                same = same and sets[i].numel() + sets[j].numel() - union == inter[i][j]
    ctx.reset()
    emit({"op": "baseline", "z": z, "nsets": 8, "pairs": len(per_pair), "merge_ms_per_pair": round(median(per_pair), 3),
          "merge_ms_total": round(sum(per_pair), 3), "pool_rows_and_pairs_ms": round(pool_ms, 3),
          "ratio": round(sum(per_pair) / pool_ms, 1), "equal_to_pool": same})
    if not same:
        raise SystemExit("the pairwise merges and the pool disagree")
    del sets, ones, masks
    torch.cuda.empty_cache()


def command(torch, dev, gen, ctx, args, emit):
    n = args.set_kmers
    tmp = tempfile.mkdtemp(prefix="pool_probe_")
    try:
        universe = torch.unique(torch.randint(0, 1 << 50, (2 * n,), dtype=torch.int64, device=dev, generator=gen))
        names = []
        for i in range(32):
            keys = universe[torch.rand(universe.numel(), device=dev, generator=gen) < 0.5]
            w = torch.ones(keys.numel(), dtype=torch.int32, device=dev)
            ctx.reset()
            ctx.push_run(keys.data_ptr(), w.data_ptr(), keys.numel())
            ctx.finish()
            for suffix, data in ctx.emit().items():
                with open(os.path.join(tmp, "s%d%s" % (i, suffix)), "wb") as f:
                    f.write(data)
            names.append(os.path.join(tmp, "s%d" % i))
        ctx.reset()
        torch.cuda.empty_cache()
        # with the budgets the command works out for itself, then with 16 GB per context
        for budget in (None, 16):
            cmd = [GOSS, "pool-samples", "-v", "-O", os.path.join(tmp, "out")] + ([] if budget is None else ["--hbm-budget", str(budget)])
            for nm in names:
                cmd += ["--kmer-set-in", nm]
            t = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            dt = time.perf_counter() - t
            if p.returncode:
                raise SystemExit("goss pool-samples failed: " + p.stderr.decode())
            with open("%s_command_%s.log" % (os.path.splitext(args.out)[0], budget or "default"), "wb") as f:      # (the command's own progress messages)
                f.write(p.stderr)
            lines = open(os.path.join(tmp, "out.sim")).read().count("\n")
            emit({"op": "command", "nsets": 32, "set_kmers": n, "universe": int(universe.numel()), "hbm_budget_gb": budget, "seconds": round(dt, 2),
                  "sim_lines": lines,
                  "index_bytes": sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if f.startswith("out-index")),
                  "union_bytes": sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if f.startswith("out-union"))})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
