#!/usr/bin/env python3
"""`xenome index` as one process against the four goss commands it is made of as four processes, on one MI355X: the two
synthetic genomes of tools/near_probe.py (A: 100 Mbp of random bases; B: A with 1 % of its bases substituted), written
as FASTA, indexed at k = 25 without --hbm-budget.

  one    xenome index -P idx -G a.fa -H b.fa -v                  one process, one context shared by its four steps
  four   goss build-kmer-set (twice), merge-and-annotate-kmer-sets, compute-near-kmers, each -v, one after another:
         what a pipeline ran before the executable existed, and the baseline

Each form is run --reps times (3), alternating, into a fresh directory; the figure is the median wall time, all runs
kept.  Per step: what the step's own last message says it took ("total build time", "total elapsed time"), for the four
processes also each process's wall time, and how often a context was created and reused.  The index files of the two
forms are compared byte for byte.  One JSON line per run and one summary line, appended to
profiles/xenome/suite_probe.jsonl.

usage: python tools/suite_probe.py [--genome 100000000] [--rate 0.01] [--k 25] [--reps 3] [--dir DIR] [--out FILE]"""
import argparse
import filecmp
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
XENOME = os.path.join(ROOT, "gossamer_amd", "xenome")
STEPS = ("build graft", "build host", "merge and annotate", "near k-mers")
TOOK = re.compile(r"\ttotal (?:build|elapsed) time: ([0-9.eE+-]+)")


def write_genomes(d, n, rate):
    """a.fa and b.fa in d, made on the device as near_probe makes them"""
    import torch
    from tips_probe import substitute
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    lut = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    a = lut[torch.randint(0, 4, (n,), device=dev, generator=gen)]
    b = a.clone()
    substitute(b, rate, dev)
    differing = int((a != b).sum())
    width = 100
    for name, t in (("a", a), ("b", b)):
        rows = t[:n // width * width].reshape(-1, width)
        text = torch.cat([rows, torch.full((rows.shape[0], 1), 10, dtype=torch.uint8, device=dev)], dim=1).cpu().numpy()
        with open(os.path.join(d, name + ".fa"), "wb") as f:
            f.write(b">%s\n" % name.encode())
            text.tofile(f)
            tail = t[n // width * width:].cpu().numpy().tobytes()
            if tail:
                f.write(tail + b"\n")
    del a, b
    torch.cuda.empty_cache()
    return differing


def run(argv, cwd):
    t0 = time.perf_counter()
    p = subprocess.run(argv, cwd=cwd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(argv), p.returncode, err[-2000:]))
    return wall, err


def contexts(err):
    return {"created": err.count("\tGPU context created"), "reused": err.count("\tGPU context reused")}


def one_process(d, k):
    wall, err = run([XENOME, "index", "-P", "idx", "-G", "../a.fa", "-H", "../b.fa", "-K", str(k), "-v"], d)
    took = [float(x) for x in TOOK.findall(err)]          # four steps, then the command's own total
    return {"form": "one", "wall_s": wall, "steps_s": dict(zip(STEPS, took[:4])), "command_s": took[4] if len(took) > 4 else None,
            "contexts": contexts(err)}


def four_processes(d, k):
    cmds = (["build-kmer-set", "-k", str(k), "-I", "../a.fa", "-O", "idx-graft"], ["build-kmer-set", "-k", str(k), "-I", "../b.fa", "-O", "idx-host"],
            ["merge-and-annotate-kmer-sets", "-G", "idx-graft", "-G", "idx-host", "-O", "idx-both"], ["compute-near-kmers", "-G", "idx-both"])
    t0 = time.perf_counter()
    steps, walls, ctx = {}, {}, {"created": 0, "reused": 0}
    for name, c in zip(STEPS, cmds):
        wall, err = run([GOSS] + c + ["-v"], d)
        took = TOOK.findall(err)
        steps[name] = float(took[-1]) if took else None
        walls[name] = wall
        for key, v in contexts(err).items():
            ctx[key] += v
    return {"form": "four", "wall_s": time.perf_counter() - t0, "steps_s": steps, "process_wall_s": walls, "contexts": ctx}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the genomes and the indexes go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xenome", "suite_probe.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()

    top = args.dir or tempfile.mkdtemp(prefix="suite_probe_")
    os.makedirs(top, exist_ok=True)
    try:
        t0 = time.perf_counter()
        differing = write_genomes(top, args.genome, args.rate)
        emit({"probe": "suite", "what": "genomes", "bases": args.genome, "differing": differing, "k": args.k,
              "seconds": time.perf_counter() - t0})
        runs = {"one": [], "four": []}
        for rep in range(args.reps):
            for form, fn in (("four", four_processes), ("one", one_process)):
                d = os.path.join(top, "%s%d" % (form, rep))
                os.makedirs(d)
                rec = fn(d, args.k)
                rec.update({"probe": "suite", "what": "run", "rep": rep})
                emit(rec)
                runs[form].append(rec["wall_s"])
        # the two forms wrote the same index
        a, b = os.path.join(top, "one0"), os.path.join(top, "four0")
        names = sorted(os.listdir(a))
        same = names == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)
        emit({"probe": "suite", "what": "summary", "bases": args.genome, "k": args.k, "reps": args.reps,
              "one_process_wall_s": {"median": statistics.median(runs["one"]), "all": runs["one"]},
              "four_processes_wall_s": {"median": statistics.median(runs["four"]), "all": runs["four"]},
              "index_files": len(names), "index_bytes": sum(os.path.getsize(os.path.join(a, n)) for n in names), "same_files": same})
        if not same:
            raise SystemExit("the two forms wrote different indexes")
    finally:
        if not args.dir:
            shutil.rmtree(top, ignore_errors=True)


if __name__ == "__main__":
    main()
