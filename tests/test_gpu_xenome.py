"""`xenome index` and `xenome classify` against the goss commands they are made of: the index files byte for byte those of
build-kmer-set (twice), merge-and-annotate-kmer-sets and compute-near-kmers run as four processes, the classified reads
and the table those of group-reads on <prefix>-both; the one context the four steps of `xenome index` share, counted
from the log; and a context that has built a set, reset, held to a fresh one on the merge-and-annotate and the gray set
that follow.  The inputs are checked on the models (classify_model.py, near_model.py) before any device work: every
class of reads -- graft, host, both, neither, ambiguous -- occurs, single and paired."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import classify_model as cm
import gossamer_amd as g
import match_model as mm
import near_model as nm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
XENOME = os.path.join(ROOT, "gossamer_amd", "xenome")
CLASSES = ("lhs", "rhs", "both", "neither", "ambiguous")
SEED = 20


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(g.binding.LIB_PATH) and os.path.exists(GOSS) and os.path.exists(XENOME)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])


def genomes(n, seed):
    """graft: n random bases; host: the graft with one substitution about every 40 bases and one 60-base stretch replaced"""
    rng = random.Random(seed)
    graft = [rng.choice("ACGT") for _ in range(n)]
    host = list(graft)
    at = n // 2 - 30
    p = rng.randrange(15, 40)
    while p < n:
        if not at - 5 <= p < at + 65:
            host[p] = rng.choice([c for c in "ACGT" if c != host[p]])
        p += rng.randrange(35, 46)
    host[at:at + 60] = [rng.choice("ACGT") for _ in range(60)]
    return "".join(graft), "".join(host), at


def index_model(graft, host, K):
    """(sorted keys, lhs bits, rhs bits) of <prefix>-both after compute-near-kmers"""
    a = mm.object_keys(graft.encode() + b"\n", K, False)
    b = mm.object_keys(host.encode() + b"\n", K, False)
    keys = sorted(a | b)
    lhs, rhs, _ = nm.near_kmers(keys, [int(x in a) for x in keys], [int(x in b) for x in keys], K)
    return keys, lhs, rhs


class World:
    """the two genomes at K, their model index, and 60 reads of 30 to 50 bases of which every class holds some"""

    def __init__(self, K, n):
        self.K = K
        self.graft, self.host, at = genomes(n, SEED + K)
        self.keys, self.lhs, self.rhs = index_model(self.graft, self.host, K)
        self.rank_of = {x: i for i, x in enumerate(self.keys)}
        rng = random.Random(SEED + K + 1)
        unrelated = mm.genome(rng, 4000)
        pool = []
        for _ in range(600):
            L = rng.randrange(30, 51)
            kind = rng.randrange(5)
            if kind == 0:                                     # the graft's side of the replaced stretch
                p = rng.randrange(at, at + 60 - 30)
                r = self.graft[p:p + min(L, at + 60 - p)]
            elif kind == 1:                                   # the host's
                p = rng.randrange(at, at + 60 - 30)
                r = self.host[p:p + min(L, at + 60 - p)]
            elif kind == 2:                                   # anywhere, short: between two substitutions it is common to both
                L = min(L, rng.randrange(30, 34))
                p = rng.randrange(0, n - L)
                r = self.graft[p:p + L]
            elif kind == 3:                                   # nobody's
                p = rng.randrange(0, len(unrelated) - L)
                r = unrelated[p:p + L]
            else:                                             # half of each side of the stretch
                p, q = rng.randrange(at, at + 35), rng.randrange(at, at + 35)
                r = self.graft[p:p + 25] + self.host[q:q + 25]
            if rng.randrange(2):
                r = mm.rc_text(r)
            pool.append(r.encode())
        by = {c: [r for r in pool if self.cls(r) == c] for c in CLASSES}
        assert all(len(by[c]) >= 12 for c in CLASSES), {c: len(v) for c, v in by.items()}
        # twelve of every class; the mate of a read is another read of its class, so that every class has pairs too
        self.reads, self.mates = [], []
        for c in CLASSES:
            self.reads += by[c][:12]
            self.mates += by[c][6:12] + by[c][:6]
        order = list(range(60))
        rng.shuffle(order)
        self.reads = [self.reads[i] for i in order]
        self.mates = [self.mates[i] for i in order]
        assert len(self.reads) == 60 and all(30 <= len(r) <= 50 for r in self.reads + self.mates)
        single = [self.cls(r) for r in self.reads]
        paired = [cm.file_of(self.mask(a) | self.mask(b)) for a, b in zip(self.reads, self.mates)]
        assert all(single.count(c) >= 1 for c in CLASSES), single
        assert all(paired.count(c) >= 1 for c in CLASSES), paired
        # k-mers of both sides, of one side, and gray ones (both bits cleared by compute-near-kmers) all occur
        bits = set(zip(self.lhs, self.rhs))
        assert bits == {(0, 0), (0, 1), (1, 0), (1, 1)}, bits

    def mask(self, read):
        return cm.read_mask(read, self.K, self.rank_of, self.lhs, self.rhs)[0]

    def cls(self, read):
        return cm.file_of(self.mask(read))

    def write(self, d):
        os.makedirs(d, exist_ok=True)
        files = {"g.fa": mm.as_fasta([self.graft.encode()]), "h.fa": mm.as_fasta([self.host.encode()]),
                 "r.fq": mm.as_fastq(self.reads), "m.fq": mm.as_fastq(self.mates), "r.fa": mm.as_fasta(self.reads),
                 "r.txt": b"".join(r + b"\n" for r in self.reads)}
        for name, data in files.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(data)
        return set(files)


@functools.lru_cache(maxsize=None)
def world(K, n):
    return World(K, n)


@pytest.fixture(scope="module")
def world9():
    return world(9, 400)


def run(exe, args, cwd):
    p = subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def messages(err):
    return [line.split("\t", 2)[2] for line in err.splitlines() if line.count("\t") >= 2]


def produced(d, inputs):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in os.listdir(str(d)) if f not in inputs}


def goss_index(d, K, verbose=False):
    """the four goss commands, one process each -> (stdout of all, stderr of the first)"""
    v = ["-v"] if verbose else []
    out, first = b"", None
    for args in (["build-kmer-set", "-k", K, "-I", "g.fa", "-O", "idx-graft"] + v, ["build-kmer-set", "-k", K, "-I", "h.fa", "-O", "idx-host"],
                 ["merge-and-annotate-kmer-sets", "-G", "idx-graft", "-G", "idx-host", "-O", "idx-both"], ["compute-near-kmers", "-G", "idx-both"]):
        rc, o, err = run(GOSS, args, d)
        assert rc == 0, err
        out += o
        first = err if first is None else first
    return out, first


@pytest.fixture(scope="module")
def indexed(world9, tmp_path_factory):
    """directory x: `xenome index -v`; directory s: the four goss commands"""
    x, s = tmp_path_factory.mktemp("x"), tmp_path_factory.mktemp("s")
    inputs = world9.write(str(x))
    world9.write(str(s))
    rc, xout, xerr = run(XENOME, ["index", "-P", "idx", "-G", "g.fa", "-H", "h.fa", "-K", 9, "-v"], x)
    assert rc == 0, xerr
    sout, serr = goss_index(s, 9, verbose=True)
    return {"x": x, "s": s, "inputs": inputs, "xout": xout, "xerr": xerr, "sout": sout, "serr": serr}


def assert_same_index(got, want):
    assert sorted(got) == sorted(want)
    assert all(f.startswith(("idx-graft", "idx-host", "idx-both")) for f in got)
    for f in (p + s for p in ("idx-graft", "idx-host", "idx-both") for s in (".header", ".kmers.header", ".kmers.high-bits")):
        assert f in got, f
    assert "idx-both.lhs-bits" in got and "idx-both.rhs-bits" in got
    for f in want:
        assert got[f] == want[f], f


def test_index_writes_the_files_of_the_four_goss_commands(world9, indexed):
    got, want = produced(indexed["x"], indexed["inputs"]), produced(indexed["s"], indexed["inputs"])
    assert_same_index(got, want)
    assert indexed["xout"] == indexed["sout"] and indexed["xout"].count(b"\t") == 2          # merge-and-annotate's line of three counts
    # ... and the two bitmaps are the model's: the gray k-mers have lost both bits
    assert got["idx-both.lhs-bits"] == nm.words_to_bytes(nm.pack_bits(world9.lhs))
    assert got["idx-both.rhs-bits"] == nm.words_to_bytes(nm.pack_bits(world9.rhs))
    msgs = messages(indexed["xerr"])
    steps = ["building graft reference kmer set", "building host reference kmer set", "merging host and graft reference kmer sets",
             "computing marginal kmers"]
    assert [m for m in msgs if m in steps] == steps and msgs[-1].startswith("total elapsed time: ")


def test_the_four_steps_share_one_context(indexed):
    msgs = messages(indexed["xerr"])
    said = [m.split(" (")[0] for m in msgs if m.startswith("GPU context ")]
    assert sorted(said) == ["GPU context created"] + ["GPU context reused"] * 3, said
    # every step says so once, after its own headline
    steps = [i for i, m in enumerate(msgs) if m in ("building graft reference kmer set", "building host reference kmer set",
                                                    "merging host and graft reference kmer sets", "computing marginal kmers")]
    for lo, hi in zip(steps, steps[1:] + [len(msgs)]):
        assert sum(1 for m in msgs[lo:hi] if m.startswith("GPU context ")) == 1, msgs[lo:hi]
    assert msgs[steps[0]:steps[1]].count("GPU context created (k=9, k-mer set, device 0)") == 1
    # a command run alone creates its own and reuses nothing
    alone = [m.split(" (")[0] for m in messages(indexed["serr"]) if m.startswith("GPU context ")]
    assert alone == ["GPU context created"], alone


def test_index_over_existing_output(world9, indexed, tmp_path):
    """a second run writes the same files again, as build-kmer-set does over a set that is there"""
    inputs = world9.write(str(tmp_path))
    for _ in range(2):
        rc, out, err = run(XENOME, ["index", "-P", "idx", "-G", "g.fa", "-H", "h.fa", "-K", 9], tmp_path)
        assert (rc, err) == (0, "") and out == indexed["xout"]
        assert_same_index(produced(tmp_path, inputs), produced(indexed["s"], indexed["inputs"]))
    rc, out, err = run(GOSS, ["build-kmer-set", "-k", 9, "-I", "g.fa", "-O", "idx-graft"], indexed["s"])
    assert (rc, out, err) == (0, b"", "")
    assert_same_index(produced(indexed["s"], indexed["inputs"]), produced(tmp_path, inputs))


CLASSIFY = {
    "fastq": (["-i", "r.fq"], []),
    "pairs": (["--pairs", "-i", "r.fq", "-i", "m.fq"], []),
    "names": (["-i", "r.fq", "--graft-name", "human", "--host-name", "mouse", "--output-filename-prefix", "s"],
              ["--lhs-name", "human", "--rhs-name", "mouse", "--output-filename-prefix", "s"]),
    "dont-write": (["-i", "r.fq", "--dont-write-reads"], []),
    "fasta": (["-I", "r.fa"], []),
    "lines": (["--line-in", "r.txt", "-M", "0.5", "-T", "2", "--preserve-read-order"], []),
}


@pytest.mark.parametrize("name", sorted(CLASSIFY))
def test_classify_is_group_reads_on_the_both_set(world9, indexed, name):
    xargs, names = CLASSIFY[name]
    gargs = [a for a in xargs if a not in ("--graft-name", "human", "--host-name", "mouse", "--output-filename-prefix", "s")]
    x, s = indexed["x"], indexed["s"]
    before = {d: set(os.listdir(str(d))) for d in (x, s)}
    rc, xout, xerr = run(XENOME, ["classify", "-P", "idx"] + xargs, x)
    assert rc == 0 and xerr == "", xerr
    rc, sout, serr = run(GOSS, ["group-reads", "-G", "idx-both"] + gargs + (names or ["--lhs-name", "graft", "--rhs-name", "host"]), s)
    assert rc == 0 and serr == "", serr
    got, want = produced(x, before[x]), produced(s, before[s])
    try:
        assert xout == sout and sorted(got) == sorted(want) and all(got[f] == want[f] for f in want)
        # and both are the model's: the files, their names under xenome's defaults, and the table
        fmt = {"fasta": "fasta", "lines": "line"}.get(name, "fastq")
        items = [(fmt, open(os.path.join(str(x), f), "rb").read()) for f in xargs if f in ("r.fq", "m.fq", "r.fa", "r.txt")]
        lhs_name, rhs_name, prefix = ("human", "mouse", "s") if name == "names" else ("graft", "host", "")
        files, table = cm.group_reads(items, 9, world9.keys, world9.lhs, world9.rhs, pairs=name == "pairs", prefix=prefix,
                                      lhs_name=lhs_name, rhs_name=rhs_name, dont_write=name == "dont-write")
        assert xout == table
        assert got == files and all(len(v) > 0 for v in got.values())          # (every class holds reads)
        if name == "fastq":
            assert sorted(got) == ["ambiguous.fastq", "both.fastq", "graft.fastq", "host.fastq", "neither.fastq"]
        if name == "pairs":
            assert sorted(got) == sorted("%s_%d.fastq" % (c, h) for c in ("ambiguous", "both", "graft", "host", "neither") for h in (1, 2))
        if name == "names":
            assert sorted(got) == ["s_ambiguous.fastq", "s_both.fastq", "s_human.fastq", "s_mouse.fastq", "s_neither.fastq"]
        if name == "dont-write":
            assert got == {}
    finally:
        for d in (x, s):
            for f in set(os.listdir(str(d))) - before[d]:
                os.unlink(os.path.join(str(d), f))


def test_default_k_on_2000_bases(tmp_path):
    w = world(25, 2000)
    x, s = tmp_path / "x", tmp_path / "s"
    inputs = w.write(str(x))
    w.write(str(s))
    rc, xout, xerr = run(XENOME, ["index", "-P", "idx", "-G", "g.fa", "-H", "h.fa"], x)
    assert (rc, xerr) == (0, ""), xerr
    sout, _ = goss_index(s, 25)
    got = produced(x, inputs)
    assert_same_index(got, produced(s, inputs))
    assert xout == sout
    assert got["idx-both.lhs-bits"] == nm.words_to_bytes(nm.pack_bits(w.lhs))
    assert got["idx-both.rhs-bits"] == nm.words_to_bytes(nm.pack_bits(w.rhs))
    rc, xout, xerr = run(XENOME, ["classify", "-P", "idx", "--pairs", "-i", "r.fq", "-i", "m.fq", "--dont-write-reads"], x)
    assert (rc, xerr) == (0, ""), xerr
    items = [("fastq", mm.as_fastq(w.reads)), ("fastq", mm.as_fastq(w.mates))]
    assert xout == cm.group_reads(items, 25, w.keys, w.lhs, w.rhs, pairs=True, lhs_name="graft", rhs_name="host", dont_write=True)[1]


# ---- a context that is reset between steps ---------------------------------------------------------------------------

def _merge_and_gray(ctx, a, b):
    """merge-and-annotate of two pushed runs (weights 1 and 2) on ctx and the gray set of the result"""
    for keys, w in ((a, 1), (b, 2)):
        k = np.array(keys, dtype=np.uint64)
        c = np.full(len(keys), w, dtype=np.uint32)
        ctx.push_run_host(k.ctypes.data, c.ctypes.data, len(keys))
    counts = ctx.finish()
    keys, cnt = ctx.result()
    ctx.emit()
    with g.Object.from_context(ctx) as obj:          # (the set as emitted, device to device; the bitmaps come after)
        ctx.emit_count_bits(1, ".lhs-bits")
        files = ctx.emit_count_bits(2, ".rhs-bits")
        nw = (obj.count + 63) // 64
        lhs = np.frombuffer(files[".lhs-bits"], dtype=np.uint64)[:nw]
        rhs = np.frombuffer(files[".rhs-bits"], dtype=np.uint64)[:nw]
        nl, nr, gray = obj.near_kmers(lhs.copy(), rhs.copy())
    return counts.distinct, keys, cnt.tolist(), files, nl.tolist(), nr.tolist(), gray


def test_reset_leaves_nothing_a_following_merge_or_gray_set_trips_over():
    K = 25
    w = world(K, 2000)
    a = sorted(mm.object_keys(w.graft.encode() + b"\n", K, False))
    b = sorted(mm.object_keys(w.host.encode() + b"\n", K, False))
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=1 << 30) as fresh:
        want = _merge_and_gray(fresh, a, b)
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=1 << 30) as ctx:
        # a set built from bases and emitted, as the first steps of `xenome index` leave the context
        ctx.push_host(w.host.encode() + b"\n" + mm.rc_text(w.graft).encode() + b"\n")
        built = ctx.finish()
        assert built.distinct == len(set(a) | set(b))
        ctx.emit()
        assert ".kmers.header" in ctx.files()
        ctx.reset()
        got = _merge_and_gray(ctx, a, b)
        # ... and once more after a merge
        ctx.reset()
        again = _merge_and_gray(ctx, a, b)
    assert got[0] == want[0] == len(set(a) | set(b))
    for x, y, z in zip(got, want, again):
        assert x == y == z
    # the model's word on both: the counts are the membership masks, the gray set is near_model's
    keys = sorted(set(a) | set(b))
    sa, sb = set(a), set(b)
    assert want[1] == keys and want[2] == [int(x in sa) + 2 * int(x in sb) for x in keys]
    assert want[4] == nm.pack_bits(w.lhs)[:(len(keys) + 63) // 64] and want[5] == nm.pack_bits(w.rhs)[:(len(keys) + 63) // 64]
    assert want[6] == sum(1 for x, l, r in zip(keys, w.lhs, w.rhs) if (l, r) == (0, 0) and (x in sa) != (x in sb)) > 0
