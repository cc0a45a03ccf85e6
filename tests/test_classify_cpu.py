"""The model of classify_reads and of group-reads (classify_model.py) against hand-worked cases, the corpus of the GPU
tests (classify_cases.py) against vacuity, the declarations of include/goss_gpu_classify.h, and what `goss group-reads`
refuses before it asks for a device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import classify_cases as cc
import classify_model as cm
import match_edges as me
import match_model as mm
import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
HELP_LINE = "group-reads      filter reads keeping/discarding those that coincide with a graph."


def kv(s):
    return o.kmer_value(s)


# ---- the model, by hand ------------------------------------------------------------------------------------------------

def test_class_and_file_tables():
    rows = [  # mask, file, class string
        (0, "neither", "neither"), (1, "both", "both"), (2, "rhs", "definitely R"), (3, "rhs", "probably R"),
        (4, "lhs", "definitely L"), (5, "lhs", "probably L"), (6, "ambiguous", "ambiguous"), (7, "ambiguous", "ambiguous"),
        (8, "both", "both"), (9, "both", "probably both"), (10, "rhs", "definitely R"), (11, "rhs", "probably R"),
        (12, "lhs", "definitely L"), (13, "lhs", "probably L"), (14, "ambiguous", "ambiguous"), (15, "ambiguous", "ambiguous")]
    assert [(m, cm.file_of(m), cm.class_str("L", "R", m)) for m in range(16)] == rows
    assert cm.file_name("lhs", "line") == "lhs.txt" and cm.file_name("rhs", "fasta", prefix="p") == "p_rhs.fasta"
    assert cm.file_name("lhs", "fastq", lhs_name="", half=2) == "graft_2.fastq"
    assert cm.file_name("rhs", "fastq", prefix="x", rhs_name="", half=1) == "x_host_1.fastq"
    assert cm.file_name("neither", "line", prefix="x", half=1) == "x_neither_1.txt"
    assert cm.file_name("lhs", "line", lhs_name="mouse") == "mouse.txt"


def test_three_keys_four_reads():
    # K = 3.  AGA, CCA and GGT are canonical as they stand; their reverse complements are TCT, TGG and ACC
    K = 3
    assert [mm.canonical(kv(s), K) == kv(s) for s in ("AGA", "CCA", "GGT")] == [True] * 3
    keys = sorted(kv(s) for s in ("AGA", "CCA", "GGT"))
    assert keys == [kv("AGA"), kv("CCA"), kv("GGT")] == [0b001000, 0b010100, 0b101011]
    lhs, rhs = [0, 0, 1], [1, 0, 0]                      # AGA right only (class 1), CCA neither (0), GGT left only (2)
    data = b"ACC\nTCTNGGT\nTTTTT\nTGGT"                  # rc(GGT) | rc(AGA), GGT | nothing | rc(CCA), GGT
    classes, nwin, counts = cm.classify(data, K, keys, lhs, rhs)
    assert classes == [4, 2 | 4, 0, 1 | 4] and nwin == [1, 2, 3, 2]
    assert counts == [1, 0, 0, 0, 1, 1, 1] + [0] * 9
    assert cm.info_of(data, K, keys, lhs, rhs) == {"reads": 4, "windows": 8, "counts": counts}
    files, out = cm.group_reads([("line", data)], K, keys, lhs, rhs)
    assert files == {"neither.txt": b"TTTTT\n", "both.txt": b"", "rhs.txt": b"", "lhs.txt": b"ACC\nTGGT\n", "ambiguous.txt": b"TCTNGGT\n"}
    # both bits: class 3
    assert cm.classify(b"ACC\n", K, keys, [0, 0, 1], [0, 0, 1])[0] == [8]
    # pairs: one mask per pair, each half to its own file; the second pair is ambiguous only together
    a, b = b"ACC\nACC\n", b"TTTTT\nAGA\n"
    files, out = cm.group_reads([("line", a), ("line", b)], K, keys, lhs, rhs, pairs=True, prefix="p", lhs_name="", rhs_name="h")
    assert files == {"p_neither_1.txt": b"", "p_neither_2.txt": b"", "p_both_1.txt": b"", "p_both_2.txt": b"", "p_graft_1.txt": b"ACC\n",
                     "p_graft_2.txt": b"TTTTT\n", "p_h_1.txt": b"", "p_h_2.txt": b"", "p_ambiguous_1.txt": b"ACC\n", "p_ambiguous_2.txt": b"AGA\n"}
    assert out.splitlines()[-5] == b"1\t50\t" and out.splitlines()[-4] == b"0\t0\th"
    # one group of inputs only: the lines win over FASTA and FASTQ, FASTA over FASTQ
    items = [("fastq", mm.as_fastq([b"AGA"])), ("fasta", mm.as_fasta([b"CCA"])), ("line", b"ACC\n")]
    assert cm.group_reads(items, K, keys, lhs, rhs)[0]["lhs.txt"] == b"ACC\n"
    files, _ = cm.group_reads(items[:2], K, keys, lhs, rhs)
    assert files["both.fasta"] == b"CCA\n" and sorted(files) == ["ambiguous.fasta", "both.fasta", "lhs.fasta", "neither.fasta", "rhs.fasta"]
    assert cm.group_reads(items[:1], K, keys, lhs, rhs)[0]["rhs.fastq"] == b"AGA\n"
    assert cm.group_reads(items, K, keys, lhs, rhs, dont_write=True) == ({}, b"100\t0\t0\t0\t0\n")
    assert cm.bitmap_files("u", [1, 0, 0], [0, 1, 0]) == {"u.lhs-bits": bytes([1] + [0] * 7), "u.rhs-bits": bytes([2] + [0] * 7)}


def test_statistics_text():
    counts = [1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    exp = ("Statistics\n"
           "B\tG\tH\tM\tcount\tpercent\tclass\n"
           "0\t0\t0\t0\t1\t33.3333\t\"neither\"\n"
           "0\t0\t0\t1\t0\t0\t\"both\"\n"
           "0\t0\t1\t0\t0\t0\t\"definitely mouse\"\n"
           "0\t0\t1\t1\t0\t0\t\"probably mouse\"\n"
           "0\t1\t0\t0\t1\t33.3333\t\"definitely \"\n"
           "0\t1\t0\t1\t0\t0\t\"probably \"\n"
           "0\t1\t1\t0\t0\t0\t\"ambiguous\"\n"
           "0\t1\t1\t1\t0\t0\t\"ambiguous\"\n"
           "1\t0\t0\t0\t0\t0\t\"both\"\n"
           "1\t0\t0\t1\t0\t0\t\"probably both\"\n"
           "1\t0\t1\t0\t0\t0\t\"definitely mouse\"\n"
           "1\t0\t1\t1\t0\t0\t\"probably mouse\"\n"
           "1\t1\t0\t0\t0\t0\t\"definitely \"\n"
           "1\t1\t0\t1\t0\t0\t\"probably \"\n"
           "1\t1\t1\t0\t0\t0\t\"ambiguous\"\n"
           "1\t1\t1\t1\t1\t33.3333\t\"ambiguous\"\n"
           "\nSummary\n"
           "count\tpercent\tclass\n"
           "1\t33.3333\t\n"
           "0\t0\tmouse\n"
           "0\t0\tboth\n"
           "1\t33.3333\tneither\n"
           "1\t33.3333\tambiguous\n")
    assert cm.stats_text(counts, "", "mouse").decode() == exp
    assert cm.stats_text(counts, "", "mouse", dont_write=True) == b"33.3333\t0\t0\t33.3333\t33.3333\n"
    # percentages that print as integers, and one with six significant digits
    counts = [0, 0, 2, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert cm.stats_text(counts, dont_write=True) == b"25\t50\t25\t0\t0\n"
    assert cm.stats_text([1] + [0] * 14 + [6], dont_write=True) == b"0\t0\t0\t14.2857\t85.7143\n"
    assert cm.num(100.0) == "100" and cm.num(100.0 * 1 / 3000000) == "3.33333e-05"


# ---- the corpus --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [25, 32])
def test_sixteen(K):
    gens, sets, keys, lhs, rhs = cc.genomes(K)
    assert all(len(s) >= 250 for s in sets)
    assert all(not (sets[i] & sets[j]) for i in range(4) for j in range(i))
    assert len(keys) == sum(len(s) for s in sets)
    rank = {x: i for i, x in enumerate(keys)}
    for j, s in enumerate(sets):
        assert {(lhs[rank[x]], rhs[rank[x]]) for x in s} == {cc.BITS[j]} == {(j >> 1, j & 1)}
    made = cc.sixteen_reads(K)
    classes, nwin, counts = cc.expected("sixteen%d" % K)
    assert len(classes) == len(made)
    per_mask = [0] * 16
    for (m, text), c in zip(made, classes):
        if m is not None:
            assert c == m, (m, c, text)
            per_mask[m] += 1
    assert per_mask == [3] * 16 and set(classes) == set(range(16))
    lens = {len(t) for m, t in made if m is None}
    assert lens == {0, K - 1, K, K + 1}
    data = cc.fixture("sixteen%d" % K)["data"]
    assert b"\n\n" in data and b"N" in data and any(ch in data for ch in b"acgt")
    # both strands are used: some piece is found only in its reverse complement
    assert any(g[p:p + K] in t.upper() for g in gens for _, t in made for p in range(0, 300 - K, 7))
    assert any(mm.rc_text(g[p:p + K]) in t.upper() for g in gens for _, t in made for p in range(0, 300 - K, 7))


def test_dense():
    c = cc.fixture("dense")
    assert c["K"] == 5 and len(c["keys"]) == 512 and c["keys"] == sorted({o.normalize(v, 5) for v in range(1024)})
    assert {(a, b) for a, b in zip(c["lhs"], c["rhs"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    classes, nwin, counts = cc.expected("dense")
    spans = mm.read_spans(c["data"])
    assert len(spans) == 2000 and {e - b for b, e in spans} == {5, 6, 7, 8, 9}
    assert len(set(classes)) >= 8 and all(m for m in classes)
    by_run = {}
    for (b, e), m in zip(spans, classes):
        if b // 64 == (e - 1) // 64:                      # the read lies in one run
            by_run.setdefault(b // 64, []).append(m)
    assert any(len(v) >= 5 and len(set(v)) >= 3 for v in by_run.values())


def test_long():
    c = cc.fixture("long")
    K = c["K"]
    before, body, after, pieces = cc.long_parts()
    assert K == 31 and len(body) == 3 * 2048 + 500
    classes, nwin, counts = cc.expected("long")
    assert classes[1] == 15 and len(classes) == 3
    for j, p in enumerate(pieces):
        assert cm.classify(p.encode(), K, c["keys"], c["lhs"], c["rhs"])[0] == [1 << j]
        at = c["data"].find(p.encode())
        assert at // 2048 == j and (at + len(p) - 1) // 2048 == j            # a tile of its own
    # the body without its pieces is foreign
    bare = list(body)
    for j, p in enumerate(pieces):
        at = j * 2048 + cc.LONG_PIECE_AT
        bare[at:at + len(p)] = "N" * len(p)
    assert cm.classify("".join(bare).encode(), K, c["keys"], c["lhs"], c["rhs"])[0] == [0]
    alone = [cm.classify(t.encode(), K, c["keys"], c["lhs"], c["rhs"])[0][0] for t in (before, after)]
    assert alone == [classes[0], classes[2]] == [4, 0]


@pytest.mark.parametrize("L", cc.EDGE_LENGTHS)
def test_edges(L):
    for phase in me.PHASES:
        data, where = me.sweep(L, phase, True)
        for miss in (False, True):
            name = "edges%dp%d%s" % (L, phase, "miss" if miss else "")
            c = cc.fixture(name)
            assert c["data"] == data and (c["lhs"], c["rhs"]) == ([1], [0]) and len(c["keys"]) == 1
            classes, nwin, counts = cc.expected(name)
            hits = mm.match(data, L, set(c["keys"]), normalize=True, any=True)[1]
            assert classes == [4 if h else 0 for h in hits] and len(classes) == len(where) == L + 2
            # one read per d: with the planted key every d gives 4, with the strand no lookup finds every d gives 0
            assert set(classes) == ({0} if miss else {4})
        x = me.key_of(me.planted(L)[0])
        assert cc.fixture("edges%dp%d" % (L, phase))["keys"] == [mm.canonical(x, L)]
        other = cc.fixture("edges%dp%dmiss" % (L, phase))["keys"][0]
        assert other != mm.canonical(x, L) and mm.canonical(other, L) == mm.canonical(x, L)


@pytest.mark.parametrize("n", cc.RANK_SIZES)
def test_ranks(n):
    c = cc.fixture("ranks%d" % n)
    assert len(c["keys"]) == n and c["keys"] == cc.genomes(25)[2][:n]
    classes, nwin, counts = cc.expected("ranks%d" % n)
    assert classes == [1 << (j % 4) for j in range(n)] and nwin == [1] * n
    if n > 64:
        assert classes[63] != classes[64]
    if n > 128:
        assert classes[127] != classes[128]
    for j, (b, e) in enumerate(mm.read_spans(c["data"])):
        assert e - b == 25 and mm.windows(c["data"][b:e], 25)[0][1] == c["keys"][j]


def test_pairs():
    a, b, want = cc.pairs()
    assert len(a) == len(b) == 40
    _, _, keys, lhs, rhs = cc.genomes(25)
    rank_of = {x: i for i, x in enumerate(keys)}
    ma = [cm.read_mask(r, 25, rank_of, lhs, rhs)[0] for r in a]
    mb = [cm.read_mask(r, 25, rank_of, lhs, rhs)[0] for r in b]
    assert list(zip(ma, mb)) == list(want)
    together = [cm.file_of(x | y) for x, y in zip(ma, mb)]
    assert set(together) == {"neither", "both", "lhs", "rhs", "ambiguous"}
    assert any(t not in (cm.file_of(x), cm.file_of(y)) for t, x, y in zip(together, ma, mb))
    files, out = cm.group_reads([("line", b"\n".join(a) + b"\n"), ("line", b"\n".join(b) + b"\n")], 25, keys, lhs, rhs, pairs=True)
    assert len(files) == 10 and all(files.values())
    assert sum(v.count(b"\n") for n, v in files.items() if "_1." in n) == 40


def test_case_names_are_what_the_issue_lists():
    assert cc.NAMES == (["sixteen25", "sixteen32", "dense", "long"]
                        + ["edges%dp%d%s" % (L, p, m) for L in (25, 31, 32, 63) for p in (0, 1024) for m in ("", "miss")]
                        + ["ranks%d" % n for n in (1, 63, 64, 65, 129)])


# ---- the library's declarations ----------------------------------------------------------------------------------------

def test_classify_symbols_are_declared_and_exported():
    """include/goss_gpu_classify.h, included by goss_gpu.h after goss_gpu_near.h: what it declares is what the binding lists
    and the library exports; the three calls refuse a NULL object"""
    import gossamer_amd as g
    text = open(os.path.join(ROOT, "include", "goss_gpu_classify.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(goss_gpu_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(g.CLASSIFY_SYMBOLS) == ["goss_gpu_object_classify_bits_host", "goss_gpu_object_classify_reads",
                                                   "goss_gpu_object_classify_reads_host"]
    top = open(os.path.join(ROOT, "include", "goss_gpu.h")).read()
    assert 0 < top.find('#include "goss_gpu_near.h"') < top.find('#include "goss_gpu_classify.h"')
    assert "GOSS_CLASSIFY_NORMALIZE = 1" in text and g.CLASSIFY_NORMALIZE == 1
    assert re.search(r"uint64_t reads;\s*uint64_t windows;\s*uint64_t counts\[16\];\s*float ms;", text)
    assert C.sizeof(g.binding.ClassifyInfo) == 8 * 18 + 8
    L = g.load()
    for n in names:
        assert hasattr(L, n), n
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.goss_gpu_object_classify_reads.argtypes = [P, P, U64, P, P, U32, U64, P, P, P, P]
    L.goss_gpu_object_classify_bits_host.argtypes = [P, P, P]
    L.goss_gpu_object_classify_reads_host.argtypes = [P, P, U64, U32, U64, P, P, P, P]
    assert L.goss_gpu_object_classify_reads(None, None, 0, None, None, 0, 0, None, None, None, None) == -1
    assert L.goss_gpu_object_classify_bits_host(None, None, None) == -1
    assert L.goss_gpu_object_classify_reads_host(None, None, 0, 0, 0, None, None, None, None) == -1


# ---- the command, before any device ------------------------------------------------------------------------------------

def run_goss(*args, cwd=None):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode()


def test_cli_usage_errors():
    tail = "use\n\tgoss group-reads -h\nfor more usage information.\n"
    rc, _, err = run_goss("group-reads")
    assert rc == 1 and err == "mandatory option graph-in was not given.\n" + tail
    rc, _, err = run_goss("group-reads", "-G", "a", "-G", "b")
    assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + tail
    rc, _, err = run_goss("group-reads", "-G", "a", "--bogus")
    assert rc == 1 and err == "unknown option '--bogus'\n" + tail
    rc, _, err = run_goss("group-reads", "-h")
    assert rc == 1 and "  " + HELP_LINE + "\n" in err
    for opt in ("--max-memory", "--pairs", "--lhs-name", "--rhs-name", "--output-filename-prefix", "--dont-write-reads",
                "--preserve-read-order", "--line-in", "--device"):
        assert opt in err, opt
    rc, _, err = run_goss("help")
    assert "  " + HELP_LINE + "\n" in err


def test_cli_file_errors_come_before_any_output(tmp_path):
    """a missing .header, a missing .lhs-bits, a mis-sized .rhs-bits: named, and no class file has been created"""
    work = tmp_path / "work"
    work.mkdir()
    reads = tmp_path / "r.txt"
    reads.write_bytes(b"ACGTACGTAC\n")
    opts = ["--line-in", str(reads), "-M", "2.5", "-T", "3", "--preserve-read-order", "--output-filename-prefix", "p"]
    missing = str(tmp_path / "nothing")
    rc, out, err = run_goss("group-reads", "-G", missing, *opts, cwd=str(work))
    assert rc == 1 and out == b"" and err.startswith("error performing group-reads:\n") and "'%s.header'" % missing in err
    assert "for more usage information" not in err
    keys = sorted({o.normalize(v, 5) for v in range(0, 1024, 3)})
    base = str(tmp_path / "u")
    for name, data in o.write_kmer_set(keys, 5, out=base).items():
        open(name, "wb").write(data)
    rc, out, err = run_goss("group-reads", "-G", base, *opts, cwd=str(work))
    assert rc == 1 and out == b"" and "'%s.lhs-bits'" % base in err and "No such file" in err
    nwords = (len(keys) - 1) // 64 + 1
    open(base + ".lhs-bits", "wb").write(bytes(8 * nwords))
    rc, out, err = run_goss("group-reads", "-G", base, *opts, cwd=str(work))
    assert rc == 1 and out == b"" and "'%s.rhs-bits'" % base in err and "No such file" in err
    open(base + ".rhs-bits", "wb").write(bytes(8 * nwords + 8))
    rc, out, err = run_goss("group-reads", "-G", base, *opts, cwd=str(work))
    assert rc == 1 and out == b"" and "file '%s.rhs-bits' holds %d bytes" % (base, 8 * nwords + 8) in err
    assert "the %d k-mers of '%s' need %d" % (len(keys), base, 8 * nwords) in err
    assert os.listdir(str(work)) == []
