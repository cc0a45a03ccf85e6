"""No GPU: the model of the elect tests (elect_model.py) against cases worked out by hand, the corpus of the GPU tests
(elect_cases.py) against vacuity, gossamer_amd.elect against the model, the declarations of include/goss_gpu_elect.h, and
what `goss elect-reads` answers before it needs a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classify_cases as cc
import elect_cases as ec
import elect_model as em
import match_edges as me
import match_model as mm
import pool_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
HELP_LINE = "elect-reads      classify reads according to reference"


# ---- the model, by hand ------------------------------------------------------------------------------------------------

def hand_set():
    """K = 3: AAC (ref 0), ACG (refs 0 and 1; its own reverse complement is CGT), GGA (ref 1), TTT's normal form (no ref)"""
    K = 3
    texts = ("AAC", "ACG", "GGA", "TTT")
    keys = sorted({mm.canonical(me.key_of(t.encode()), K) for t in texts})
    word = {mm.canonical(me.key_of(t.encode()), K): w for t, w in zip(texts, (1, 3, 2, 0))}
    return K, keys, [word[x] for x in keys]


def test_word_by_hand():
    K, keys, colours = hand_set()
    data = b"AAC\nAACG\nGGATTT\nTTT\nAC\n\nCCCC\nGTT\nAANAAC\n"
    words, nwin, by_count = em.colour_reads(data, K, keys, colours)
    #                AAC  AAC|ACG  GGA,GAT,ATT,TTT  TTT(zero word)  none  none  CCC x2 absent  rc(AAC)  AAC after N
    assert words == [1, 3, 2, 0, 0, 0, 0, 1, 1]
    assert nwin == [1, 2, 4, 1, 0, 0, 2, 1, 1]
    assert by_count[:3] == [4, 4, 1] and sum(by_count) == 9


def test_decision_by_hand():
    # t = 0: a read with a window matches whatever it hits, a read without one does not
    assert em.elect_single(0, 1, 0) and not em.elect_single(0, 0, 0) and not em.elect_single(3, 0, 0)
    assert em.elect_single(1, 1, 1) and not em.elect_single(0, 5, 1)
    assert em.elect_single(3, 1, 2) and not em.elect_single(2, 9, 2) and not em.elect_single(1 << 63, 1, 2)
    # the pair whose second mate hits only reference 1 at t = 2: word 2 >= 2, matched; only reference 0: word 1 < 2
    assert em.elect_pair(0, 1, 2, 1, 2) and not em.elect_pair(0, 1, 1, 1, 2)
    assert not em.elect_pair(0, 1, 2, 1, 2, numeric_second_mate=False)
    # both mates together reach the threshold either way
    assert em.elect_pair(1, 1, 2, 1, 2) and em.elect_pair(1, 1, 2, 1, 2, numeric_second_mate=False)
    # a first mate without windows: only the second test can match, and it needs a window of the second mate
    assert not em.elect_pair(3, 0, 0, 0, 1) and em.elect_pair(0, 0, 1, 1, 1) and not em.elect_pair(0, 0, 1, 0, 1)
    # the first mate's word counts in the second test even when the first mate had no window to bring it (it cannot)
    assert em.elect_pair(0, 0, 0, 1, 0) and not em.elect_pair(0, 0, 0, 0, 0) and em.elect_pair(0, 1, 0, 0, 0)
    # bit 63 alone is a large number: matched at any threshold by the numeric rule
    assert em.elect_pair(0, 1, 1 << 63, 1, 64) and not em.elect_pair(0, 1, 1 << 63, 1, 64, numeric_second_mate=False)
    assert em.elect([1, 2, 0, 1], [1, 1, 1, 1], 2, pairs=True) == [True, False]
    assert em.elect([1, 2, 0, 1], [1, 1, 1, 1], 1) == [True, True, False, True]


def test_names_and_file_table_by_hand():
    assert em.file_name("m", "fasta") == "m.fasta" and em.file_name("out/m", "fastq", 2) == "out/m_2.fastq" and em.file_name("m.x", "line", 1) == "m.x_1.txt"
    items = [("fastq", b""), ("line", b""), ("fastq", b"")]
    assert [t[0] for t in em.file_table(items, False, "m", "n")] == ["m.fastq", "n.fastq", "m.txt", "n.txt"]
    assert [t[0] for t in em.file_table(items, True, "", "n")] == ["n_1.fastq", "n_2.fastq", "n_1.txt", "n_2.txt"]
    assert em.file_table(items, True, "", "") == []
    K, keys, colours = hand_set()
    files, m, u = em.elect_reads([("line", b"AAC\nAACG\nTTT\nAC\n")], K, keys, colours, t=2, match_prefix="m", non_match_prefix="n")
    assert (files, m, u) == ({"m.txt": b"AACG\n", "n.txt": b"AAC\nTTT\nAC\n"}, 1, 3)
    files, m, u = em.elect_reads([("line", b"AAC\nAACG\nTTT\nAC\n")], K, keys, colours, t=0, match_prefix="m")
    assert (files, m, u) == ({"m.txt": b"AAC\nAACG\nTTT\n"}, 3, 1)
    pair = [("line", b"AC\nAC\nAAC\n"), ("line", b"GGA\nAAC\nCCC\n")]
    files, m, u = em.elect_reads(pair, K, keys, colours, t=2, pairs=True, match_prefix="m", non_match_prefix="n")
    assert files == {"m_1.txt": b"AC\n", "m_2.txt": b"GGA\n", "n_1.txt": b"AC\nAAC\n", "n_2.txt": b"AAC\nCCC\n"} and (m, u) == (1, 2)
    files, m, u = em.elect_reads(pair, K, keys, colours, nrefs=2, pairs=True, match_prefix="m", numeric_second_mate=False)
    assert files == {"m_1.txt": b"", "m_2.txt": b""} and (m, u) == (0, 3)
    assert em.references([{5, 9}, {9}, {1}]) == ([1, 5, 9], [4, 1, 3])


def test_binding_elect_is_the_model():
    import gossamer_amd as g
    words, nwin, _ = ec.expected("command")
    pw, pn = words[:len(words) // 2 * 2], nwin[:len(words) // 2 * 2]
    for t in (0, 1, 2, 3, 64):
        assert g.elect(words, nwin, t) == em.elect(words, nwin, t)
        assert g.elect(np.array(words, dtype=np.uint64), np.array(nwin, dtype=np.uint32), t, pairs=False) == em.elect(words, nwin, t)
        for numeric in (True, False):
            assert g.elect(pw, pn, t, pairs=True, numeric_second_mate=numeric) == em.elect(pw, pn, t, True, numeric)
    assert g.elect(np.array([1 << 63], dtype=np.uint64).view(np.int64), [1], 1) == [True]
    with pytest.raises(ValueError):
        g.elect([1, 2, 3], [1, 1, 1], 1, pairs=True)
    with pytest.raises(ValueError):
        g.elect([1, 2], [1], 1)


# ---- the corpus against its own claims ---------------------------------------------------------------------------------

def test_case_names_are_what_the_issue_lists():
    assert ec.NAMES == (["every_rank", "uniform", "mixed", "both", "both_swapped", "tiles", "tile_newlines"]
                        + ["ranks%d" % n for n in (1, 63, 64, 65, 129)]
                        + ["edges%dp%d%s" % (L, p, m) for L in (25, 31, 32, 63) for p in (0, 1024) for m in ("", "miss")]
                        + ["pool%d" % S for S in (1, 2, 30, 31, 33, 64)] + ["command"])


def test_every_rank():
    c = ec.fixture("every_rank")
    assert c["K"] == 5 and len(c["keys"]) == 512 and set(c["keys"]) == {mm.canonical(x, 5) for x in range(1024)}
    for w in ec.SPECIAL:
        assert c["colours"].count(w) >= 70
    words, nwin, by_count = ec.expected("every_rank")
    spans = mm.read_spans(c["data"])
    assert len(words) == 1500 and {e - b for b, e in spans} == set(range(5, 21))
    assert by_count[0] >= 10 and by_count[1] >= 10 and by_count[64] >= 100 and sum(1 for x in by_count if x) >= 10
    assert any(w >> 32 and w & 0xFFFFFFFF for w in words) and (1 << 63) in words and 1 in words
    # a read all of whose windows are present and bring the zero word: windows, no bits
    zero = {x for x, w in zip(c["keys"], c["colours"]) if w == 0}
    assert any(w == 0 and n and all(x in zero for x in mm.canonical_many([(x, r) for _, x, r in mm.windows(c["data"][b:e], 5)]))
               for (b, e), w, n in zip(spans, words, nwin))
    # several reads with different words share one run of 64 positions
    by_run = {}
    for (b, e), w in zip(spans, words):
        if (e - 1) // 64 == b // 64:
            by_run.setdefault(b // 64, []).append(w)
    assert any(len(v) >= 4 and len(set(v)) >= 3 for v in by_run.values())
    assert len(c["data"]) > 8 * 2048                                                  # more than one block


def test_or_paths():
    u, m, colours = ec.or_reads()
    assert len(u) == len(m) == 24 and ec.W_A ^ ec.W_B == (1 << 35) | (1 << 50) and (ec.W_A ^ ec.W_B) & 0xFFFFFFFF == 0
    rank_of = {x: i for i, x in enumerate(ec.all5())}

    def per_window(t):
        return [colours[rank_of[x]] for x in mm.canonical_many([(x, r) for _, x, r in mm.windows(t.encode(), 5)])]
    assert per_window(u) == [ec.W_U] * 20
    assert per_window(m) == [ec.W_A, ec.W_B] * 10
    assert ec.expected("uniform")[:2] == ([ec.W_U], [20])
    assert ec.expected("mixed")[:2] == ([ec.W_A | ec.W_B], [20])
    assert ec.expected("both")[:2] == ([ec.W_U, ec.W_A | ec.W_B], [20, 20])
    assert ec.expected("both_swapped")[:2] == ([ec.W_A | ec.W_B, ec.W_U], [20, 20])
    assert len(ec.fixture("both")["data"]) == 50                                      # one run of 64 positions


def test_tiles():
    c = ec.fixture("tiles")
    words, nwin, _ = ec.expected("tiles")
    assert len(words) == 3 and words[1] == sum(1 << b for b in ec.TILE_BITS) and sum(1 for b in ec.TILE_BITS if b >= 32) == 2
    _, body, _, pieces = cc.long_parts()
    for j, p in enumerate(pieces):
        assert em.colour_reads(p.encode(), 31, c["keys"], c["colours"])[0] == [1 << ec.TILE_BITS[j]]
        at = c["data"].find(p.encode())
        assert at // 2048 == j and (at + len(p) - 1) // 2048 == j                     # a tile of its own
    c = ec.fixture("tile_newlines")
    data = c["data"]
    assert data[2046:2050].count(b"\n") == 2 and data[2047:2049] == b"\n\n" and data[2046] != 10 and data[2049] != 10
    words, nwin, _ = ec.expected("tile_newlines")
    assert words == [1 << ec.TILE_BITS[1], 0, 1 << ec.TILE_BITS[2]] and nwin[1] == 0 and nwin[0] == 2047 - 30 and nwin[2] == 102 - 30


@pytest.mark.parametrize("n", cc.RANK_SIZES)
def test_ranks(n):
    words, nwin, by_count = ec.expected("ranks%d" % n)
    assert words == [1 << (r % 64) for r in range(n)] and nwin == [1] * n and by_count[1] == n


@pytest.mark.parametrize("L", cc.EDGE_LENGTHS)
def test_edges(L):
    for phase in me.PHASES:
        for miss in (False, True):
            name = "edges%dp%d%s" % (L, phase, "miss" if miss else "")
            words, nwin, _ = ec.expected(name)
            assert len(words) == L + 2 and set(words) == ({0} if miss else {ec.EDGE_WORD})
            assert ec.fixture(name)["data"] == me.sweep(L, phase, True)[0]
    assert ec.EDGE_WORD >> 32 and ec.EDGE_WORD & 0xFFFFFFFF


@pytest.mark.parametrize("S", ec.POOL_SIZES)
def test_pools(S):
    keys, masks = ec.pool(S)
    samples = ec.pool_samples(S)
    assert len(samples) == S and all(samples) and pm.union_order(samples) == list(keys)
    assert all(0 < m < (1 << S) for m in masks)
    pos = pm.positions(samples)
    z = len(keys)
    back = [0] * z
    for p in pos:
        back[p % z] |= 1 << (p // z)
    assert back == list(masks) and pm.index_shape(samples)[0] == S * z
    if S > 1:
        assert any(m >> (S - 1) for m in masks) and len(set(masks)) == (3 if S == 2 else len(masks))
    words, nwin, by_count = ec.expected("pool%d" % S)
    assert sum(1 for w in words if w) >= 100 and sum(1 for w in words if not w) >= 10


def test_command_corpus():
    texts, ref_sets, keys, colours = ec.command_refs()
    assert [len(s) > 200 for s in ref_sets] == [True] * 3 and set(colours) == {1, 2, 3, 4}
    words, nwin, _ = ec.expected("command")
    assert set(words) == set(range(8))
    for t in (0, 1, 2, 3):
        hits = em.elect(words, nwin, t)
        assert 0 < sum(hits) < len(hits)
    assert sum(em.elect(words, nwin, 0)) > sum(em.elect(words, nwin, 1)) > sum(em.elect(words, nwin, 2)) > sum(em.elect(words, nwin, 3))
    a, b = ec.command_pairs()
    assert len(a) == len(b) == 46
    rank_of = {x: i for i, x in enumerate(keys)}
    wa = [em.read_word(r, 25, rank_of, colours) for r in a]
    wb = [em.read_word(r, 25, rank_of, colours) for r in b]
    assert (wa[40], wb[40]) == ((0, 0), (2, 36)) and (wa[41], wb[41]) == ((0, 0), (1, 36)) and wa[43] == wb[43] == (0, 0)
    numeric = [em.elect_pair(*x, *y, 2) for x, y in zip(wa, wb)]
    meant = [em.elect_pair(*x, *y, 2, numeric_second_mate=False) for x, y in zip(wa, wb)]
    assert numeric[40] and not meant[40] and not numeric[41] and numeric != meant


# ---- the library's declarations ----------------------------------------------------------------------------------------

def test_elect_symbols_are_declared_and_exported():
    """include/goss_gpu_elect.h, included by goss_gpu.h after goss_gpu_taxo.h: what it declares is what the binding lists
    and the library exports; the four calls refuse a NULL object"""
    import gossamer_amd as g
    text = open(os.path.join(ROOT, "include", "goss_gpu_elect.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(goss_gpu_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(g.ELECT_SYMBOLS) == ["goss_gpu_object_colour_reads", "goss_gpu_object_colour_reads_host",
                                                "goss_gpu_object_colours_from_index", "goss_gpu_object_colours_host"]
    top = open(os.path.join(ROOT, "include", "goss_gpu.h")).read()
    assert 0 < top.find('#include "goss_gpu_taxo.h"') < top.find('#include "goss_gpu_elect.h"')
    assert "GOSS_ELECT_NORMALIZE = 1" in text and g.ELECT_NORMALIZE == 1 and "GOSS_ELECT_MAX_COLOURS = 64" in text and g.ELECT_MAX_COLOURS == 64
    assert re.search(r"uint64_t reads;\s*uint64_t windows;\s*uint64_t by_count\[65\];\s*float ms;", text)
    assert C.sizeof(g.binding.ElectInfo) == 8 * 67 + 8
    L = g.load()
    for n in names:
        assert hasattr(L, n), n
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.goss_gpu_object_colours_host.argtypes = [P, P, U32]
    L.goss_gpu_object_colours_from_index.argtypes = [P, P, P]
    L.goss_gpu_object_colour_reads.argtypes = [P, P, U64, U32, U64, P, P, P, P]
    L.goss_gpu_object_colour_reads_host.argtypes = [P, P, U64, U32, U64, P, P, P, P]
    assert L.goss_gpu_object_colours_host(None, None, 1) == -1
    assert L.goss_gpu_object_colours_from_index(None, None, None) == -1
    assert L.goss_gpu_object_colour_reads(None, None, 0, 0, 0, None, None, None, None) == -1
    assert L.goss_gpu_object_colour_reads_host(None, None, 0, 0, 0, None, None, None, None) == -1


# ---- the command, before any device ------------------------------------------------------------------------------------

def run_goss(*args, cwd=None):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode()


def test_cli_help_and_option_table():
    rc, out, err = run_goss("elect-reads", "-h")
    assert rc == 1 and out == b"" and "  " + HELP_LINE + "\n" in err
    for opt in ("--ref-fasta", "--ref-index", "--pool", "-I [ --fasta-in ]", "-i [ --fastq-in ]", "--line-in", "-K [ --kmer-size ]", "--pairs",
                "--ref-threshold", "--match-prefix", "--non-match-prefix", "--preserve-read-order", "--dont-write-reads", "-M [ --max-memory ]",
                "-T [ --num-threads ]", "--device", "--hbm-budget", "--tmp-dir"):
        assert opt in err, opt
    assert "single-seq" not in err
    rc, _, err = run_goss("help")
    assert "  " + HELP_LINE + "\n" in err


def test_cli_usage_errors(tmp_path):
    tail = "use\n\tgoss elect-reads -h\nfor more usage information.\n"
    rc, out, err = run_goss("elect-reads")
    assert rc == 1 and out == b"" and err == "no references: give ref-fasta, ref-index or pool.\n" + tail
    rc, _, err = run_goss("elect-reads", "--ref-index", "a", "--bogus")
    assert rc == 1 and err == "unknown option '--bogus'\n" + tail
    rc, _, err = run_goss("elect-reads", "--ref-index", "a", "--single-seq-refs", "x")
    assert rc == 1 and err == "unknown option '--single-seq-refs'\nunknown option 'x'\n" + tail
    rc, _, err = run_goss("elect-reads", "--pool", "p", "--ref-index", "a")
    assert rc == 1 and err == "pool stands in for the references: ref-fasta and ref-index cannot be given with it.\n" + tail
    # more than 64 references: refused, where the reference's mask bit would shift out
    many = [x for i in range(65) for x in ("--ref-index", "r%d" % i)]
    rc, _, err = run_goss("elect-reads", *many)
    assert rc == 1 and err == "65 references were given; a read's word holds at most 64.\n" + tail
    rc, _, err = run_goss("elect-reads", "--ref-index", "a", "-K", "64")
    assert rc == 1 and "kmer-size" in err and "out of range" in err and err.endswith(tail)
    rc, _, err = run_goss("elect-reads", "--ref-index", "a", "--ref-threshold", "x")
    assert rc == 1 and "the argument ('x') for option '--ref-threshold' is invalid" in err
    rc, _, err = run_goss("elect-reads", "--ref-fasta", str(tmp_path / "nothing.fa"))
    assert rc == 1 and "cannot open file '%s' for reading" % (tmp_path / "nothing.fa") in err
    # a reference index that is not there, and one whose K differs from -K: before any device, and no file is left
    work = tmp_path / "work"
    work.mkdir()
    rc, out, err = run_goss("elect-reads", "--ref-index", str(tmp_path / "nothing"), "--match-prefix", "m", cwd=str(work))
    assert rc == 1 and out == b"" and "'%s.header'" % (tmp_path / "nothing") in err
    import oracle_lib as o
    keys = sorted({o.normalize(v, 5) for v in range(0, 1024, 3)})
    base = str(tmp_path / "five")
    for name, data in o.write_kmer_set(keys, 5, out=base).items():
        open(name, "wb").write(data)
    rc, out, err = run_goss("elect-reads", "--ref-index", base, "--match-prefix", "m", "--dont-write-reads", "-M", "1.5", "-T", "2", cwd=str(work))
    assert rc == 1 and out == b"" and err == "reference index %s has k=5, but --kmer-size is 25.\n" % base + tail
    assert os.listdir(str(work)) == []
