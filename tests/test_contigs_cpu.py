"""print-contigs (linear segments) without a GPU: the pure-Python model (contigs_model.py) against answers that follow
by construction from the pieces of tips_cases.py, the per-path rule against the `seen` bitmap, the number formatting,
and the command's usage errors."""
import os
import random
import subprocess

import pytest

import contigs_model as cm
import tips_cases
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
KS = (15, 27, 30, 31, 55)
USE = "use\n\tgoss %s -h\nfor more usage information.\n"
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rank(edges, e):
    i = edges.index(e)
    return i


def test_normalize_restates_the_oracle(oracle):
    rng = random.Random(5)
    for k in (1, 2, 15, 27, 31, 32, 33, 55, 62):
        for _ in range(200):
            v = rng.getrandbits(2 * k)
            assert cm.normalize(v, k) == oracle.normalize(v, k), (k, v)
        if k % 4 == 0:                                   # its own reverse complement
            pal = tm.encode("ACGT" * (k // 4))
            assert cm.normalize(pal, k) == oracle.normalize(pal, k) == pal


def test_double_formatting():
    assert cm.fmt_double(3.0) == "3"
    assert cm.fmt_double(2.5) == "2.5"
    assert cm.fmt_double(10.0 / 3.0) == "3.33333"
    assert cm.fmt_double(123456.7) == "123457"
    assert cm.fmt_double(1234567.0) == "1.23457e+06"
    assert cm.fmt_double(0.0) == "0"
    assert cm.fmt_double(0.5 ** 0.5) == "0.707107"
    assert cm.mean_sd(10, 34, 3) == (10.0 / 3.0, (34.0 / 3.0 - (10.0 / 3.0) * (10.0 / 3.0)) ** 0.5)


def test_body_lines():
    assert cm.body("") == "" and cm.body("", False) == ""
    assert cm.body("A" * 60) == "A" * 60 + "\n"
    assert cm.body("A" * 61) == "A" * 60 + "\nA\n"
    assert cm.body("A" * 125, False) == "A" * 125 + "\n"


@pytest.mark.parametrize("K", KS)
def test_isolated_path_is_one_segment(K):
    strings, _ = tips_cases.Pieces(K).isolated(4)
    text = strings[0][0]
    edges, counts = tm.graph_of(strings, K)
    segs, info = cm.linear_segments(edges, counts, K)
    assert info["starts"] == 2 and info["taken"] == 1 and len(segs) == 1 and info["rule_ok"]
    s = segs[0]
    # both end nodes are dead ends: all K + 6 bases; the strand whose first edge ranks lower
    fwd, rev = rank(edges, tm.encode(text[:K + 1])), rank(edges, tm.encode(rc_text(text)[:K + 1]))
    assert s.bases == (text if fwd < rev else rc_text(text)) and s.first_rank == min(fwd, rev)
    assert (s.edges, s.len, s.min, s.max, s.s, s.s2) == (6, K + 6, 4, 4, 24, 96)
    assert s.include_fst and s.include_lst and all(info["seen"])
    assert cm.render(segs, K) == (">1\n" + cm.body(s.bases)).encode()
    assert cm.render(segs, K, verbose_headers=True, line_breaks=False) == (">1 %d:4:4:4:0\n%s\n" % (K + 6, s.bases)).encode()
    assert cm.render(segs, K, sequence=False) == ("Number\tLength\tMinCov\tMaxCov\tMeanCov\tStdDevCov\n1\t%d\t4\t4\t4\t0\n" % (K + 6)).encode()
    # the filters: on the printed length, on the smallest multiplicity
    assert len(cm.linear_segments(edges, counts, K, min_length=K + 6)[0]) == 1
    assert cm.linear_segments(edges, counts, K, min_length=K + 7)[0] == []
    assert cm.linear_segments(edges, counts, K, min_coverage=5)[0] == []


@pytest.mark.parametrize("K", [k for k in KS if k % 2 == 1])
def test_lone_palindrome_is_its_own_mirror(K):
    strings, _ = tips_cases.Pieces(K).lone_palindrome(7)
    text = strings[0][0]
    assert rc_text(text) == text
    edges, counts = tm.graph_of(strings, K)
    segs, info = cm.linear_segments(edges, counts, K)
    assert info["starts"] == 1 and len(segs) == 1 and info["rule_ok"]
    s = segs[0]
    assert s.bases == text == rc_text(s.bases)
    assert s.first_rank == rank(edges, tm.revcomp(edges[s.end_rank], K + 1))
    assert s.edges == len(edges) == 7


def stem_fork(K, seed=0):
    """a stem that ends in a node N from which two branches leave: three paths meet at N (in = 1, out = 2)"""
    p = tips_cases.Pieces(K, seed)
    stem, n = p.rnd(K + 4), p.rnd(K)
    return n, [(stem + n, 6), (n + "A" + p.rnd(K + 2), 3), (n + "C" + p.rnd(K + 2), 5)]


@pytest.mark.parametrize("K", KS)
def test_fork_node_is_printed_by_the_canonical_rule(K):
    seen_kinds = set()
    for seed in range(6):
        n, strings = stem_fork(K, seed)
        edges, counts = tm.graph_of(strings, K)
        segs, info = cm.linear_segments(edges, counts, K)
        assert info["rule_ok"] and len(segs) == 3 and info["starts"] == 6
        nv = tm.encode(n)
        canon = cm.normalize(nv, K) == nv
        seen_kinds.add(canon)
        for s in segs:
            # the segment seen on the strand of the construction
            fwd = s.bases if (s.full.endswith(n) or s.full.startswith(n)) else rc_text(s.bases)
            full = s.full if (s.full.endswith(n) or s.full.startswith(n)) else rc_text(s.full)
            if full.endswith(n):                              # the stem
                assert s.edges == K + 4 and fwd.endswith(n) == (not canon) and len(fwd) == K + 4 + (0 if canon else K)
            else:                                             # a branch
                assert full.startswith(n) and s.edges == K + 3
                assert fwd.startswith(n) == canon and len(fwd) == K + 3 + (K if canon else 0)
        # every edge or its reverse complement lies on exactly one printed segment
        on = {}
        for s in segs:
            for r in s.ranks:
                on[r] = on.get(r, 0) + 1
        for r, e in enumerate(edges):
            rr = rank(edges, tm.revcomp(e, K + 1))
            assert on.get(r, 0) + (on.get(rr, 0) if rr != r else 0) == 1
    assert K != 15 or seen_kinds == {True, False}


@pytest.mark.parametrize("K", KS)
def test_cycle_is_never_printed(K):
    p = tips_cases.Pieces(K, 3)
    g = p.rnd(5 * K)
    strings = [(g + g[:K], 2)]
    edges, counts = tm.graph_of(strings, K)
    assert len(edges) == 2 * len(g)
    segs, info = cm.linear_segments(edges, counts, K)
    assert segs == [] and info["starts"] == 0 and not any(info["seen"])
    # beside a path: the path is printed, the cycle's edges stay unseen
    more, _ = p.isolated(4)
    e2, c2 = tm.graph_of(strings + more, K)
    segs, info = cm.linear_segments(e2, c2, K)
    assert len(segs) == 1 and info["seen"].count(False) == 2 * len(g)


_reads = {}


def read_graphs(oracle, K):
    """(raw edges, counts, cleaned edges, counts) of the error reads: trimmed at 1, three prune iterations"""
    if K not in _reads:
        reads = tips_cases.error_reads(**READS)
        edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
        te, tc = tm.trim(edges, counts, 1)
        ce, cc, _ = tm.prune(te, tc, K, 3)[-1]
        _reads[K] = (edges, counts, ce, cc)
    return _reads[K]


@pytest.mark.parametrize("K", [27, 33])
def test_error_reads(oracle, K):
    edges, counts, ce, cc = read_graphs(oracle, K)
    segs, info = cm.linear_segments(edges, counts, K)
    assert info["rule_ok"] and len(segs) >= 500
    # a path shorter than K with both ends excluded keeps its last `edges` bases
    short = [s for s in segs if s.edges < K and not s.include_fst and not s.include_lst]
    assert len(short) > 100
    for s in short:
        assert s.len == s.edges and s.bases == s.full[K:] and len(s.full) == s.edges + K
    both = [s for s in segs if s.edges >= K and not s.include_fst and not s.include_lst]
    for s in both:
        assert s.len == s.edges - K and s.bases == s.full[K:len(s.full) - K]
    # --print-rcs changes nothing in this form of the command
    segs_rc, info_rc = cm.linear_segments(edges, counts, K, print_rcs=True)
    assert info_rc["rule_ok"]
    for kw in (dict(), dict(verbose_headers=True, line_breaks=False), dict(sequence=False)):
        assert cm.render(segs, K, **kw) == cm.render(segs_rc, K, **kw)
    # the filters drop segments and renumber the rest
    some, _ = cm.linear_segments(edges, counts, K, min_length=K + 10, min_coverage=5)
    assert 0 < len(some) < len(segs)
    assert [s.first_rank for s in some] == [s.first_rank for s in segs if s.len >= K + 10 and s.min >= 5]
    # the cleaned graph: few, long segments
    csegs, cinfo = cm.linear_segments(ce, cc, K)
    assert cinfo["rule_ok"] and cinfo["longest"] >= 500 and 0 < len(csegs) < 100


@pytest.mark.parametrize("K", KS)
def test_rule_agrees_with_the_bitmap_on_the_hand_made_graphs(K):
    edges, counts, _ = tips_cases.combined_graph(K)
    for print_rcs in (False, True):
        segs, info = cm.linear_segments(edges, counts, K, print_rcs=print_rcs)
        assert info["rule_ok"] and info["starts"] > 0 and segs
    a = cm.linear_segments(edges, counts, K)[0]
    b = cm.linear_segments(edges, counts, K, print_rcs=True)[0]
    assert cm.render(a, K, verbose_headers=True) == cm.render(b, K, verbose_headers=True)
    assert cm.text_of(a) == b"".join(cm.body(s.bases).encode() for s in a)


def test_usage_errors(tmp_path):
    cmd = "print-contigs"
    rc, _, err = run_goss(cmd)
    assert rc == 1 and err == "mandatory option graph-in was not given.\n" + USE % cmd
    rc, _, err = run_goss(cmd, "-G", "a", "-G", "b")
    assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + USE % cmd
    rc, _, err = run_goss(cmd, "-h")
    assert rc == 1
    for opt in ("--graph-in", "--output-file", "--min-length", "--min-coverage", "--no-sequence", "--verbose-headers",
                "--no-line-breaks", "--print-rcs", "--print-linear-segments"):
        assert opt in err, opt
    rc, _, err = run_goss("help")
    assert "print-contigs" in err
    for opt in ("--print-entailed-contigs", "--include-entailed-contigs"):
        rc, _, err = run_goss(cmd, "-G", "a", opt)
        assert rc == 1 and err.startswith("not implemented: --print-entailed-contigs") and err.endswith(USE % cmd)
    rc, _, err = run_goss(cmd, "-G", "a", "--min-length", "x")
    assert rc == 1 and "the argument ('x') for option '--min-length' is invalid" in err
    rc, _, err = run_goss(cmd, "-G", "a", "-o", "/nonexistent-dir/x")
    assert rc == 1 and "The given value of the option output-file was invalid.\n\tcannot create file '/nonexistent-dir/x'\n" in err
    # accepted and ignored: -T, --print-rcs; the command then fails on the missing input, not on its options
    rc, _, err = run_goss(cmd, "-G", str(tmp_path / "none"), "-T", "8", "--print-rcs", "--print-linear-segments", "-v")
    assert rc == 1 and err.startswith("error performing print-contigs:\n") and "none.header" in err
    # a supergraph beside the graph: refused, naming the option that prints linear segments
    (tmp_path / "gr-supergraph.header").write_bytes(b"")
    rc, out, err = run_goss(cmd, "-G", str(tmp_path / "gr"))
    assert rc == 1 and out == b"" and "supergraph contigs are not implemented" in err and "--print-linear-segments" in err
    rc, _, err = run_goss(cmd, "-G", str(tmp_path / "gr"), "--print-linear-segments")
    assert rc == 1 and "supergraph contigs" not in err and "gr.header" in err
