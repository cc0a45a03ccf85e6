"""build-entry-edge-set without a GPU: the pure-Python model (entries_model.py) on graphs whose answers follow by hand,
the rounding rule, the expected file set, and the command's usage errors."""
import os
import random
import struct
import subprocess

import pytest

import entries_model as em
import tips_cases
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
USE = "use\n\tgoss %s -h\nfor more usage information.\n"
K = 15


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def test_fast_revcomp_restates_the_slow_one():
    rng = random.Random(11)
    for k in (1, 3, 4, 16, 28, 32, 34, 56, 63):
        for v in [0, 1, (1 << (2 * k)) - 1] + [rng.getrandbits(2 * k) for _ in range(50)]:
            assert em.revcomp(v, k) == tm.revcomp(v, k), (k, v)


def test_rounding_is_half_away_from_zero():
    assert [em.round_half_away(x) for x in (0.5, 1.5, 2.5, 3.5, 2.4999, 2.5001, 7.0)] == [1, 2, 3, 4, 2, 3, 7]
    assert em.round_half_away(0.49999999999999994) == 0          # (floor(x + 0.5) would say 1)


def test_one_linear_path():
    text = rnd(random.Random(1), K + 6)
    edges, counts = tm.graph_of([(text, 4)], K)
    m = em.entry_edge_set(edges, counts, K)
    first = sorted(edges.index(tm.encode(t[:K + 1])) for t in (text, rc_text(text)))
    assert m["starts"] == first
    assert m["len"] == [6, 6] and m["cnt"] == [4, 4] and m["ends"] == [1, 0]
    assert m["hist"] == {4: 2} and m["cycle_edges"] == 0 and m["longest"] == 6


def test_fork():
    # a node without incoming edges forks into two dead-end branches of K + 3 edges: the two first edges are entries
    # (out = 2), and so is each branch's free end on the other strand (in = 0), whose path stops with the edge into
    # rc(N) (in = 2).  Four paths of K + 3 edges, each the mirror image of one on the other strand.
    strings, _ = tips_cases.Pieces(K).fork(3, 5)
    edges, counts = tm.graph_of(strings, K)
    m = em.entry_edge_set(edges, counts, K)
    assert len(m["starts"]) == 4 and m["len"] == [K + 3] * 4
    assert sorted(m["cnt"]) == [3, 3, 5, 5] and m["hist"] == {3: 2, 5: 2}
    for j, e in enumerate(m["ends"]):
        assert e != j and m["ends"][e] == j and m["cnt"][e] == m["cnt"][j]
    heads = {edges.index(tm.encode(t[:K + 1])) for t, _ in strings}
    assert heads < set(m["starts"])
    assert m["cycle_edges"] == 0


def test_palindromic_path():
    strings, _ = tips_cases.Pieces(K).lone_palindrome(7)
    edges, counts = tm.graph_of(strings, K)
    assert len(edges) == 7
    m = em.entry_edge_set(edges, counts, K)
    assert m["starts"] == [edges.index(tm.encode(strings[0][0][:K + 1]))]
    assert m["len"] == [7] and m["cnt"] == [7] and m["ends"] == [0]


def test_pure_cycle(oracle):
    ring = rnd(random.Random(2), 40)
    edges, counts = tm.graph_of([(ring + ring[:K], 3)], K)
    assert len(edges) == 80
    m, files = em.expected(oracle, edges, counts, K)
    assert m["starts"] == [] and m["cycle_edges"] == 80 and m["hist"] == {} and m["longest"] == 0
    assert files["-entries.header"] == struct.pack("<QQ", 2011041901, K)
    assert files["-entries.ends.upr"] == files["-entries.ends.lwr"] == files["-entries.counts-hist.txt"] == b""
    assert files["-entries.counts.ord0"] == files["-entries.lengths.ord0"] == b""
    assert struct.unpack("<8Q", files["-entries.edges.header"])[5:] == (1 << (2 * (K + 1)), 0, 0)


def two_edge_paths(fwd, bwd):
    """a lone path of two edges whose strands carry the multiplicities `fwd` and `bwd`, each in path order"""
    text = rnd(random.Random(3), K + 2)
    e = [tm.encode(text[i:i + K + 1]) for i in range(2)]
    r = [tm.encode(rc_text(text)[i:i + K + 1]) for i in range(2)]
    got = dict(zip(e + r, list(fwd) + list(bwd)))
    edges = sorted(got)
    return edges, [got[x] for x in edges], edges.index(e[0]), edges.index(r[0])


def test_half_rounds_away_and_paths_keep_their_own_counts():
    edges, counts, f, b = two_edge_paths([1, 2], [2, 3])
    m = em.entry_edge_set(edges, counts, K)
    assert m["starts"] == sorted([f, b]) and m["len"] == [2, 2]
    by_start = dict(zip(m["starts"], m["cnt"]))
    assert by_start[f] == 2                    # 1.5
    assert by_start[b] == 3                    # 2.5: round-to-even would say 2
    assert m["ends"] == [1, 0]


def test_file_set_names(oracle):
    edges, counts, _ = tips_cases.combined_graph(K)
    m, files = em.expected(oracle, edges, counts, K)
    n = len(m["starts"])
    assert n > 0 and len(m["cnt"]) == len(m["len"]) == len(m["ends"]) == n
    assert all(m["ends"][e] == j for j, e in enumerate(m["ends"]))
    assert sum(m["hist"].values()) == n and list(m["hist"]) == sorted(m["hist"])
    assert sum(m["len"]) + m["cycle_edges"] == len(edges)
    vba = ["%s.ord%s" % (c, s) for c in (".counts", ".lengths") for s in ("0", "1", "2")]
    vba += ["%s.ord%dp%s" % (c, i, s) for c in (".counts", ".lengths") for i in (1, 2)
            for s in (".header", ".high-bits", "-d0", "-d1")]
    fixed = [".header", ".counts-hist.txt", ".ends.upr", ".ends.lwr", ".edges.header", ".edges.high-bits", ".edges-d0", ".edges-d1"] + vba
    rest = set(files) - {"-entries" + s for s in fixed}
    assert {"-entries" + s for s in fixed} <= set(files)
    assert rest and all(".low-bits" in name for name in rest)
    assert len(files["-entries.ends.upr"]) == n and len(files["-entries.ends.lwr"]) == 4 * n
    assert len(files["-entries.counts.ord0"]) == len(files["-entries.lengths.ord0"]) == n
    assert struct.unpack("<8Q", files["-entries.edges.header"])[7] == n


def test_missing_reverse_complement_is_refused():
    edges, counts, _ = tips_cases.combined_graph(K)
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with pytest.raises(ValueError, match="edge %d has no reverse complement" % be.index(beg)):
        em.entry_edge_set(be, bc, K)


def test_usage_errors():
    """GossCmdFactoryBuildEntryEdgeSet::create (GossCmdBuildEntryEdgeSet.cc:68-84): refused before any device is opened"""
    cmd = "build-entry-edge-set"
    rc, out, err = run_goss(cmd)
    assert rc == 1 and out == b"" and err == "mandatory option graph-in was not given.\n" + USE % cmd
    rc, _, err = run_goss(cmd, "-G", "a", "-G", "b")
    assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + USE % cmd
    rc, _, err = run_goss(cmd, "-G", "a", "-T", "many")
    assert rc == 1 and "num-threads" in err
    rc, _, err = run_goss("help")
    assert "build-entry-edge-set" in err
