"""The corpus of trim-relative and merge-graph-with-reference: graphs as sorted (edges, counts) lists of Python ints, built
without a device and deterministic.  test_relative_cpu.py holds every case to what its name claims and the two
statements of relative_model.py to one another; test_gpu_relative.py runs the device over the same cases.

Planted forks.  placed() lays groups of out-edges down at exact ranks.  Its forward nodes are small integers whose last
base is not T, so as K-mers they begin with AA; a forward edge v.b is (v << 2) | b.  The mirror image of v.b begins with
comp(b) comp(last(v)), which is never AA, so every mirror image sorts behind every forward edge: the forward edges
occupy the ranks 0 .. F - 1 in the order given, a group of g edges after `pad` single-edge nodes starts at rank `pad`.
Two mirror images leave the same node only if their forward edges are the same edge, so the upper half holds single
edges only: they are never judged and go as mirror images alone.  complement() maps every base to its complement
(without reversing): the set stays closed under reverse complement, the order is reversed and the groups are kept, so
the first group of a graph becomes the last of its complement.
"""
import random
from collections import namedtuple

import dense_graphs as dg
import tips_model as tm

RELS = (-1.0, 0.0, 0.02, 0.25, 0.5, 1.0, 1.5)
KS = (15, 30, 31, 32, 62)             # one-word keys, their limit (K + 1 = 31 bases), two-word keys, their limit
BIG = (1 << 32) - 2                   # the largest multiplicity the device takes

# rels: the cutoffs the device runs the case under (the CPU test runs every case under all of RELS)
Case = namedtuple("Case", "name K edges counts rels tags")
MergeCase = namedtuple("MergeCase", "name K edges counts ref_edges ref_counts tags")


def complement(edges, counts, K):
    top = (1 << (2 * (K + 1))) - 1
    return [top - e for e in reversed(edges)], list(reversed(counts))


def placed(K, groups, extra=()):
    """Sorted (edges, counts) of the forward groups -- [(bases, counts)], e.g. ("AC", (1, 3)) for a fork of two -- their
    mirror images with the same multiplicities, and `extra` [(edge, count)] as given."""
    got = {}
    v = 0
    for bases, cnts in groups:
        while v % 4 == 3:
            v += 1
        assert v < 1 << (2 * (K - 2)) and len(bases) == len(cnts) and list(bases) == sorted(set(bases))
        for b, c in zip(bases, cnts):
            e = (v << 2) | "ACGT".index(b)
            got[e] = got[tm.revcomp(e, K + 1)] = c
        v += 1
    for e, c in extra:
        assert e not in got
        got[e] = c
    edges = sorted(got)
    return edges, [got[e] for e in edges]


SINGLE = ("C", (7,))


def fork(size, minor=1, major=99):
    """a group of `size` out-edges whose first is the minor one"""
    return ("ACGT"[:size] if size < 4 else "ACGT", (minor,) + (major,) * (size - 1))


def palindrome(K):
    """a (K+1)-mer that is its own reverse complement (K odd), away from the forward region of placed()"""
    assert K % 2 == 1
    half = ("ACGT" * K)[:(K + 1) // 2]
    return tm.encode(half + dg.rc_text(half))


def mutual(K):
    """Two forks whose minor edges are each other's mirror image: e = v.A with from-node v, rc(e) = T.rc(v) with
    from-node w; v gets a major edge v.C and w a major edge w.b, and the two majors get their mirror images."""
    v = tm.encode(("CAGGT" * K)[:K])
    e = (v << 2) | 0
    r = tm.revcomp(e, K + 1)
    w = r >> 2
    b = (r & 3) ^ 1
    got = {e: 1, r: 1}
    for major in ((v << 2) | 1, (w << 2) | b):
        got[major] = got[tm.revcomp(major, K + 1)] = 60
    edges = sorted(got)
    return edges, [got[x] for x in edges]


def redrawn(edges, K, seed):
    """multiplicities for a dense graph, one per strand pair, drawn so that most forks have a minor edge"""
    rng = random.Random(seed)
    got = {}
    for e in edges:
        r = tm.revcomp(e, K + 1)
        if e <= r:
            got[e] = got[r] = rng.choice((1, 1, 2, 3, 50, 100, 100, 400))
    return [got[e] for e in edges]


_cases = []


def corpus():
    if _cases:
        return list(_cases)
    add = lambda name, K, ec, rels=(0.02, 0.25), tags=(): _cases.append(Case(name, K, ec[0], ec[1], tuple(rels), tuple(tags)))
    # the 40 dense graphs, multiplicities redrawn
    for i, (name, K, edges, _) in enumerate(dg.corpus()):
        add("dense-" + name, K, (edges, redrawn(edges, K, i)), RELS if i % 8 == 0 or len(edges) >= 2048 else (0.25,), ("dense",))
    # a fork of 2, 3, 4 out-edges that starts at offsets 61 .. 63 of a wave's 64 ranks and 253 .. 255 of a workgroup's 256
    for off in (61, 62, 63, 253, 254, 255):
        for size in (2, 3, 4):
            groups = [SINGLE] * off + [fork(size)] + [SINGLE] * 3
            add("straddle-%d-%d" % (off, size), 15, placed(15, groups), (0.02,), ("straddle", "off%d" % off, "size%d" % size))
    # the first and the last group of the graph
    first = placed(15, [fork(3)] + [SINGLE] * 70)
    add("first-group", 15, first, (0.02,), ("first",))
    add("last-group", 15, complement(first[0], first[1], 15), (0.02,), ("last",))
    # 1, 2, 63, 64, 65 and 257 edges (63, 64, 65 are among the dense graphs too, unplanted)
    add("edges-1", 15, ([palindrome(15)], [5]), (0.25,), ("n1",))
    add("edges-2", 15, placed(15, [SINGLE]), (0.25,), ("n2",))
    add("edges-63", 15, placed(15, [SINGLE] * 29 + [fork(2)], [(palindrome(15), 4)]), (0.25,), ("n63",))
    add("edges-64", 15, placed(15, [SINGLE] * 30 + [fork(2)]), (0.25,), ("n64",))
    add("edges-65", 15, placed(15, [SINGLE] * 30 + [fork(2)], [(palindrome(15), 4)]), (0.25,), ("n65",))
    add("edges-257", 15, placed(15, [SINGLE] * 124 + [fork(4)], [(palindrome(15), 4)]), (0.25,), ("n257",))
    # thresholds hit exactly and missed by one
    add("exact-1-3", 15, placed(15, [("AC", (1, 3))]), (0.25, 0.26), ("exact",))
    add("exact-2-98", 15, placed(15, [("AG", (2, 98))]), (0.02,), ("exact",))
    add("exact-1-99", 15, placed(15, [("CT", (1, 99))]), (0.02,), ("exact",))
    add("equal-counts", 15, placed(15, [("AT", (8, 8))]), RELS, ("equal",))
    # a total above 2^32: four edges near 2^32 - 2
    add("total-over-32-bits", 15, placed(15, [("ACGT", (BIG, BIG, BIG, BIG - 4))]), (0.25, 0.02), ("wide_total",))
    # an edge that is its own reverse complement, below its threshold: one bit, counted once
    add("self-complementary-minor", 1, ([tm.encode("AA"), tm.encode("AT"), tm.encode("TT")], [10, 1, 10]), (0.25,), ("selfrc",))
    # two forks whose minor edges are each other's mirror image
    for K in (5, 31):
        add("mutual-minors-k%d" % K, K, mutual(K), (0.25,), ("mutual",))
    # both key widths
    for K in KS:
        groups = [SINGLE] * 5 + [fork(2)] + [SINGLE] * 60 + [fork(4, 2, 70)] + [SINGLE] * 3 + [("AGT", (50, 1, 50))]
        add("planted-k%d" % K, K, placed(K, groups), (0.02, 0.5), ("planted",))
    return list(_cases)


def _pairs(edges, counts, K):
    """[(e, rc(e), count)] with e <= rc(e), in rank order of e"""
    by = dict(zip(edges, counts))
    return [(e, tm.revcomp(e, K + 1), by[e]) for e in edges if e <= tm.revcomp(e, K + 1)]


def _graph(pairs):
    got = {}
    for e, r, c in pairs:
        got[e] = got[r] = c
    edges = sorted(got)
    return edges, [got[e] for e in edges]


_merge = []


def merge_corpus():
    if _merge:
        return list(_merge)

    def add(name, K, a, b, tags=()):
        _merge.append(MergeCase(name, K, a[0], a[1], b[0], b[1], tuple(tags)))

    empty = ([], [])
    for K in (15, 31):
        base = placed(K, [SINGLE] * 40 + [fork(3)] + [SINGLE] * 40)
        pairs = _pairs(base[0], base[1], K)
        other = [(e, r, c + 1000 + i) for i, (e, r, c) in enumerate(pairs)]                 # counts that differ everywhere
        add("ref-empty-k%d" % K, K, base, empty, ("ref_empty",))
        add("in-empty-k%d" % K, K, empty, base, ("in_empty",))
        add("disjoint-k%d" % K, K, _graph(pairs[::2]), _graph(other[1::2]), ("disjoint",))
        add("identical-k%d" % K, K, base, _graph(other), ("identical",))
        add("ref-in-in-k%d" % K, K, base, _graph(other[::3]), ("ref_subset",))
        add("in-in-ref-k%d" % K, K, _graph(pairs[1::3]), _graph(other), ("in_subset",))
        add("interleaved-k%d" % K, K, _graph(pairs[::2] + pairs[1::4]), _graph(other[1::2] + other[::4]), ("interleaved",))
        oe, oc = _graph(other)
        add("one-edge-less-k%d" % K, K, base, (oe[:7] + oe[8:], oc[:7] + oc[8:]), ("one_edge",))
    add("both-empty", 15, empty, empty, ("in_empty", "ref_empty"))
    # an output much smaller than the estimate: 4 096 edges in, one strand pair of them in the reference
    name, K, edges, _ = max(dg.corpus(), key=lambda g: len(g[2]))
    big = (edges, redrawn(edges, K, 99))
    add("estimate-decides", K, big, _graph([(e, r, 70000) for e, r, _ in _pairs(big[0], big[1], K)[5:6]]), ("small_output",))
    # the reference holds an edge with multiplicity 0: present, so it stays, with 0
    zero = placed(62, [fork(2)] + [SINGLE] * 3)
    add("zero-count-in-ref-k62", 62, zero, (zero[0], [0] + [300] * (len(zero[0]) - 1)), ("zero_count",))
    return list(_merge)
