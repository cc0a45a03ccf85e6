"""The model of read links (links_model.py) held to cases worked out by hand, the corpus (links_cases.py) held to the
conditions its cases exist for, and the three host helpers of the binding held to hand-worked values.  No GPU.

The hand-made graph, K = 2 (edges are trinucleotides), from the strings CCAGATCT and TCAGATCT and their mirror images:

    rank  edge  segment          CCA --\\                       /--> TCA (3)
      0   AGA   0                (1)    CA -> CAG AGA -> GA -> GAT ATC -> TC
      1   ATC   2                TCA --/     (0)   ^           (2)      \\--> TCT CTG (4) -> TG -> TGA (5) -> GA
      2   CAG   0   entry 0      (3)               TGA (5)                                  \\-> TGG (6)
      3   CCA   1   entry 1
      4   CTG   4
      5   GAT   2   entry 2      node CA has two edges in and one out: the join.  CAG is the only edge out of CA, AGA
      6   TCA   3   entry 3      the only one out of AG, GAT out of GA, ATC out of AT: a read that comes in through CCA
      7   TCT   4   entry 4      is carried on segment 1 up to the fork at TC.
      8   TGA   5   entry 5
      9   TGG   6   entry 6
"""
import numpy as np
import pytest

import gossamer_amd as g
import links_cases as lc
import links_model as lm
import tips_model as tm
from gossamer_amd import (LINK_DTYPE, LINK_MISS, LINK_NONE, LINK_NON_UNIQUE, READ_LINKS_SYMBOLS,  # noqa: F401
                          estimate_coverage, filter_links, unique_segments)

K = 2
EDGES, COUNTS = tm.graph_of([("CCAGATCT", 1), ("TCAGATCT", 1)], K)
MISS = lm.MISS


def test_hand_graph_segments():
    assert [dg_text for dg_text in map(lambda e: "".join("ACGT"[(e >> (2 * (2 - i))) & 3] for i in range(3)), EDGES)] == \
        ["AGA", "ATC", "CAG", "CCA", "CTG", "GAT", "TCA", "TCT", "TGA", "TGG"]
    m = lm.Model(EDGES, K)
    assert m.starts == [2, 3, 5, 6, 7, 8, 9]
    assert m.seg_of == [0, 2, 0, 1, 4, 2, 3, 4, 5, 6]
    assert g.LINK_NONE == lm.NONE and g.LINK_MISS == lm.MISS and g.LINK_NON_UNIQUE == lm.NON_UNIQUE


def test_join_by_hand_both_tables():
    """CCAGATCT: windows CCA CAG AGA GAT ATC TCT.  Exact: 1 0 0 2 2 4.  Carry: CCA is looked up (1); CAG, AGA, GAT and
    ATC are each the only edge out of the node before them and take 1; TCT leaves the fork TC and is looked up (4)."""
    m = lm.Model(EDGES, K)
    read = "CCAGATCT\n"
    assert m.thread_windows(read, carry=False) == [1, 0, 0, 2, 2, 4]
    assert m.thread_windows(read, carry=True) == [1, 1, 1, 1, 1, 4]
    exact, ie = m.read_links([read], carry=False)
    carry, ic = m.read_links([read], carry=True)
    assert exact == {(1, 0): [1, 0], (0, 2): [1, 0], (2, 4): [1, 0]}
    assert carry == {(1, 4): [1, 0]}
    assert ie == dict(reads=1, windows=6, misses=0, carried=0, hits=6, records=3)
    assert ic == dict(reads=1, windows=6, misses=0, carried=4, hits=6, records=1)
    # segment 0 not unique, exact: 1 primes, two windows that are no hit, 2 closes (1, 2) with gap 2, then (2, 4)
    unique = [s != 0 for s in range(m.entries)]
    assert m.thread_windows(read, unique, carry=False) == [1, lm.NON_UNIQUE, lm.NON_UNIQUE, 2, 2, 4]
    assert m.read_links([read], unique, carry=False)[0] == {(1, 2): [1, 2], (2, 4): [1, 0]}


def test_carry_across_n_reset_and_miss_by_hand():
    m = lm.Model(EDGES, K)
    # CAG is the only edge out of to(CCA) = CA: the carry holds across the N; a new read looks it up
    assert m.thread_windows("CCANCAG\n", carry=True) == [1, 1]
    assert m.thread_windows("CCANCAG\n", carry=False) == [1, 0]
    assert m.thread_windows("CCA\nCAG\n", carry=True) == [1, 0]
    # CCAAGA: CCA, CAA and AAG (no edges), AGA: one record with the two misses as its gap, in either mode
    for carry in (False, True):
        assert m.thread_windows("CCAAGA\n", carry=carry) == [1, MISS, MISS, 0]
        table, info = m.read_links(["CCAAGA\n"], carry=carry)
        assert table == {(1, 0): [1, 2]} and info["misses"] == 2 and info["carried"] == 0
    # a hit on b itself changes nothing: 1 primes, 1 again (after the Ns), CAA AAC ACA miss, 0 closes with gap 3
    assert m.read_links(["CCANNCCAACAG\n"], carry=False)[0] == {(1, 0): [1, 3]}
    # lower case and '\r' and short reads and empty lines
    assert m.thread_windows("cCaGa\r\n\nCC\n", carry=False) == [1, 0, 0]
    assert m.read_links(["CCAGA", "\n", ""], carry=False)[1]["reads"] == 2
    # the sums are unbounded: 2^32 records of one link need no test, the model adds Python integers
    table, _ = m.read_links(["CCAGA\n" * 5], carry=False)
    assert table == {(1, 0): [5, 0]}


def test_cycle_has_no_segment():
    edges, _ = tm.graph_of([("ACAGAC", 1)], 2)                 # the circular string ACAG and its mirror CTGT: 8 edges,
    m = lm.Model(edges, 2)                                     # every node one in, one out
    assert len(edges) == 8 and m.entries == 0 and set(m.seg_of) == {lm.NONE}
    for carry in (False, True):
        assert m.thread_windows("ACAGACAG\n", carry=carry) == [MISS] * 6


@pytest.mark.parametrize("K", lc.PLANTED_K)
def test_planted_cases_hold_their_conditions(K):
    graph = lc.planted(K)
    m = lm.Model(graph["edges"], K)
    assert lm.NONE in m.seg_of                                  # the pure cycle
    names = set()
    for name, batches, pattern, condition in lc.planted_cases(K):
        assert name not in names and (pattern in lc.UNIQUE_PATTERNS or pattern[0] == "without")
        names.add(name)
        if name.startswith("one-link"):
            assert len(batches[0]) == lc.MANY * (K + 3)         # (the model's answer is the GPU test's business)
            continue
        assert condition(m, batches), (K, name)
    assert any(n.startswith("self-complementary") for n in names) == ((K + 1) % 2 == 0)


def test_dense_reads_hold_every_window():
    for k in range(1, 6):
        s = lc.de_bruijn(k + 1)
        assert len(s) == 4 ** (k + 1) + k and len(set(lm.windows_of(s, k))) == 4 ** (k + 1)
        whole, cut, odd = lc.dense_reads(k)
        assert set(lm.windows_of(whole.strip(), k)) == {w for r in cut.split("\n") for w in lm.windows_of(r, k)}
        assert "N" in odd and "n" in odd and "\r" in odd and "\n\n" in odd and any(c.islower() for c in odd)
    assert len(lc.dense_reads(5)[0]) > 2 * 2048                 # one read across three tiles
    corpus = lc.dense()
    assert len(corpus) == 40
    differ = 0
    for name, k, edges, counts, batches in corpus:
        m = lm.Model(edges, k)
        differ += m.read_links(batches, carry=True)[0] != m.read_links(batches, carry=False)[0]
    assert differ >= 10                                         # the carry decides the counts on dense graphs


# ---- the host helpers --------------------------------------------------------------------------------------------------

def test_unique_segments_by_hand():
    """f = ln 2 / 2 + (n / (2 rho)) (rho^2 - c^2 / 2).  rho = 2, c = 2: f = 0.3466 + n / 2: 4.85 at n = 9, 5.35 at n = 10.
    rho = 10, c = 10: f = 0.35 + 2.5 n, far above 5: only length + K decides, 49 against 50."""
    assert g.unique_segments([9, 10], [2, 2], 45, 2.0).tolist() == [False, True]
    assert g.unique_segments([22, 23], [10, 10], 27, 10.0).tolist() == [False, True]
    # c well above rho: the bracket is negative
    assert g.unique_segments([100], [30], 27, 10.0).tolist() == [False]
    # f = 5.0 exactly passes (>=): rho = 1, c = 0: f = k0 + n / 2 -> n such that ... no integer n gives 5.0; the float
    # expression itself, operation by operation:
    n, c, rho = np.float64(37.0), np.float64(3.0), np.float64(4.5)
    f = np.float64(np.log(2.0)) / 2.0 + (n / (2 * rho)) * (rho * rho - (c * c) / 2.0)
    assert g.unique_segments([37], [3], 27, 4.5).tolist() == [bool(f >= 5.0)]
    assert g.unique_segments([], [], 27, 10.0).tolist() == []


def test_estimate_coverage_by_hand():
    hist = {x: 1000 // x for x in range(1, 61)}                 # falling
    for x, y in ((18, 300), (19, 400), (20, 500), (21, 450)):
        hist[x] = y
    assert g.estimate_coverage(hist) == 20                      # the first rise is at 18; the largest y from there on
    assert g.estimate_coverage(sorted(hist.items())) == 20
    falling = {x: 1000 - x for x in range(1, 61)}
    assert g.estimate_coverage(falling) == 0                    # never rises: 0, not an error (the reference's)
    late = dict(falling)
    late[55] = 5000
    assert g.estimate_coverage(late) == 0                       # a peak beyond the fiftieth row is never seen
    gap = dict(hist)
    del gap[10]
    with pytest.raises(ValueError, match="discontinuous"):
        g.estimate_coverage(gap)
    gap = dict(hist)
    del gap[55]                                                 # a gap beyond the fiftieth row is not seen either
    assert g.estimate_coverage(gap) == 20
    with pytest.raises(ValueError, match="Not enough data"):
        g.estimate_coverage({x: 5 for x in range(1, 50)})


def test_filter_links_by_hand():
    table = np.array([(1, 2, 5, 10), (1, 3, 9, 9), (4, 3, 2, 7), (5, 6, 1, 100)], dtype=g.LINK_DTYPE)
    # one: (5, 6) goes; the others become count 1 with their average gap 2, 1, 3.  two: a = 1 keeps b = 2 (a tie among
    # counts of 1: the smallest id).  three: b = 3 has only (4, 3) left.
    got = g.filter_links(table, 2)
    assert got.tolist() == [(1, 2, 1, 2), (4, 3, 1, 3)]
    assert g.filter_links(table[:0], 1).tolist() == []
    # three alone: two rows into b = 7, the smaller a stays
    got = g.filter_links(np.array([(9, 7, 3, 3), (8, 7, 3, 6)], dtype=g.LINK_DTYPE), 1)
    assert got.tolist() == [(8, 7, 1, 2)]
