"""Pure-Python model of `translucent trim-relative` and `translucent merge-graph-with-reference` over decoded edge lists.

Written from the semantics of the reference's commands (TransCmdTrimRelative.cc:81-280,
TransCmdMergeGraphWithReference.cc:43-110), not from their text.  Edges are (K+1)-mers as Python ints, first base in the
most significant used bits; a list is sorted, so the edges that leave one node (edge >> 2) are adjacent, at most four.

trim-relative is stated twice.  zapped_serial() is the reference's loop as it stands: J blocks of ranks that start at
beginRank(from(select(i * (N / J)))), each walked in rank order with the running node and its counts, processNode on
every node with two or more out-edges.  trim_relative() is the order-free statement the device computes: per node
group, then the mirror closure.  test_relative_cpu.py holds the two equal for J = 1, 2, 3, 4, 7 and J > N on every case:
the blocks start at the first edge of a node, so no group is cut and J decides nothing.

Where the reference and this build part (both models follow this build):
  * an empty graph gives the empty graph (the reference calls select(0) on it);
  * an edge below its threshold whose reverse complement is absent refuses the whole pass, naming the lowest such
    rank (the reference sets the bit at the rank the absent edge would have, another edge's or one past the end).
"""
from bisect import bisect_left
from itertools import groupby

import tips_model as tm

REPORT_FIELDS = ("edges_before", "edges_after", "forks", "below", "mirror_only")
RECOUNT_FIELDS = ("edges_before", "edges_after")
DEFAULT_REL = 0.02


def is_below(count, total, rel):
    """processNode's test, `pCounts[i] < totalCount * mRelCoverage`: the uint64_t sum becomes a double, one
    multiplication, the uint32_t count becomes a double, one strict comparison"""
    return float(count) < float(total) * rel


def mirror_rank(edges, K, r):
    """rank(reverseComplement(select(r))), or the refusal"""
    rc = tm.revcomp(edges[r], K + 1)
    q = bisect_left(edges, rc)
    if q >= len(edges) or edges[q] != rc:
        raise ValueError("edge %d has no reverse complement in the graph" % r)
    return q


# ---- the loop as it stands ---------------------------------------------------------------------------------------------

def zapped_serial(edges, counts, K, rel, J):
    """The set of ranks the reference's J threads zap, the blocks run one after the other."""
    N = len(edges)
    zapped = set()
    if N == 0:
        return zapped

    def process_node(node_begin, cnts):
        total = sum(cnts)
        cull = [node_begin + i for i, c in enumerate(cnts) if is_below(c, total, rel)]
        if not cull:
            return
        for r in list(cull):
            cull.append(mirror_rank(edges, K, r))
        zapped.update(cull)

    def block(begin, end):
        i = begin
        node_begin = node_end = i
        cnts = [counts[i]]
        cur_node = edges[i] >> 2
        i += 1
        while i < end:
            cur_rank = i
            i += 1
            cur_count = counts[cur_rank]
            node_end = cur_rank
            next_node = edges[cur_rank] >> 2
            if next_node == cur_node:
                cnts.append(cur_count)
                continue
            if len(cnts) <= 1:                           # only one out edge
                cur_node = next_node
                node_begin = node_end
                cnts = [cur_count]
                continue
            process_node(node_begin, cnts)
            cur_node = next_node
            node_begin = node_end
            cnts = [cur_count]
        if len(cnts) > 1:
            process_node(node_begin, cnts)

    S = N // J
    starts = [bisect_left(edges, (edges[i * S] >> 2) << 2) for i in range(J)] + [N]       # beginRank(from(select(i * S)))
    for b, e in zip(starts, starts[1:]):
        if b != e:
            block(b, e)
    return zapped


# ---- the order-free statement ------------------------------------------------------------------------------------------

def judge(edges, counts, rel):
    """(ranks below their own node's threshold, number of forks): per group of equal from-nodes of two or more edges"""
    below, forks = set(), 0
    for _, grp in groupby(range(len(edges)), key=lambda r: edges[r] >> 2):
        ranks = list(grp)
        if len(ranks) < 2:
            continue
        forks += 1
        total = sum(counts[r] for r in ranks)
        below.update(r for r in ranks if is_below(counts[r], total, rel))
    return below, forks


def trim_relative(edges, counts, K, rel=DEFAULT_REL):
    """(surviving edges, their counts, report, the estimate the builder gets): the set below, closed under the mirror
    image; the estimate is the exact survivor count, N - zapped.count()"""
    n = len(edges)
    below, forks = judge(edges, counts, rel)
    zap = set(below)
    for r in sorted(below):
        zap.add(mirror_rank(edges, K, r))
    keep = [i for i in range(n) if i not in zap]
    rep = {"edges_before": n, "edges_after": len(keep), "forks": forks, "below": len(below), "mirror_only": len(zap) - len(below)}
    return [edges[i] for i in keep], [counts[i] for i in keep], rep, len(keep)


# ---- merge-graph-with-reference ------------------------------------------------------------------------------------------

def merge_with_reference(in_edges, in_counts, ref_edges, ref_counts):
    """(edges, counts, report, the estimate the builder gets): the edges of graph-in that graph-ref holds, with
    graph-ref's multiplicities; Graph::Builder(K, out, fac, itr.count()) -- the input's edge count, not the output's"""
    ref = dict(zip(ref_edges, ref_counts))
    out = [(e, ref[e]) for e in in_edges if e in ref]
    rep = {"edges_before": len(in_edges), "edges_after": len(out)}
    return [e for e, _ in out], [c for _, c in out], rep, len(in_edges)


def merge_serial(in_edges, in_counts, ref_edges, ref_counts):
    """The reference's two iterators as they stand (TransCmdMergeGraphWithReference.cc:79-105): (edges, counts)"""
    out_e, out_c = [], []
    i = j = 0
    ref_valid = j < len(ref_edges)
    while i < len(in_edges) and ref_valid:
        edge = in_edges[i]
        while ref_edges[j] < edge:
            j += 1
            ref_valid = j < len(ref_edges)
            if not ref_valid:
                break
        if ref_valid and ref_edges[j] == edge:
            out_e.append(ref_edges[j])
            out_c.append(ref_counts[j])
            j += 1
            ref_valid = j < len(ref_edges)
        i += 1
    return out_e, out_c
