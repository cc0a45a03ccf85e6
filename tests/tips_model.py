"""Pure-Python model of trim-graph -C and of one prune-tips iteration over a decoded edge list.

Written from the semantics of the reference's commands (GossCmdPruneTips.cc:82-225, Graph::linearPath,
GossCmdTrimGraph.cc:97-124), not from their text.  Edges are (K+1)-mers as Python ints, first base in the
most significant used bits; the list is sorted and every edge has its reverse complement in it.
"""
from bisect import bisect_left

REPORT_FIELDS = ("edges_before", "edges_after", "candidates", "tips", "zapped", "too_long", "both_joined", "isolated",
                 "outweighed", "joined_at_begin", "joined_at_end")


def revcomp(x, length):
    r = 0
    for _ in range(length):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def encode(text):
    v = 0
    for ch in text:
        v = (v << 2) | "ACGT".index(ch)
    return v


def trim(edges, counts, cutoff):
    keep = [i for i, c in enumerate(counts) if c > cutoff]
    return [edges[i] for i in keep], [counts[i] for i in keep]


def prune_once(edges, counts, K):
    """One iteration: (surviving edges, their counts, report).  All decisions are taken against the graph as given."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1

    def out_range(node):                     # ranks of the edges that leave `node`
        lo = bisect_left(edges, node << 2)
        hi = lo
        while hi < n and hi < lo + 4 and (edges[hi] >> 2) == node:
            hi += 1
        return lo, hi

    def out_deg(node):
        lo, hi = out_range(node)
        return hi - lo

    def in_deg(node):
        return out_deg(revcomp(node, K))

    def rank(e):
        return bisect_left(edges, e)

    # not a graph lint-graph passes: refused as a whole, naming the first offending edge
    for i, e in enumerate(edges):
        r = rank(revcomp(e, K + 1))
        if r >= n or edges[r] != revcomp(e, K + 1):
            raise ValueError("edge %d has no reverse complement in the graph" % i)

    rep = dict.fromkeys(REPORT_FIELDS, 0)
    rep["edges_before"] = n
    zap = set()
    for beg in edges:
        if in_deg(beg >> 2) != 0:
            continue
        rep["candidates"] += 1
        path = [beg]
        e = beg
        long = False
        while True:
            to = e & node_mask
            lo, hi = out_range(to)
            if hi - lo != 1 or in_deg(to) != 1:
                break
            nxt = edges[lo]
            if nxt == beg:
                break
            e = nxt
            path.append(e)
            if len(path) > 2 * K:
                long = True
                break
        if long:
            rep["too_long"] += 1
            continue
        end = path[-1]
        beg_con = out_deg(beg >> 2) > 1
        end_to = end & node_mask
        end_con = in_deg(end_to) > 1 or out_deg(end_to) > 0
        if beg_con and end_con:
            rep["both_joined"] += 1
            continue
        if not beg_con and not end_con:
            rep["isolated"] += 1
            continue
        if end_con:
            c, node = counts[rank(end)], revcomp(end_to, K)
        else:
            c, node = counts[rank(beg)], beg >> 2
        lo, hi = out_range(node)
        if any(counts[j] < c for j in range(lo, hi)):
            rep["outweighed"] += 1
            continue
        rep["tips"] += 1
        rep["zapped"] += 2 * len(path)
        rep["joined_at_end" if end_con else "joined_at_begin"] += 1
        for x in path:
            zap.add(rank(x))
            zap.add(rank(revcomp(x, K + 1)))
    keep = [i for i in range(n) if i not in zap]
    rep["edges_after"] = len(keep)
    return [edges[i] for i in keep], [counts[i] for i in keep], rep


def prune(edges, counts, K, iterations):
    """[(edges, counts, report)] after each of `iterations` rounds."""
    out = []
    for _ in range(iterations):
        edges, counts, rep = prune_once(edges, counts, K)
        out.append((edges, counts, rep))
    return out


def graph_of(strings, K):
    """Sorted (edges, counts) of the graph that holds every (K+1)-mer of the given (text, multiplicity) strings and its
    reverse complement.  No (K+1)-mer may come from two places with different multiplicities."""
    got = {}
    for text, mult in strings:
        for i in range(len(text) - K):
            e = encode(text[i:i + K + 1])
            for x in (e, revcomp(e, K + 1)):
                if got.setdefault(x, mult) != mult:
                    raise ValueError("edge %s given with two multiplicities" % text[i:i + K + 1])
    edges = sorted(got)
    return edges, [got[e] for e in edges]
