"""Pure-Python model of trim-paths and clip-links over a decoded edge list, in two forms each.

  *_serial   the reference's loop restated as it stands (GossCmdTrimPaths.cc:87-148,222; GossCmdClipLinks.cc:50-76,
             121-160; the walk is Graph::linearPath, Graph.tcc:19-46, unbounded): serial over the ranks, with clip-links'
             `seen` bitset, its two uint32 sums and its double division.  They return the survivors, the report, the
             estimate the reference's builder gets, and a marker where that estimate is undefined (zapCount > z).
  *_set      an order-free statement: the set of removed ranks as a function of the graph alone, with the integer
             form of the ratio test and a walk that gives up after 2K + 1 edges -- what the device computes.

Edges are (K+1)-mers as Python ints (tips_model.graph_of), the list sorted, every edge with its reverse complement.
"""
from bisect import bisect_left

from tips_model import graph_of, revcomp  # noqa: F401  (graph_of: for the callers)

U32 = 1 << 32
NO_EDGE = (1 << 64) - 1
PATHS_FIELDS = ("edges_before", "edges_after", "candidates", "paths", "zapped", "too_long", "spared_by_cutoff", "missing_rc")
LINKS_FIELDS = ("edges_before", "edges_after", "candidates", "links", "edges", "too_long", "major_out", "major_in", "missing_rc")
THIRD = 1.0 / 3.0


class Graph:
    def __init__(self, edges, counts, K):
        self.edges, self.counts, self.K, self.n = edges, counts, K, len(edges)
        self.node_mask = (1 << (2 * K)) - 1
        for i, e in enumerate(edges):                  # not a graph lint-graph passes: refused as a whole
            r = self.rank(revcomp(e, K + 1))
            if r >= self.n or edges[r] != revcomp(e, K + 1):
                raise ValueError("edge %d has no reverse complement in the graph" % i)

    def rank(self, e):
        return bisect_left(self.edges, e)

    def rc_rank(self, i):
        return self.rank(revcomp(self.edges[i], self.K + 1))

    def out_range(self, node):                         # ranks of the edges that leave `node`
        lo = bisect_left(self.edges, node << 2)
        hi = lo
        while hi < self.n and hi < lo + 4 and (self.edges[hi] >> 2) == node:
            hi += 1
        return lo, hi

    def out_deg(self, node):
        lo, hi = self.out_range(node)
        return hi - lo

    def in_deg(self, node):
        return self.out_deg(revcomp(node, self.K))

    def frm(self, i):
        return self.edges[i] >> 2

    def to(self, i):
        return self.edges[i] & self.node_mask

    def linear_path(self, beg, limit=None):
        """ranks of Graph::linearPath from rank `beg`; with `limit`, None once the path has more than `limit` edges"""
        path = []
        e = beg
        while True:
            lo, hi = self.out_range(self.to(e))
            if hi - lo != 1 or self.in_deg(self.to(e)) != 1:
                break
            if lo == beg:
                break
            path.append(e)
            if limit is not None and len(path) + 1 > limit:
                return None
            e = lo
        path.append(e)
        return path

    def in_ranks(self, node):
        """ranks of the edges that enter `node`, as minorIn finds them: the reverse complements of what leaves rc(node)"""
        lo, hi = self.out_range(revcomp(node, self.K))
        return [self.rc_rank(r) for r in range(lo, hi)]

    def survivors(self, zap):
        keep = [i for i in range(self.n) if i not in zap]
        return [self.edges[i] for i in keep], [self.counts[i] for i in keep]


def minor_double(c, s):
    """double(c) / double(s) < 1.0 / 3.0 with C++'s division: x / 0 is inf, 0 / 0 is NaN, neither is below a third"""
    if s == 0:
        return False
    return float(c) / float(s) < THIRD


def minor_int(c, s):
    return s != 0 and 3 * c < s


# ---- trim-paths ----------------------------------------------------------------------------------------------------------

def trim_paths_serial(edges, counts, K, cutoff=None):
    """(edges, counts, report, estimate, undefined): `estimate` is z - zapCount, what the reference's builder gets;
    where zapCount > z that is undefined, `undefined` is True and `estimate` is the exact number of survivors."""
    g = Graph(edges, counts, K)
    rep = dict.fromkeys(PATHS_FIELDS, 0)
    rep["edges_before"] = g.n
    rep["missing_rc"] = NO_EDGE
    zapped = set()
    for i in range(g.n):
        if g.in_deg(g.frm(i)) != 0:
            continue
        rep["candidates"] += 1
        path = g.linear_path(i)
        if len(path) > 2 * K:
            rep["too_long"] += 1
            continue
        if cutoff is not None and any(counts[r] >= cutoff for r in path):
            rep["spared_by_cutoff"] += 1
            continue
        zap_ranks = []
        for r in path:
            zap_ranks += [r, g.rc_rank(r)]
        zapped.update(zap_ranks)
        rep["paths"] += 1
        rep["zapped"] += len(zap_ranks)
    e2, c2 = g.survivors(zapped)
    rep["edges_after"] = len(e2)
    undefined = rep["zapped"] > g.n
    return e2, c2, rep, (len(e2) if undefined else g.n - rep["zapped"]), undefined


def trim_paths_set(edges, counts, K, cutoff=None):
    """(removed ranks, report): nothing here depends on an order"""
    g = Graph(edges, counts, K)
    starts = {i for i in range(g.n) if g.in_deg(g.frm(i)) == 0}
    paths = {i: g.linear_path(i, 2 * K) for i in starts}
    long = {i for i in starts if paths[i] is None}
    spared = {i for i in starts - long if cutoff is not None and max(counts[r] for r in paths[i]) >= cutoff}
    gone = starts - long - spared
    removed = {r for i in gone for r in paths[i]} | {g.rc_rank(r) for i in gone for r in paths[i]}
    rep = {"edges_before": g.n, "edges_after": g.n - len(removed), "candidates": len(starts), "paths": len(gone),
           "zapped": sum(2 * len(paths[i]) for i in gone), "too_long": len(long), "spared_by_cutoff": len(spared),
           "missing_rc": NO_EDGE}
    return removed, rep


# ---- clip-links ----------------------------------------------------------------------------------------------------------

def clip_links_serial(edges, counts, K, use_seen=True, ratios=None):
    """(edges, counts, report, estimate): the estimate is z, for numZapped is never updated.  `ratios`: a set that
    collects every (c, s) the two tests were asked about.  A start that fails several tests is counted under the first it
    fails in the order length, fork, join (the reference evaluates fork, join, length, all without side effects)."""
    g = Graph(edges, counts, K)
    rep = dict.fromkeys(LINKS_FIELDS, 0)
    rep["edges_before"] = g.n
    rep["missing_rc"] = NO_EDGE
    seen = [False] * g.n
    zap = set()
    for i in range(g.n):
        if use_seen and seen[i]:
            continue
        lo, hi = g.out_range(g.frm(i))
        if hi - lo == 1:
            continue
        rep["candidates"] += 1
        ranks = g.linear_path(i)
        for r in ranks:
            seen[r] = True
        c_f, c_t = counts[i], counts[ranks[-1]]
        c_out_sum = 0
        for r in range(lo, hi):
            c_out_sum = (c_out_sum + counts[r]) % U32
        c_in_sum = 0
        for r in g.in_ranks(g.to(ranks[-1])):
            c_in_sum = (c_in_sum + counts[r]) % U32
        if ratios is not None:
            ratios.update([(c_f, c_out_sum), (c_t, c_in_sum)])
        minor_out, minor_in, short = minor_double(c_f, c_out_sum), minor_double(c_t, c_in_sum), len(ranks) <= 2 * K
        if minor_out and minor_in and short:
            rep["links"] += 1
            rep["edges"] += len(ranks)
            for r in ranks:
                zap.add(r)
                zap.add(g.rc_rank(r))
        elif not short:
            rep["too_long"] += 1
        elif not minor_out:
            rep["major_out"] += 1
        else:
            rep["major_in"] += 1
    e2, c2 = g.survivors(zap)
    rep["edges_after"] = len(e2)
    return e2, c2, rep, g.n


def clip_links_set(edges, counts, K):
    """(removed ranks, report): nothing here depends on an order"""
    g = Graph(edges, counts, K)

    def group_sum(ranks):
        return sum(counts[r] for r in ranks) % U32

    starts = {i for i in range(g.n) if g.out_deg(g.frm(i)) >= 2}
    paths = {i: g.linear_path(i, 2 * K) for i in starts}
    long = {i for i in starts if paths[i] is None}
    major_out = {i for i in starts - long if not minor_int(counts[i], group_sum(range(*g.out_range(g.frm(i)))))}
    major_in = {i for i in starts - long - major_out
                if not minor_int(counts[paths[i][-1]], group_sum(g.in_ranks(g.to(paths[i][-1]))))}
    gone = starts - long - major_out - major_in
    removed = {r for i in gone for r in paths[i]} | {g.rc_rank(r) for i in gone for r in paths[i]}
    rep = {"edges_before": g.n, "edges_after": g.n - len(removed), "candidates": len(starts), "links": len(gone),
           "edges": sum(len(paths[i]) for i in gone), "too_long": len(long), "major_out": len(major_out),
           "major_in": len(major_in), "missing_rc": NO_EDGE}
    return removed, rep


def survivors_of(edges, counts, removed):
    keep = [i for i in range(len(edges)) if i not in removed]
    return [edges[i] for i in keep], [counts[i] for i in keep]
