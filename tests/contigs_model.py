"""Pure-Python model of print-contigs in its linear-segments form over a decoded edge list.

Written from the semantics of the reference's command (printLinearSegments, GossCmdPrintContigs.cc:49-193;
Graph::linearPath, Graph.tcc:21-46), not from its text: the sequential loop over the ranks with its `seen` bitmap,
literally.  Edges are (K+1)-mers as Python ints, first base in the most significant used bits; the list is sorted and
every edge has its reverse complement in it (tips_model.graph_of builds such lists).
"""
import math
from bisect import bisect_left

from tips_model import revcomp

FNV_SEED = 14695981039346656037
FNV_PRIME = 1099511628211
MASK64 = (1 << 64) - 1

TABLE_FIELDS = ("first_rank", "edges", "min", "max", "s", "s2", "include_fst", "include_lst", "len", "end_rank")


def fnv(v):
    """FNV-1a-64 of the 16 little-endian bytes of a position (the order position_type::normalize goes by)"""
    h = FNV_SEED
    for b in v.to_bytes(16, "little"):
        h = ((h ^ b) * FNV_PRIME) & MASK64
    return h


def normalize(v, k):
    """whichever of a k-mer and its reverse complement hashes lower; on a tie the smaller value"""
    r = revcomp(v, k)
    hv, hr = fnv(v), fnv(r)
    if hv > hr or (hv == hr and r < v):
        return r
    return v


def fmt_double(x):
    """a double as a C++ ostream prints it by default: six significant digits, %g"""
    return "%g" % x


def mean_sd(s, s2, m):
    a = float(s) / m
    rad = float(s2) / m - a * a
    # a negative radicand would print "-nan" in the reference; with multiplicities below 2^26 a variance that is not
    # zero is at least 1 / m^2 and the doubles hold every term exactly enough: the model's inputs never get there
    assert rad >= 0.0, (s, s2, m)
    return a, math.sqrt(rad)


class Segment(dict):
    __getattr__ = dict.__getitem__


def linear_segments(edges, counts, K, min_length=0, min_coverage=0, print_rcs=False):
    """(segments in printing order, info).  A segment holds TABLE_FIELDS, `bases` (the text it prints), `full` (all
    edges + K bases of its path) and `ranks` (the path).
    info: starts, taken (starts the loop did not skip, before the filters), seen (the bitmap when the loop ends),
    rule_ok (the per-path rule i <= rank(rc(end)) agreed with the bitmap at every start), longest (edges)."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1

    def out_range(node):
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
        r = bisect_left(edges, e)
        assert r < n and edges[r] == e
        return r

    for i, e in enumerate(edges):
        r = bisect_left(edges, revcomp(e, K + 1))
        if r >= n or edges[r] != revcomp(e, K + 1):
            raise ValueError("edge %d has no reverse complement in the graph" % i)

    seen = [False] * n
    segs = []
    info = {"starts": 0, "taken": 0, "rule_ok": True, "longest": 0}
    for i in range(n):
        e = edges[i]
        e_f = e >> 2
        if in_deg(e_f) == 1 and out_deg(e_f) == 1:
            continue
        info["starts"] += 1
        # Graph::linearPath: onward while the node reached has one edge out and one in
        path = [i]
        x = e
        while True:
            to = x & node_mask
            lo, hi = out_range(to)
            if hi - lo != 1 or in_deg(to) != 1:
                break
            if edges[lo] == e:
                break
            x = edges[lo]
            path.append(lo)
        info["longest"] = max(info["longest"], len(path))
        end = path[-1]
        end_rc = rank(revcomp(edges[end], K + 1))
        if (i <= end_rc) != (not seen[i]):
            info["rule_ok"] = False
        if seen[i]:
            continue
        info["taken"] += 1
        assert not seen[end_rc]
        seen[i] = True
        seen[end_rc] = True
        for r in path:
            seen[r] = True
            if not print_rcs:
                seen[rank(revcomp(edges[r], K + 1))] = True
        m = len(path)
        ws = [counts[r] for r in path]
        fst = edges[path[0]] >> 2
        lst = edges[end] & node_mask
        include_fst = in_deg(fst) == 0 or normalize(fst, K) == fst
        include_lst = out_deg(lst) == 0 or normalize(lst, K) != lst
        length = m + K
        if length >= K and not include_fst:
            length -= K
        if length >= K and not include_lst:
            length -= K
        if not (length >= min_length and min(ws) >= min_coverage):
            continue
        e0 = edges[path[0]]
        full = "".join("ACGT"[(e0 >> (2 * (K - b))) & 3] for b in range(K + 1))
        full += "".join("ACGT"[edges[r] & 3] for r in path[1:])
        assert len(full) == m + K
        skip = 0 if include_fst else K
        segs.append(Segment(first_rank=i, edges=m, min=min(ws), max=max(ws), s=sum(ws) & MASK64,
                            s2=sum(w * w for w in ws) & MASK64, include_fst=include_fst, include_lst=include_lst,
                            len=length, end_rank=end, bases=full[skip:skip + length], full=full, ranks=path))
    info["seen"] = seen
    return segs, info


def body(bases, line_breaks=True):
    """the lines of one segment: 60 bases each, every line (the last, partial one too) ended by a line feed; nothing
    for an empty segment"""
    if not bases:
        return ""
    if not line_breaks:
        return bases + "\n"
    return "".join(bases[i:i + 60] + "\n" for i in range(0, len(bases), 60))


def stats(seg, K):
    a, d = mean_sd(seg.s, seg.s2, seg.edges)
    return (seg.edges + K, seg.min, seg.max, fmt_double(a), fmt_double(d))


def render(segs, K, verbose_headers=False, line_breaks=True, sequence=True):
    """the bytes the command writes"""
    out = []
    if not sequence:
        out.append("Number\tLength\tMinCov\tMaxCov\tMeanCov\tStdDevCov\n")
    for no, seg in enumerate(segs, 1):
        if not sequence:
            out.append("%d\t%d\t%d\t%d\t%s\t%s\n" % ((no,) + stats(seg, K)))
            continue
        out.append(">%d" % no)
        if verbose_headers:
            out.append(" %d:%d:%d:%s:%s" % stats(seg, K))
        out.append("\n")
        out.append(body(seg.bases, line_breaks))
    return "".join(out).encode()


def text_of(segs, line_breaks=True):
    """the bodies back to back: what the device holds as the text"""
    return "".join(body(s.bases, line_breaks) for s in segs).encode()
