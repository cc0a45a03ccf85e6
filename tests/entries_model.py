"""Pure-Python model of build-entry-edge-set over a decoded edge list.

Written from the semantics of the reference's command (EntryEdgeSet::build, EntryEdgeSet.cc:154-287; the walk is
Graph::linearPath, Graph.tcc:19-46), not from its text.  Edges are (K+1)-mers as Python ints, first base in the most
significant used bits; the list is sorted and every edge has its reverse complement in it (tips_model.graph_of builds
such lists).  The multiplicities are taken as given: an edge and its reverse complement may carry different ones.

  entry edge   in(from(e)) != 1 or out(from(e)) != 1; E_0 .. E_{n-1} in rank order
  len_j        edges of the linear path that starts at E_j (onward while the node reached has one edge out and one in)
  cnt_j        (uint32) round(double(sum of the path's multiplicities) / double(len_j)), half away from zero
  ends_j       the number among the entries of the reverse complement of the path's last edge
"""
import math
import struct
from bisect import bisect_left
from collections import Counter

import numpy as np

VERSION = 2011041901
BASE = "-entries"

# reverse complement of the four bases of one byte
_RC_BYTE = bytes(((3 - (b & 3)) << 6) | ((3 - ((b >> 2) & 3)) << 4) | ((3 - ((b >> 4) & 3)) << 2) | (3 - (b >> 6)) for b in range(256))


def revcomp(x, length):
    """tips_model.revcomp, a byte at a time"""
    nbytes = (2 * length + 7) // 8
    r = int.from_bytes(x.to_bytes(nbytes, "little").translate(_RC_BYTE), "big")
    return r >> (8 * nbytes - 2 * length)


def round_half_away(x):
    """boost::math::round of a non-negative double"""
    if x < 0.5:
        return 0
    c = math.ceil(x)                 # (c - x is exact from 0.5 on)
    return c - 1 if c - x > 0.5 else c


def entry_edge_set(edges, counts, K):
    """dict(starts, cnt, len, ends, hist, end_edges, cycle_edges, longest): starts are the entry edges' ranks in the
    graph; hist maps cnt to its number of entries; end_edges are the ranks of the paths' last edges."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1
    rc_rank = [0] * n
    for i, e in enumerate(edges):
        rc = revcomp(e, K + 1)
        r = bisect_left(edges, rc)
        if r >= n or edges[r] != rc:
            raise ValueError("edge %d has no reverse complement in the graph" % i)
        rc_rank[i] = r
    # every edge has its mirror image, so in(node) = out(rc(node)) is the number of edges that arrive at the node
    out_deg = Counter(e >> 2 for e in edges)
    in_deg = Counter(e & node_mask for e in edges)

    def plain(node):
        return in_deg.get(node, 0) == 1 and out_deg.get(node, 0) == 1

    starts = [i for i, e in enumerate(edges) if not plain(e >> 2)]
    number = {r: j for j, r in enumerate(starts)}
    cnt, length, ends, end_edges = [], [], [], []
    on_path = 0
    for i in starts:
        x, m, s = i, 1, counts[i]
        while True:
            to = edges[x] & node_mask
            if not plain(to):
                break
            nx = bisect_left(edges, to << 2)
            if nx == i:
                break
            x = nx
            m += 1
            s += counts[x]
        on_path += m
        length.append(m)
        cnt.append(round_half_away(float(s) / float(m)) & 0xFFFFFFFF)
        end_edges.append(x)
        ends.append(number[rc_rank[x]])
    hist = dict(sorted(Counter(cnt).items()))
    return dict(starts=starts, cnt=cnt, len=length, ends=ends, hist=hist, end_edges=end_edges,
                cycle_edges=n - on_path, longest=max(length, default=0))


def file_set(oracle, edges, K, model, base=BASE):
    """{name: bytes} of the object: the names as on disk less the graph's name"""
    n = len(model["starts"])
    out = {}
    z = 1 << (2 * (K + 1))
    for name, data in oracle.write_sparse_array([edges[r] for r in model["starts"]], z, n, base="x").items():
        out[base + ".edges" + name[1:]] = data
    for col, key in ((".counts", "cnt"), (".lengths", "len")):
        for name, data in oracle.write_vba(model[key], n, base="x").items():
            out[base + col + name[1:]] = data
    out[base + ".counts-hist.txt"] = "".join("%d\t%d\n" % kv for kv in model["hist"].items()).encode()
    ends = np.asarray(model["ends"], dtype=np.uint64)
    out[base + ".ends.upr"] = (ends >> np.uint64(32)).astype(np.uint8).tobytes()
    out[base + ".ends.lwr"] = (ends & np.uint64(0xFFFFFFFF)).astype("<u4").tobytes()
    out[base + ".header"] = struct.pack("<QQ", VERSION, K)
    return out


def expected(oracle, edges, counts, K, base=BASE):
    """(model, files)"""
    model = entry_edge_set(edges, counts, K)
    return model, file_set(oracle, edges, K, model, base)

