"""The exact model of count-components, in pure Python (GossCmdCountComponents.cc:37-127, 171-311).

A union-find over NODES keyed by K-mer value: every marked edge unions its from-node and its to-node, and the
component of an edge is the class of its from-node.  That is deliberately another formulation than the device's
edge-to-edge hooks over the link arrays.  The table holds the TRUE figures; reference_table() restates the rows the
reference prints, which count the start edge of every component twice.
"""
import math

from tips_model import revcomp

NONE = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def components(edges, counts, K, marked=None):
    """(labels, table): labels[i] = index of the component of edge i (NONE where unmarked), components numbered by
    ascending smallest rank; table[c] = (start, edges, min, max, s, s2, mirror), s and s2 modulo 2^64, mirror = the
    component of rc(start edge), NONE when that edge is unmarked."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1
    on = [True] * n if marked is None else [bool(m) for m in marked]
    parent = {}
    for i, e in enumerate(edges):
        if not on[i]:
            continue
        a, b = e >> 2, e & node_mask
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[ra] = rb
    index = {}                                   # root node -> component index, in order of first appearance by rank
    labels = [NONE] * n
    rows = []
    for i, e in enumerate(edges):
        if not on[i]:
            continue
        r = _find(parent, e >> 2)
        if r not in index:
            index[r] = len(rows)
            rows.append([i, 0, NONE, 0, 0, 0, NONE])
        c = index[r]
        labels[i] = c
        row = rows[c]
        m = counts[i]
        row[1] += 1
        row[2] = min(row[2], m)
        row[3] = max(row[3], m)
        row[4] = (row[4] + m) & MASK64
        row[5] = (row[5] + m * m) & MASK64
    rank = {e: i for i, e in enumerate(edges)}
    for row in rows:
        row[6] = labels[rank[revcomp(edges[row[0]], K + 1)]]
    return labels, [tuple(r) for r in rows]


def marks(edges, K, reads_text):
    """(marked, windows, hits): every forward (K+1)-window of the text (ACGTacgt only; any other byte, a newline
    included, restarts the window) looked up among the edges -- no reverse complement, no normalisation."""
    rank = {e: i for i, e in enumerate(edges)}
    marked = [False] * len(edges)
    L = K + 1
    mask = (1 << (2 * L)) - 1
    windows = hits = 0
    run = v = 0
    if isinstance(reads_text, bytes):
        reads_text = reads_text.decode("latin-1")
    for ch in reads_text:
        code = "ACGT".find(ch.upper()) if ch in "ACGTacgt" else -1
        if code < 0:
            run = v = 0
            continue
        v = ((v << 2) | code) & mask
        run += 1
        if run >= L:
            windows += 1
            i = rank.get(v)
            if i is not None:
                hits += 1
                marked[i] = True
    return marked, windows, hits


def reference_table(table, counts):
    """The bytes `goss count-components` prints: the start edge of every component counted twice
    (GossCmdCountComponents.cc:252-255), doubles as the stream prints them ('%g')."""
    out = ["Comp\tSize\tMin\tMax\tMean\tStd Dev\n"]
    for i, (start, n, lo, hi, s, s2, _) in enumerate(table):
        m = counts[start]
        size, s, s2 = n + 1, (s + m) & MASK64, (s2 + m * m) & MASK64
        mean = s / float(size)
        std = math.sqrt(float(size) * s2 - float(s) * s) / size
        out.append("%d\t%d\t%d\t%d\t%g\t%g\n" % (i, size, lo, hi, mean, std))
    return "".join(out).encode()


def keep(edges, counts, K, rank):
    """(edges, counts) of the whole-graph component of the edge of that rank and of its reverse complement: what -O
    writes for the start of the first component (GossCmdCountComponents.cc:270-309)."""
    labels, _ = components(edges, counts, K)
    other = edges.index(revcomp(edges[rank], K + 1))
    want = {labels[rank], labels[other]}
    sel = [i for i in range(len(edges)) if labels[i] in want]
    return [edges[i] for i in sel], [counts[i] for i in sel]
