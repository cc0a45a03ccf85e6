"""The exact model of build-subgraph's growth, in pure Python (GossCmdBuildSubgraph.cc:95-212).

The order-free statement over Python sets of edge VALUES ((K+1)-mers as ints; from(e) = e >> 2, to(e) = e & mask(2K)):
no ranks, no link arrays, no scan order.  test_subgraph_cpu.py pins it to the reference's own loop restated literally;
the device is checked against it.

  start   I = the marked edges and their reverse complements
  node    P = I; per pass F = the edges outside I that leave to(e) or enter from(e) for an e of P; I |= F; P = F;
          logged: |F|
  linear  a segment is a class of the edges joined through nodes with exactly one edge in and one out.  Per pass S =
          the segments that hold an edge of P and their mirror segments; I |= S; F = the edges outside I that leave
          to(s) or enter from(s) for an s of S; I |= F; P = F; logged: the growth of I
"""
from tips_model import revcomp


def _adjacency(edges, K):
    node_mask = (1 << (2 * K)) - 1
    out, into = {}, {}
    for e in edges:
        out.setdefault(e >> 2, []).append(e)
        into.setdefault(e & node_mask, []).append(e)
    return node_mask, out, into


def segments(edges, K):
    """{edge: frozenset of the edges of its segment}"""
    _, out, into = _adjacency(edges, K)
    parent = {e: e for e in edges}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for node, leaving in out.items():
        entering = into.get(node, [])
        if len(leaving) == 1 and len(entering) == 1:
            a, b = find(entering[0]), find(leaving[0])
            if a != b:
                parent[a] = b
    members = {}
    for e in edges:
        members.setdefault(find(e), set()).add(e)
    return {e: frozenset(members[find(e)]) for e in edges}


def start_set(edges, K, marked):
    got = set()
    for e, m in zip(edges, marked):
        if m:
            got.add(e)
            got.add(revcomp(e, K + 1))
    return got


def grow_steps(edges, K, marked, radius, linear_paths=False):
    """yields (marks as a list of bools in rank order, logged number) after the start set (None) and after every pass"""
    node_mask, out, into = _adjacency(edges, K)
    seg = segments(edges, K) if linear_paths else None
    I = start_set(edges, K, marked)
    assert I <= set(edges)
    yield [e in I for e in edges], None
    P = set(I)
    for _ in range(radius):
        before = len(I)
        if linear_paths:
            S = set()
            for e in P:
                S |= seg[e]
                S |= seg[revcomp(e, K + 1)]
            I |= S
            P = S
        F = set()
        for e in P:
            for f in out.get(e & node_mask, []) + into.get(e >> 2, []):
                if f not in I:
                    F.add(f)
        I |= F
        P = F
        yield [e in I for e in edges], len(I) - before


def grow(edges, K, marked, radius, linear_paths=False):
    """(marks after the last pass as a list of bools in rank order, [logged number of every pass])"""
    steps = list(grow_steps(edges, K, marked, radius, linear_paths))
    return steps[-1][0], [s[1] for s in steps[1:]]


def subgraph(edges, counts, K, marked, radius, linear_paths=False):
    """(edges, counts, added) of what build-subgraph writes"""
    marks, added = grow(edges, K, marked, radius, linear_paths)
    sel = [i for i, m in enumerate(marks) if m]
    return [edges[i] for i in sel], [counts[i] for i in sel], added
