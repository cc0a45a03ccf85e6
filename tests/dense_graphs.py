"""Dense graphs at K = 1 .. 5 for the graph pass tests: random symmetric subsets of all 4^(K+1) edges, and a few planted
graphs whose structure is the point.

At these K every degenerate local structure that the hand-made pieces of tips_cases.py plant one at a time occurs in
almost every graph: nodes that are their own reverse complement (even K), edges that are (odd K), self-loops,
two-cycles, nodes with four edges on both sides, tips that overlap, and edge counts at which the last word of a bitmap
is full, missing or one bit long.  The graphs are the smallest on which the link pass, the list ranking and the
union-find can still go wrong: 1 to 4 096 edges.

Everything here is plain Python and deterministic.  test_dense_graphs_cpu.py holds the corpus to what it claims;
test_gpu_dense_graphs.py runs every pass of the device over it.

How the seeds below were chosen.  find_seeds() (not run at import, a few seconds by hand) walks seed = 0, 1, 2, ... for
every (K, density) of _RANDOM and keeps the first seed whose graph has the wanted number of edges -- the six counts
around a 32-bit and a 64-bit word come from K = 3 (an odd count needs an odd number of self-complementary edges, hence
odd K) and 32 from K = 2, straight from seed and density, without trimming -- and, for the rows that name one, the
wanted property: `too_long`, a tip candidate of the first prune-tips iteration that walks more than 2K edges, which at
density 0.1 one graph in a few dozen has; `cycle`, edges on a cycle that no entry edge leads into; `uneven`,
joined_at_begin != joined_at_end in the first iteration; `second`, iteration 2 removes a
tip).  No graph of the corpus is emptied by pruning: a dense graph always keeps a branching core, and of the planted
ones the lone paths are `isolated`, which prune-tips leaves alone.
"""
import random

import components_model as cpm
import entries_model as em
import tips_model as tm

MAX_GRAPHS = 40
MAX_EDGES = 4096


def text_of(e, length):
    return "".join("ACGT"[(e >> (2 * (length - 1 - i))) & 3] for i in range(length))


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def random_graph(K, density, seed, max_count=6):
    """Sorted (edges, counts): every edge e <= rc(e) of the 4^(K+1) taken with probability `density`, one multiplicity
    of 1 .. max_count drawn per pair and given to both strands."""
    rng = random.Random(seed * 1000003 + K * 101 + int(density * 1000))
    got = {}
    for e in range(1 << (2 * (K + 1))):
        r = tm.revcomp(e, K + 1)
        if e <= r and rng.random() < density:
            got[e] = got[r] = rng.randint(1, max_count)
    edges = sorted(got)
    return edges, [got[e] for e in edges]


def planted(K):
    """[(name, [(text, multiplicity)])] for tips_model.graph_of:
    homopolymer   A x (K + 3): one self-loop per strand, n = 2
    acac          ACAC.. of 2(K + 1) bases: a two-cycle and its mirror image
    atat          ATAT.. of 2(K + 1) bases: a two-cycle that is its own mirror image
    tail          A x (K + 2) + C + G x (K + 1): a self-loop that runs into a path that ends in the mirror self-loop
    lone          K + 1 even: u + rc(u) with |u| = (K + 1) / 2, one edge that is its own reverse complement, n = 1
    complete      K <= 4: all 4^(K+1) edges, one string per strand pair"""
    out = [("homopolymer", [("A" * (K + 3), 3)]),
           ("acac", [("AC" * (K + 1), 2)]),
           ("atat", [("AT" * (K + 1), 4)]),
           ("tail", [("A" * (K + 2) + "C" + "G" * (K + 1), 5)])]
    if (K + 1) % 2 == 0:
        u = ("ACGGT" * K)[:(K + 1) // 2]
        out.append(("lone", [(u + rc_text(u), 6)]))
    if K <= 4:
        out.append(("complete", [(text_of(e, K + 1), 1 + e % 6) for e in range(1 << (2 * (K + 1)))
                                 if e <= tm.revcomp(e, K + 1)]))
    return out


# (K, density, seed, edges wanted or None, property wanted or None): see the module's comment
_RANDOM = (
    (1, 0.5, 14, None, "cycle"),
    (2, 0.5, 6, 32, None),
    (3, 0.12, 436, 31, "cycle"),
    (3, 0.12, 65, 33, "cycle"),
    (3, 0.25, 71, 63, None),
    (3, 0.25, 61, 64, None),
    (3, 0.25, 17, 65, None),
    (3, 0.5, 121, None, "second"),
    (4, 0.1, 120, None, "too_long"),
    (4, 0.5, 0, None, None),
    (5, 0.1, 0, None, "uneven"),
    (5, 0.3, 0, None, None),
    (5, 1.0, 0, None, None),
)


def _has(prop, edges, counts, K):
    if prop is None:
        return True
    if prop == "cycle":
        return em.entry_edge_set(edges, counts, K)["cycle_edges"] > 0
    steps = tm.prune(edges, counts, K, 2)
    rep = steps[0][2]
    if prop == "too_long":
        return rep["too_long"] > 0
    if prop == "uneven":
        return rep["joined_at_begin"] != rep["joined_at_end"]
    return steps[1][2]["tips"] > 0


def find_seeds(limit=2000):
    """the rows of _RANDOM with the first seed that gives each what it wants; by hand only"""
    rows = []
    for K, density, _, want_n, prop in _RANDOM:
        for seed in range(limit):
            edges, counts = random_graph(K, density, seed)
            if edges and (want_n is None or len(edges) == want_n) and _has(prop, edges, counts, K):
                rows.append((K, density, seed, want_n, prop))
                break
        else:
            raise LookupError((K, density, want_n, prop))
    return rows


_corpus = []


def corpus():
    """[(name, K, edges, counts)]: at most 40 graphs, K = 1 .. 5, 1 .. 4 096 edges each, densities 0.1 .. 1.0"""
    if not _corpus:
        for K in range(1, 6):
            for name, strings in planted(K):
                edges, counts = tm.graph_of(strings, K)
                _corpus.append(("%s-k%d" % (name, K), K, edges, counts))
            for k, density, seed, _, _ in _RANDOM:
                if k == K:
                    edges, counts = random_graph(K, density, seed)
                    _corpus.append(("random-k%d-d%g-s%d" % (K, density, seed), K, edges, counts))
        assert len(_corpus) <= MAX_GRAPHS and all(1 <= len(g[2]) <= MAX_EDGES for g in _corpus)
    return list(_corpus)


def largest(count=5):
    """the graphs with the most edges -- at these K the densest there are: the complete graphs of K = 4 and 5 and the
    random ones of K = 4 and 5 -- where the device's answers are held to one another without a model"""
    return sorted(corpus(), key=lambda g: -len(g[2]))[:count]


def blind_nodes(K, edges):
    """The nodes that two or more edges enter and none leaves, and their mirror images.  The edges that meet in such a
    node lie in one component (count-components joins what shares a node) and are not reached from one another by
    build-subgraph's growth, which goes from an edge to the edges that leave its to-node and enter its from-node."""
    node_mask = (1 << (2 * K)) - 1
    out_deg, in_deg = {}, {}
    for e in edges:
        out_deg[e >> 2] = out_deg.get(e >> 2, 0) + 1
        in_deg[e & node_mask] = in_deg.get(e & node_mask, 0) + 1
    sinks = {v for v, d in in_deg.items() if d >= 2 and v not in out_deg}
    sources = {v for v, d in out_deg.items() if d >= 2 and v not in in_deg}
    return sinks | sources


def probe_ranks(K, edges, counts, extra=3):
    """The ranks from which the device's growth is held to its own components without a model: the first, the middle
    and the last, and the smallest ranks of the `extra` largest component pairs (a component and its mirror component)
    that touch no blind node and are not the whole graph -- where there are any.  From the first three the growth is
    often held back by a blind node; from the others it has to be the component pair.  Only the CHOICE goes through
    components_model: what is compared is the device's."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1
    blind = blind_nodes(K, edges)
    labels, table = cpm.components(edges, counts, K)
    free = []
    for c, row in enumerate(table):
        if row[6] < c:
            continue                                             # (the pair is listed under its smaller component)
        mine = [e for e, lab in zip(edges, labels) if lab in (c, row[6])]
        if len(mine) < n and not any(e >> 2 in blind or e & node_mask in blind for e in mine):
            free.append((-len(mine), row[0]))
    return sorted({0, n // 2, n - 1} | set(start for _, start in sorted(free)[:extra]))


def is_planted(name):
    return not name.startswith("random")


# ---- marks ---------------------------------------------------------------------------------------------------------

PATTERNS = ("every7th", "middle", "last", "nothing")


def mark_ranks(n, pattern):
    return {"every7th": list(range(0, n, 7)), "middle": [n // 2], "last": [n - 1], "nothing": []}[pattern]


def mark_text(edges, K, pattern):
    """The marking text of a pattern as test_gpu_subgraph.reads_of makes it: one (K+1)-mer per line, so that the
    device's windows and components_model.marks see the same thing at any K.  `nothing` is one line of K bases: too
    short for a window (in a complete graph no window misses)."""
    ranks = mark_ranks(len(edges), pattern)
    if not ranks:
        return "A" * K + "\n"
    return "\n".join(text_of(edges[i], K + 1) for i in ranks) + "\n"
