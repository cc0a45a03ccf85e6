"""The dense corpus of dense_graphs.py is what it claims to be: conditions on the INPUTS of test_gpu_dense_graphs.py,
each of which holds from the models alone.  The structures the corpus is there for occur in it; every prune-tips class
occurs; the models agree with the restated loops of the reference and with one another on every graph.

The counts come out with `pytest -s`; a condition that fails names the counts it saw."""
from bisect import bisect_left

import components_model as cpm
import contigs_model as cm
import dense_graphs as dg
import entries_model as em
import subgraph_model as sm
import tips_model as tm
from test_components_cpu import reference_rows
from test_gpu_tips import CLASSES
from test_subgraph_cpu import reference_scan

RADII = range(5)


def structure(K, edges):
    """what of the structures the corpus is there for one graph holds"""
    node_mask = (1 << (2 * K)) - 1
    out_deg, in_deg = {}, {}
    for e in edges:
        out_deg[e >> 2] = out_deg.get(e >> 2, 0) + 1
        in_deg[e & node_mask] = in_deg.get(e & node_mask, 0) + 1
    return dict(n=len(edges),
                rc_edges=sum(1 for e in edges if tm.revcomp(e, K + 1) == e),
                rc_nodes=sum(1 for v in out_deg if tm.revcomp(v, K) == v),
                rc_nodes_branching=sum(1 for v, d in out_deg.items() if d >= 2 and tm.revcomp(v, K) == v),
                self_loops=sum(1 for e in edges if e >> 2 == e & node_mask),
                four_by_four=sum(1 for v, d in out_deg.items() if d == 4 and in_deg.get(v, 0) == 4))


def test_the_corpus_holds_the_structures():
    corpus = dg.corpus()
    assert len(corpus) <= dg.MAX_GRAPHS and len(set(g[0] for g in corpus)) == len(corpus)
    assert set(g[1] for g in corpus) == {1, 2, 3, 4, 5}
    total = dict(graphs=len(corpus), edges=0, rc_edges=0, rc_nodes=0, rc_nodes_branching=0, self_loops=0,
                 four_by_four=0)
    graphs_with = dict(rc_edges=0, rc_nodes_branching=0, self_loops=0, four_by_four=0, cycle_edges=0)
    sizes = []
    for name, K, edges, counts in corpus:
        assert 1 <= len(edges) <= dg.MAX_EDGES and edges == sorted(set(edges)) and len(counts) == len(edges)
        assert all(1 <= c <= 6 for c in counts)
        at = {e: i for i, e in enumerate(edges)}
        assert all(counts[at[tm.revcomp(e, K + 1)]] == counts[i] for i, e in enumerate(edges)), name
        s = structure(K, edges)
        sizes.append(s["n"])
        total["edges"] += s["n"]
        for f in ("rc_edges", "rc_nodes", "rc_nodes_branching", "self_loops", "four_by_four"):
            total[f] += s[f]
            if f in graphs_with and s[f]:
                graphs_with[f] += 1
        if not dg.is_planted(name) and em.entry_edge_set(edges, counts, K)["cycle_edges"] > 0:
            graphs_with["cycle_edges"] += 1
    print("dense corpus:", total, "graphs with:", graphs_with)
    seen = (total, graphs_with, sorted(sizes))
    # the last word of a 32-bit and of a 64-bit bitmap full, missing, one bit long; the smallest graphs there are
    for n in (1, 2, 31, 32, 33, 63, 64, 65):
        assert n in sizes, (n, seen)
    assert max(sizes) == dg.MAX_EDGES, seen
    assert graphs_with["rc_edges"] >= 5 and graphs_with["rc_nodes_branching"] >= 5, seen
    assert graphs_with["self_loops"] >= 1 and graphs_with["four_by_four"] >= 1, seen
    assert graphs_with["cycle_edges"] >= 3, seen                 # among the random graphs alone


def test_the_planted_graphs_are_what_their_names_say():
    for K in range(1, 6):
        got = {name: tm.graph_of(strings, K) for name, strings in dg.planted(K)}
        node_mask = (1 << (2 * K)) - 1
        edges, _ = got["homopolymer"]
        assert len(edges) == 2 and all(e >> 2 == e & node_mask for e in edges)
        for name in ("acac", "atat"):
            edges, counts = got[name]
            assert len(edges) == (4 if name == "acac" else 2), (K, name)
            model = em.entry_edge_set(edges, counts, K)
            assert model["starts"] == [] and model["cycle_edges"] == len(edges)
        edges, _ = got["atat"]                                   # its own mirror image
        assert sorted(tm.revcomp(e, K + 1) for e in edges) == edges
        edges, counts = got["tail"]
        loops = [e for e in edges if e >> 2 == e & node_mask]    # A.. and G.. and their mirror images
        assert len(loops) == 4 and len(edges) > 4 and em.entry_edge_set(edges, counts, K)["cycle_edges"] == 0
        assert ("lone" in got) == ((K + 1) % 2 == 0)
        if "lone" in got:
            edges, _ = got["lone"]
            assert len(edges) == 1 and tm.revcomp(edges[0], K + 1) == edges[0]
        assert ("complete" in got) == (K <= 4)
        if "complete" in got:
            assert got["complete"][0] == list(range(1 << (2 * (K + 1))))
            assert dg.random_graph(K, 1.0, 0)[0] == got["complete"][0]
    assert dg.random_graph(3, 0.3, 5) == dg.random_graph(3, 0.3, 5) != dg.random_graph(3, 0.3, 6)


def test_every_prune_tips_class_occurs():
    first = dict.fromkeys(CLASSES, 0)
    second_tips = uneven = emptied = 0
    for name, K, edges, counts in dg.corpus():
        steps = tm.prune(edges, counts, K, 3)
        rep = steps[0][2]
        for f in CLASSES:
            first[f] += rep[f]
        uneven += rep["joined_at_begin"] != rep["joined_at_end"]
        second_tips += steps[1][2]["tips"]
        emptied += any(not s[0] for s in steps)
    seen = dict(first, second_tips=second_tips, uneven_graphs=uneven, emptied=emptied)
    print("dense corpus, prune-tips iteration 1:", seen)
    for f in CLASSES:
        assert first[f] > 0, (f, seen)
    assert uneven >= 1 and second_tips >= 1, seen
    assert emptied == 0, seen                                    # as the comment of dense_graphs.py says


def test_models_agree_with_the_reference_loops():
    runs = 0
    for name, K, edges, counts in dg.corpus():
        patterns = [cpm.marks(edges, K, dg.mark_text(edges, K, p))[0] for p in dg.PATTERNS]
        for p, marked in zip(dg.PATTERNS, patterns):
            assert [i for i, m in enumerate(marked) if m] == dg.mark_ranks(len(edges), p), (name, p)
            for linear in (False, True):
                steps = list(reference_scan(edges, K, marked, max(RADII), linear))
                model = list(sm.grow_steps(edges, K, marked, max(RADII), linear))
                for radius in RADII:
                    assert model[radius] == steps[radius], (name, p, linear, radius)
                runs += 1
        for marked in [None] + patterns:
            labels, table = cpm.components(edges, counts, K, marked)
            rows = reference_rows(edges, counts, K, marked)
            assert len(rows) == len(table), name
            for (size, lo, hi, s, s2), (start, n, tlo, thi, ts, ts2, _) in zip(rows, table):
                m = counts[start]
                want = (n + 1, tlo, thi, (ts + m) & cpm.MASK64, (ts2 + m * m) & cpm.MASK64)
                assert (size, lo, hi, s, s2) == want, name
            assert [labels.index(c) for c in range(len(table))] == [r[0] for r in table], name
            runs += 1
    print("dense corpus: %d runs against the restated loops" % runs)


def paths_of(edges, K, model):
    """the ranks of every entry's path, walked from the entries model's starts and lengths alone"""
    node_mask = (1 << (2 * K)) - 1
    out = []
    for start, length in zip(model["starts"], model["len"]):
        path = [start]
        for _ in range(length - 1):
            path.append(bisect_left(edges, (edges[path[-1]] & node_mask) << 2))
        out.append(path)
    return out


def test_the_models_agree_with_one_another():
    whole_runs = cut = 0
    for name, K, edges, counts in dg.corpus():
        n = len(edges)
        node_mask = (1 << (2 * K)) - 1
        at = {e: i for i, e in enumerate(edges)}
        mirror = [at[tm.revcomp(e, K + 1)] for e in edges]
        model = em.entry_edge_set(edges, counts, K)
        segs, info = cm.linear_segments(edges, counts, K)
        labels, table = cpm.components(edges, counts, K)
        # the entries are the contigs model's starts, path by path
        assert info["starts"] == len(model["starts"]), name
        number = {r: j for j, r in enumerate(model["starts"])}
        paths = paths_of(edges, K, model)
        for s in segs:
            j = number[s.first_rank]
            assert (s.edges, s.end_rank, s.ranks) == (model["len"][j], model["end_edges"][j], paths[j]), name
        assert info["taken"] == len(segs)
        # every edge is on exactly one path or on a cycle without a start; the bitmap misses exactly the latter
        on_path = [r for p in paths for r in p]
        assert len(on_path) == len(set(on_path)) == sum(model["len"]) == n - model["cycle_edges"], name
        assert [r for r in range(n) if not info["seen"][r]] == sorted(set(range(n)) - set(on_path)), name
        assert info["rule_ok"], name
        # a linear path lies within one component; so does a cycle
        for p in paths:
            assert len(set(labels[r] for r in p)) == 1, name
        assert all(table[table[i][6]][6] == i for i in range(len(table))), name
        assert all(labels[mirror[r]] == table[labels[r]][6] for r in range(n)), name
        # Node-mode growth from one edge, run to its fixed point, stays within the component of the edge and of its
        # mirror image, and is all of it unless the two hold a blind node (dense_graphs.blind_nodes): growth goes from
        # an edge to what leaves its to-node and enters its from-node, so two edges that only share a dead end are one
        # component and do not reach one another.
        blind = dg.blind_nodes(K, edges)
        for rank in sorted({0, n // 2, n - 1}):
            marked = [i == rank for i in range(n)]
            grown, added = sm.grow(edges, K, marked, n + 1)
            assert added[-1] == 0, name
            want = {labels[rank], labels[mirror[rank]]}
            whole = [labels[i] in want for i in range(n)]
            assert all(w for w, g in zip(whole, grown) if g), (name, rank)
            if any(whole[i] and (e >> 2 in blind or e & node_mask in blind) for i, e in enumerate(edges)):
                cut += 1
                continue
            whole_runs += 1
            assert grown == whole, (name, rank)
            kept = [i for i in range(n) if grown[i]]
            assert ([edges[i] for i in kept], [counts[i] for i in kept]) == cpm.keep(edges, counts, K, rank)
    print("dense corpus: growth to the fixed point is the component pair in %d runs, held back by a blind node in %d"
          % (whole_runs, cut))
    assert whole_runs >= 60 and cut >= 5
    assert sum(1 for _, K, edges, _ in dg.largest() if not dg.blind_nodes(K, edges)) >= 2


def test_the_probe_ranks_reach_a_whole_component_pair():
    """The model-free test of test_gpu_dense_graphs.py asserts growth == component pair only where the pair touches no
    blind node: every one of its graphs that has more than one component gives it two such ranks or more, the largest
    pair of four edges or more and not the whole graph.  (The random graph of K = 5 and density 0.3 is one component
    of 1 189 edges, its mirror image included, and 35 edges beside it: four is what it has.)"""
    several = 0
    for name, K, edges, counts in dg.largest():
        n = len(edges)
        node_mask = (1 << (2 * K)) - 1
        at = {e: i for i, e in enumerate(edges)}
        blind = dg.blind_nodes(K, edges)
        labels, table = cpm.components(edges, counts, K)
        ranks = dg.probe_ranks(K, edges, counts)
        assert {0, n // 2, n - 1} <= set(ranks) and ranks == sorted(set(ranks)), name
        if len(table) == 1:
            continue
        several += 1
        free = []
        for rank in ranks:
            want = {labels[rank], labels[at[tm.revcomp(edges[rank], K + 1)]]}
            pair = [e for e, lab in zip(edges, labels) if lab in want]
            if not any(e >> 2 in blind or e & node_mask in blind for e in pair):
                free.append(len(pair))
        assert len(free) >= 2 and 4 <= max(free) < n, (name, free)
    assert several >= 2
