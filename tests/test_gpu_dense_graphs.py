"""Every graph pass of the device on every graph of the dense corpus (dense_graphs.py: K = 1 .. 5, 1 to 4 096 edges,
self-complementary nodes and edges, self-loops, two-cycles, four edges on both sides, edge counts around a bitmap word)
and on the hand-made graphs at the key widths the other graph pass tests stop short of (K = 32, 62): lint,
print-contigs, build-entry-edge-set, count-components, build-subgraph, keep_component and three prune-tips iterations,
each against its model through the comparison helpers of the pass's own test module.  Every comparison is exact.

test_dense_graphs_cpu.py holds the corpus to what it claims and the models to one another; the last test here holds the
device's answers to one another without any model."""
import random

import numpy as np
import pytest

import components_model as cpm
import contigs_model
import dense_graphs as dg
import entries_model as em
import gossamer_amd as g
import subgraph_model as sm
import test_gpu_contigs as contigs
import test_gpu_entries as entries
import tips_cases
import tips_model as tm
from test_gpu_components import CLEAN, assert_components, assert_kept
from test_gpu_subgraph import check_grow
from test_gpu_tips import assert_files, assert_reports, current, loaded

pytestmark = pytest.mark.gpu

OBJECTS_PER_K = 3
# (linear paths, radius) of the subgraph that is kept and written, per mark pattern
KEPT = {"every7th": (False, 1), "middle": (True, 3), "last": (False, 3), "nothing": (True, 1)}


def figures(info):
    """what a build says of the graph: its info less the timings and the number of launches"""
    return {k: v for k, v in info.items() if not k.startswith("ms_") and k != "launches"}


def components_twice(ctx, marked):
    """two builds in a row answer alike: the whole info, the table, the labels"""
    info, table = ctx.components(marked=marked)
    labels = ctx.component_labels()
    info2, table2 = ctx.components(marked=marked)
    assert figures(info) == figures(info2) and np.array_equal(table, table2)
    assert np.array_equal(labels, ctx.component_labels())
    return info, table, labels


def contigs_and_components(ctx, edges, counts, K):
    """steps 2 and 4 on the graph the context holds now, which may be empty; nothing stays held, the graph is as it
    was"""
    if edges:
        contigs.check_against_model(ctx, edges, counts, K)
        contigs.check_against_model(ctx, edges, counts, K, min_length=K + 2, min_coverage=2)
    else:
        # (check_against_model asks for a ranking round, which the empty graph does not take)
        for kw in (dict(), dict(min_length=K + 2, min_coverage=2)):
            table, text, info = ctx.linear_segments(**kw)
            assert (len(table), text) == (0, b"")
            for f in ("segments", "text_bytes", "paths", "taken_paths", "cycle_edges", "longest_path"):
                assert info[f] == 0, f
            for form in contigs.FORMS:
                assert ctx.contigs(**dict(kw, **form)) == contigs_model.render([], K, **form)
    assert current(ctx) == (edges, counts)
    # the empty graph has no component: an empty table, no label, and the same again
    _, _, table = assert_components(ctx, edges, counts, K)
    info, got, labels = components_twice(ctx, False)
    assert info["components"] == len(table) == len(got) and len(labels) == len(edges)
    text = dg.mark_text(edges, K, "every7th")                    # (of the empty graph: one line too short for a window)
    marked = cpm.marks(edges, K, text)[0]
    assert ctx.mark_reads(text.encode())["marked_total"] == sum(marked)
    _, _, table = assert_components(ctx, edges, counts, K, marked)
    info, got, labels = components_twice(ctx, True)
    assert info["components"] == len(table) == len(got) and info["marked_edges"] == sum(marked)
    assert [int(x) != cpm.NONE for x in labels] == marked
    ctx.components_release()
    assert current(ctx) == (edges, counts)


def grow_to_the_end(ctx, edges, K, text, linear):
    """check_grow at the radius 4 n + 4, which is beyond any diameter: the growth ends of itself.  The model makes a
    list of n marks per pass, so its passes are taken one at a time until one adds nothing -- nothing can follow an
    empty frontier -- and not 4 n + 4 times.  The device looks at what its passes added once per batch of 16
    (kGrowReadBack of graph_passes.hpp, which the number below must follow), so a radius within the first batch is run
    to its end and any other stops short."""
    n = len(edges)
    radius = 4 * n + 4
    marked = cpm.marks(edges, K, text)[0]
    assert ctx.mark_reads(text.encode())["marked_total"] == sum(marked)
    steps = sm.grow_steps(edges, K, marked, radius, linear)
    want, _ = next(steps)
    wadded = []
    for want, a in steps:
        wadded.append(a)
        if a == 0:
            break
    assert wadded[-1] == 0 and len(wadded) <= n + 1
    wadded += [0] * (radius - len(wadded))
    info, added = ctx.grow_marks(radius, linear_paths=linear)
    assert added == wadded, (K, linear)
    assert ctx.marks().tolist() == want, (K, linear)
    assert info["marked_before"] == sum(marked)
    assert info["mirrored"] == len(sm.start_set(edges, K, marked))
    assert info["marked_total"] == sum(want) == info["mirrored"] + sum(added)
    assert info["passes_run"] < radius or info["passes_run"] == radius <= 16, info
    assert all(a == 0 for a in added[info["passes_run"]:])
    return info, added, want


def run_passes(oracle, K, edges, counts, with_object, seed=0):
    """steps 1 to 7 of one graph; returns the key words of the entry edge set's object where one was opened"""
    n = len(edges)
    key_words = None
    with loaded(oracle, edges, counts, K) as ctx:
        # 1: lint
        assert ctx.lint() == CLEAN
        assert current(ctx) == (edges, counts)
        # 2, 4: print-contigs and count-components
        contigs_and_components(ctx, edges, counts, K)
        # 3: build-entry-edge-set
        model, _ = entries.check_against_model(oracle, ctx, edges, counts, K)
        if with_object:
            assert ctx.entries_build()["entries"] == len(model["starts"])
            with g.Object.from_context(ctx) as obj:
                ctx.entries_release()
                entries.check_object(obj, K, edges, model, random.Random(seed))
                key_words = obj.key_words
        assert current(ctx) == (edges, counts)
        # 5: build-subgraph's marks, both modes, every pattern, and a radius beyond any diameter
        for linear in (False, True):
            for pattern in dg.PATTERNS:
                text = dg.mark_text(edges, K, pattern)
                for radius in (0, 1, 3):
                    info, added, _ = check_grow(ctx, edges, K, text, radius, linear)
                    if pattern == "nothing":
                        assert info["marked_total"] == 0 and not any(added)
                    ctx.components_release()
                grow_to_the_end(ctx, edges, K, text, linear)
                ctx.components_release()
        assert current(ctx) == (edges, counts)
        # 7: prune-tips, one iteration at a time
        steps = tm.prune(edges, counts, K, 3)
        got = []
        for it in range(3):
            got += ctx.prune_tips(1)
            assert current(ctx) == (steps[it][0], steps[it][1]), it
        assert_reports(got, steps)
        pe, pc = steps[2][0], steps[2][1]
        assert ctx.lint() == CLEAN
        contigs_and_components(ctx, pe, pc, K)
        assert_files(oracle, ctx.emit(), pe, pc, K)
    # 5, continued: the subgraph kept and written, a context per pattern
    for pattern, (linear, radius) in KEPT.items():
        text = dg.mark_text(edges, K, pattern)
        se, sc, _ = sm.subgraph(edges, counts, K, cpm.marks(edges, K, text)[0], radius, linear)
        with loaded(oracle, edges, counts, K) as ctx:
            _, _, want = check_grow(ctx, edges, K, text, radius, linear)
            assert_components(ctx, edges, counts, K, want)       # the components of the grown marks
            assert ctx.marks().tolist() == want                  # (the build left the marks alone)
            assert ctx.keep_marked() == len(se)
            assert current(ctx) == (se, sc)
            assert ctx.lint() == CLEAN
            assert_files(oracle, ctx.emit(), se, sc, K)
        if pattern == "nothing":
            assert se == []
    # 6: the component of the first and of the last rank, kept and written
    for rank in sorted({0, n - 1}):
        with loaded(oracle, edges, counts, K) as ctx:
            assert_kept(oracle, ctx, edges, counts, K, rank)
    return key_words


def with_objects(graphs):
    """the names of the OBJECTS_PER_K largest graphs that have an entry edge at all"""
    have = [gr for gr in graphs if em.entry_edge_set(gr[2], gr[3], gr[1])["starts"]]
    return set(gr[0] for gr in sorted(have, key=lambda gr: -len(gr[2]))[:OBJECTS_PER_K])


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_every_pass_on_the_dense_corpus(oracle, K):
    graphs = [gr for gr in dg.corpus() if gr[1] == K]
    opened = with_objects(graphs)
    assert len(graphs) >= 5 and len(opened) == OBJECTS_PER_K
    for name, _, edges, counts in graphs:
        try:
            key_words = run_passes(oracle, K, edges, counts, name in opened)
        except AssertionError as e:
            raise AssertionError("%s (%d edges): %s" % (name, len(edges), e)) from e
        assert key_words == (1 if name in opened else None)


@pytest.mark.parametrize("K", [32, 62])
def test_every_pass_at_the_wide_keys(oracle, K):
    """K = 32 is the first two-word key (66 bits), K = 62 the widest (126 bits: the top of the high word is live)."""
    edges, counts, _ = tips_cases.combined_graph(K)
    assert run_passes(oracle, K, edges, counts, True) == 2
    if K == 62:
        assert any(e >> 121 for e in edges)
    # a fork of two equally strong branches: pruning empties the graph, and every pass answers for the empty graph
    fe, fc = tm.graph_of(tips_cases.Pieces(K).fork(4, 4)[0], K)
    assert tm.prune(fe, fc, K, 1)[0][0] == []
    run_passes(oracle, K, fe, fc, False)


def test_device_answers_agree_with_one_another(oracle):
    """No model: on the five largest graphs the device's passes are held to one another, so that a misreading which a
    model shares with its kernel still shows."""
    for name, K, edges, counts in dg.largest():
        n = len(edges)
        node_mask = (1 << (2 * K)) - 1
        keys = np.asarray(edges, dtype=np.uint64)
        ranks = dg.probe_ranks(K, edges, counts)
        grown = {}
        whole = 0
        with loaded(oracle, edges, counts, K) as ctx:
            _, einfo = ctx.entry_edge_set()
            table, _, sinfo = ctx.linear_segments()
            assert einfo["entries"] == sinfo["paths"] and einfo["cycle_edges"] == sinfo["cycle_edges"], name
            _, ctable = ctx.components()
            labels = ctx.component_labels()
            assert int(ctable["edges"].sum()) == n, name
            ctx.components_release()
            for rank in ranks:
                assert ctx.mark_reads((dg.text_of(edges[rank], K + 1) + "\n").encode())["marked_total"] == 1
                info, added = ctx.grow_marks(4 * n + 4)
                assert info["passes_run"] < 4 * n + 4 and added[-1] == 0, name       # (n >= 100: more than one batch)
                grown[rank] = ctx.marks()
                ctx.components_release()
            ctx.emit()
            with g.Object.from_context(ctx) as obj:
                assert obj.count == n and np.array_equal(obj.select(np.arange(n, dtype=np.uint64)), keys)
                # the component label is constant along every segment, walked edge by edge through the object
                at = table["first_rank"].astype(np.uint64)
                left = table["edges"].astype(np.int64) - 1
                first = labels[at.astype(np.int64)]
                while (left > 0).any():
                    go = left > 0
                    b, e = obj.node_ranks(obj.select(at[go]) & np.uint64(node_mask))
                    assert ((e - b) == 1).all(), name
                    at[go] = b
                    left[go] -= 1
                    assert np.array_equal(labels[at.astype(np.int64)], first), name
                assert np.array_equal(at, table["end_rank"].astype(np.uint64)), name
                # blind nodes (dense_graphs.blind_nodes), from the device's own degrees
                nodes = np.arange(1 << (2 * K), dtype=np.uint64)
                ob, oe = obj.node_ranks(nodes)
                ib, ie = obj.node_ranks(nodes, incoming=True)
                out_deg, in_deg = (oe - ob).astype(np.int64), (ie - ib).astype(np.int64)
                assert out_deg.sum() == in_deg.sum() == n
                blind = ((out_deg == 0) & (in_deg >= 2)) | ((in_deg == 0) & (out_deg >= 2))
        # the component of a rank and of its mirror image, kept, against node-mode growth to the fixed point from it
        for rank in ranks:
            pair = np.isin(labels, [labels[rank], ctable["mirror"][labels[rank]]])
            assert not (grown[rank] & ~pair).any(), (name, rank)
            touched = blind[(keys[pair] >> np.uint64(2)).astype(np.int64)]
            touched = touched | blind[(keys[pair] & np.uint64(node_mask)).astype(np.int64)]
            if not touched.any():
                assert np.array_equal(grown[rank], pair), (name, rank)
                whole += 1
            with loaded(oracle, edges, counts, K) as ctx:
                assert ctx.keep_component(rank) == int(pair.sum())
                assert current(ctx)[0] == keys[pair].tolist(), (name, rank)
        # probe_ranks gives every graph of more than one component two ranks or more at which the equality is asked
        if len(ctable) > 1:
            assert whole >= 2, (name, whole)
        if not blind.any():
            assert whole == len(ranks), (name, whole)
