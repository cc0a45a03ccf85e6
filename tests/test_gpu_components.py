"""count-components on the device (goss_gpu_components_*, Context.mark_reads / components / component_labels /
keep_component, `goss count-components`) against the pure-Python model of components_model.py: the marks, the labels,
the whole table, and the files of the kept component against the oracle's write_graph of the model's edges."""
import os
import random

import numpy as np
import pytest

import components_model as cm
import gossamer_amd as g
import tips_cases
import tips_model as tm
from test_gpu_tips import BUDGET, READS, _status, assert_files, current, graph_files, loaded, run_goss

pytestmark = pytest.mark.gpu

CLEAN = {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}


def rows_of(table):
    return [tuple(int(r[f]) for f in ("start", "edges", "min", "max", "s", "s2", "mirror")) for r in table]


def assert_components(ctx, edges, counts, K, marked=None):
    """components() of the context against the model; returns (info, labels, table) of the model's kind"""
    labels, table = cm.components(edges, counts, K, marked)
    info, got = ctx.components(marked=marked is not None)
    assert info["components"] == len(table)
    assert info["marked_edges"] == sum(1 for x in labels if x != cm.NONE)
    assert info["largest"] == max([r[1] for r in table] or [0])
    assert rows_of(got) == table
    assert ctx.component_labels().tolist() == labels
    return info, labels, table


# ---- 1: the hand-made graphs ---------------------------------------------------------------------------------------

def small_graphs(K):
    """[(name, strings, components expected)], each a graph of its own:
    sink    two paths whose last edges differ and enter one node that nothing leaves: on their strand only the
            shared to-node joins them (on the other strand they are the two branches of a source)
    source  two paths that leave one node nothing enters: the from-group joins them
    mirror  K + 1 even: a path through an edge that is its own reverse complement is its own mirror image"""
    p = tips_cases.Pieces(K, seed=7)
    t = p.rnd(K)
    a, b = p.rnd(K + 4), p.rnd(K + 4)
    if a[-1] == b[-1]:
        b = b[:-1] + p.other(a[-1])
    out = [("sink", [(a + t, 3), (b + t, 5)], 2), ("source", p.fork(4, 6)[0], 2)]
    if (K + 1) % 2 == 0:
        out.append(("mirror", p.lone_palindrome(7)[0], 1))
    return out


def test_hand_made_graphs(oracle):
    """The pieces of tips_cases.py lie side by side, so every piece is a component and its mirror image another (or the
    same one: the pieces through a self-complementary edge); then the three small graphs.  One- and two-word keys."""
    for K in (15, 27, 30, 31, 55):
        edges, counts, _ = tips_cases.combined_graph(K)
        with loaded(oracle, edges, counts, K) as ctx:
            _, _, table = assert_components(ctx, edges, counts, K)
            assert len(table) >= 12
            if K % 2 == 1:
                assert sum(1 for i, r in enumerate(table) if r[6] == i) == 2         # lone_palindrome and the hairpin piece
        for name, strings, expect in small_graphs(K):
            se, sc = tm.graph_of(strings, K)
            labels, table = cm.components(se, sc, K)
            assert len(table) == expect, (K, name)
            if name == "mirror":
                assert table[0][6] == 0 and any(tm.revcomp(e, K + 1) == e for e in se)
            else:
                assert table[0][6] == 1 and table[1][6] == 0 and table[0][1] == table[1][1] == 2 * (K + 4 if name == "sink" else K + 3)
            with loaded(oracle, se, sc, K) as ctx:
                assert_components(ctx, se, sc, K)


# ---- 2: one long path ----------------------------------------------------------------------------------------------

def test_one_long_path(oracle):
    """20 000 edges in a row (their ranks are pseudo-random along the path: deep union-find chains, concurrent hooks
    on one root): two components, and a number of launches that does not know the path's length."""
    K, n = 27, 20000
    rng = random.Random(11)
    seq = "".join(rng.choice("ACGT") for _ in range(n + K))
    kmers = [seq[i:i + K] for i in range(len(seq) - K + 1)]
    both = set(kmers) | set(tips_cases._rc_text(x) for x in kmers)
    assert len(both) == 2 * len(kmers)                                               # no K-mer twice, on either strand
    edges, counts = tm.graph_of([(seq, 3)], K)
    labels, table = cm.components(edges, counts, K)
    assert [r[1] for r in table] == [n, n] and table[0][6] == 1 and table[1][6] == 0
    with loaded(oracle, edges, counts, K) as ctx:
        info, _, _ = assert_components(ctx, edges, counts, K)
        assert info["launches"] <= 64


# ---- 3, 4: reads with substituted bases; marks -----------------------------------------------------------------------

_cache = {}


def read_graph(oracle, K):
    if K not in _cache:
        reads = tips_cases.error_reads(**READS)
        edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
        _cache[K] = (reads, edges, counts)
    return _cache[K]


@pytest.mark.parametrize("K", [27, 33])
def test_reads_with_errors(oracle, K):
    """The giant-component case of the wave-aggregated figures.  The graph holds both strands, so the giant is a PAIR:
    a component and its mirror image of the same size, 49.7 % of the edges each at K = 27 -- no single component of
    this input can hold more than half.  What is asserted of the model is therefore that the largest component and
    its mirror together hold more than half of the edges (they hold 99 %)."""
    reads, edges, counts = read_graph(oracle, K)
    labels, table = cm.components(edges, counts, K)
    assert len(table) >= 3
    big = max(range(len(table)), key=lambda i: table[i][1])
    assert table[big][6] != big and table[big][1] + table[table[big][6]][1] > len(edges) // 2
    assert table[big][1] > len(edges) * 2 // 5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        ctx.push_host(reads.encode())
        ctx.finish()
        assert current(ctx) == (edges, counts)
        assert_components(ctx, edges, counts, K)
        info1, t1 = ctx.components()
        l1 = ctx.component_labels()
        info2, t2 = ctx.components()
        assert np.array_equal(t1, t2) and np.array_equal(l1, ctx.component_labels())
        assert info1["components"] == info2["components"] == len(table)


def marking_text(reads, K):
    """(first part, second part) of the marking text: every fifth read, of them one with an N, one in lower case, one
    cut to K bases; an empty line; a line of random bases (windows that are no edges); no newline at the end; split
    between two reads"""
    lines = reads.split("\n")[:-1][::5]
    assert len(lines) >= 100
    lines[3] = lines[3][:50] + "N" + lines[3][51:]
    lines[5] = lines[5].lower()
    lines[7] = lines[7][:K]
    lines.insert(9, "")
    rng = random.Random(5)
    lines.insert(30, "".join(rng.choice("ACGT") for _ in range(80)))
    text = "\n".join(lines)
    assert len(text) > 2 * 2048 + 100 and "\n\n" in text and not text.endswith("\n")
    assert any(text[p] in "ACGT" and text[p - 1] in "ACGT" for p in (2048, 4096))     # a read straddles a tile boundary
    cut = text.index("\n", 5000) + 1
    return text[:cut], text[cut:]


def marked_model(edges, K, parts):
    marked = [False] * len(edges)
    figures = []
    for part in parts:
        m, w, h = cm.marks(edges, K, part)
        marked = [a or b for a, b in zip(marked, m)]
        figures.append((w, h, sum(marked)))
    return marked, figures


@pytest.mark.parametrize("K", [27, 33])
def test_marks(oracle, K):
    reads, edges, counts = read_graph(oracle, K)
    parts = marking_text(reads, K)
    marked, figures = marked_model(edges, K, parts)
    rank = {e: i for i, e in enumerate(edges)}
    assert any(marked[i] and not marked[rank[tm.revcomp(e, K + 1)]] for i, e in enumerate(edges))     # not symmetric
    whole, _ = cm.components(edges, counts, K)
    _, mtable = cm.components(edges, counts, K, marked)
    inside = [whole[r[0]] for r in mtable]
    assert max(inside.count(c) for c in set(inside)) > 1                              # a path is cut
    with loaded(oracle, edges, counts, K) as ctx:
        assert _status(lambda: ctx.components(marked=True))[0] == -5                  # no marks yet
        for part, (w, h, total) in zip(parts, figures):
            info = ctx.mark_reads(part.encode())
            assert (info["windows"], info["hits"], info["marked_total"]) == (w, h, total)
        _, labels, _ = assert_components(ctx, edges, counts, K, marked)
        assert [x != cm.NONE for x in labels] == marked
        # the marks outlive the build that used them; a build of all edges leaves them alone
        assert_components(ctx, edges, counts, K)
        assert_components(ctx, edges, counts, K, marked)
        ctx.components_release()
        assert _status(lambda: ctx.components(marked=True))[0] == -5
        assert current(ctx) == (edges, counts)


# ---- 5: keeping one component ------------------------------------------------------------------------------------------

def assert_kept(oracle, ctx, edges, counts, K, rank):
    ke, kc = cm.keep(edges, counts, K, rank)
    assert ctx.keep_component(rank) == len(ke)
    assert current(ctx) == (ke, kc)
    assert ctx.lint() == CLEAN
    assert_files(oracle, ctx.emit(), ke, kc, K)
    return ke


def test_keep(oracle):
    K = 15
    edges, counts, _ = tips_cases.combined_graph(K)
    _, table = cm.components(edges, counts, K)
    own = [r for i, r in enumerate(table) if r[6] == i]
    assert own and table[0][6] != 0
    for row in (table[0], own[0], own[-1]):
        with loaded(oracle, edges, counts, K) as ctx:
            ke = assert_kept(oracle, ctx, edges, counts, K, row[0])
            assert len(ke) == (row[1] if row[6] == table.index(row) else 2 * row[1])
    # a context that holds marks keeps the whole-graph component, which is larger than the marked one
    K = 27
    reads, edges, counts = read_graph(oracle, K)
    parts = marking_text(reads, K)
    marked, _ = marked_model(edges, K, parts)
    _, mtable = cm.components(edges, counts, K, marked)
    ke, _ = cm.keep(edges, counts, K, mtable[0][0])
    assert len(ke) > 2 * mtable[0][1]
    with loaded(oracle, edges, counts, K) as ctx:
        for part in parts:
            ctx.mark_reads(part.encode())
        info, _ = ctx.components(marked=True)
        assert info["components"] == len(mtable)
        assert assert_kept(oracle, ctx, edges, counts, K, mtable[0][0]) == ke


# ---- 6: the command, end to end ------------------------------------------------------------------------------------------

def test_cli_end_to_end(oracle, tmp_path):
    K = 27
    reads, edges, counts = read_graph(oracle, K)
    parts = marking_text(reads, K)
    (tmp_path / "reads.txt").write_text(reads)
    (tmp_path / "marks.txt").write_text(parts[0] + parts[1])
    built, all_out, marked_out = tmp_path / "built", tmp_path / "all", tmp_path / "marked"
    rc, _, err = run_goss("build-graph", "-k", K, "-O", built, "--line-in", tmp_path / "reads.txt")
    assert rc == 0, err

    def on_disk(base):
        return {n[len(base.name):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base.name + "-") or n.startswith(base.name + ".")}

    _, table = cm.components(edges, counts, K)
    rc, out, err = run_goss("count-components", "-v", "-G", built, "-O", all_out)
    assert rc == 0, err
    assert out == cm.reference_table(table, counts)
    for text in ("marking used edges", "finding components", "Writing largest component"):
        assert text in err
    ke, kc = cm.keep(edges, counts, K, table[0][0])
    assert_files(oracle, on_disk(all_out), ke, kc, K)
    rc, _, err = run_goss("lint-graph", "-G", all_out)
    assert rc == 0 and "warning" not in err, err

    marked, _ = marked_model(edges, K, [parts[0] + parts[1]])
    _, mtable = cm.components(edges, counts, K, marked)
    rc, out, err = run_goss("count-components", "-G", built, "-O", marked_out, "--line-in", tmp_path / "marks.txt")
    assert rc == 0, err
    assert out == cm.reference_table(mtable, counts)
    ke, kc = cm.keep(edges, counts, K, mtable[0][0])
    assert_files(oracle, on_disk(marked_out), ke, kc, K)
    rc, _, err = run_goss("lint-graph", "-G", marked_out)
    assert rc == 0 and "warning" not in err, err
    # without -O nothing is written
    rc, out, err = run_goss("count-components", "-G", built)
    assert rc == 0 and out == cm.reference_table(table, counts), err

    hdr = bytearray((tmp_path / "built.header").read_bytes())
    hdr[16] |= 1
    (tmp_path / "built.header").write_bytes(bytes(hdr))
    rc, out, err = run_goss("count-components", "-G", built, "-O", tmp_path / "never")
    assert rc == 1 and err.endswith("Asymmetric graphs not yet handled") and out == b""
    assert not os.path.exists(str(tmp_path / "never") + ".header")


# ---- 7: refusals -------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    K = 15
    edges, counts, _ = tips_cases.combined_graph(K)
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
        ctx.finish()
        assert _status(lambda: ctx.components())[0] == -5
        assert _status(lambda: ctx.mark_reads(b"ACGT\n"))[0] == -5
        assert _status(lambda: ctx.keep_component(0))[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        assert _status(lambda: ctx.components())[0] == -5
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(lambda: ctx.components())[0] == -5                      # before finish
        assert _status(lambda: ctx.mark_reads(b"ACGT\n"))[0] == -5
        assert _status(lambda: ctx.keep_component(0))[0] == -5
        ctx.finish()
        assert _status(lambda: ctx.component_labels())[0] == -5                # labels and table without a build
        ctable = ctx._L.goss_gpu_components_table
        ctable.argtypes = [g.binding.C.c_void_p, g.binding.C.c_uint64, g.binding.C.c_uint64, g.binding.C.c_void_p]
        assert ctable(ctx._h, 0, 0, None) == -5
        _, _, table = assert_components(ctx, edges, counts, K)
        room = np.zeros(len(table) + 1, dtype=g.binding.COMPONENT_DTYPE)
        assert ctable(ctx._h, 0, len(table) + 1, room.ctypes.data) == -1        # a range past the end
        assert ctable(ctx._h, len(table), 1, room.ctypes.data) == -1
        assert ctable(ctx._h, len(table), 0, room.ctypes.data) == 0
        assert _status(lambda: ctx.component_labels(1, len(edges)))[0] == -1
        assert _status(lambda: ctx.keep_component(len(edges)))[0] == -1         # edge_rank == M
        cbuild = ctx._L.goss_gpu_components_build
        assert cbuild(ctx._h, 2, g.binding.C.byref(g.binding.ComponentsInfo())) == -1       # an unknown flag
        assert current(ctx) == (edges, counts)
        ctx.emit()
        assert _status(lambda: ctx.components())[0] == -5                      # after emit
        assert _status(lambda: ctx.keep_component(0))[0] == -5
    # one reverse complement deleted: refused, naming the edge; nothing changed; the context goes on working
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        for call in (lambda: ctx.components(), lambda: ctx.keep_component(0)):
            st, msg = _status(call)
            assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
            assert current(ctx) == (be, bc)
        assert _status(lambda: ctx.component_labels())[0] == -5                # nothing is held after the failure
        assert ctx.lint()["missing_rc"] == 1
        assert_files(oracle, ctx.emit(), be, bc, K)
    # working memory that does not fit: GOSS_ERR_OOM, the result intact, nothing held.  Walk the arena down in steps
    # of 32 KB until the graph itself is refused (test_refusals of test_gpu_tips.py).
    _, redges, rcounts = read_graph(oracle, 27)
    refused = 0
    for kb in range(2048, 256, -32):
        ctx = g.Context(27, g.MODE_GRAPH, hbm_budget=kb << 10)
        try:
            try:
                ctx.push_run_graph(graph_files(oracle, redges, rcounts, 27), 2 * 28)
                ctx.finish()
            except g.GossGpuError as e:
                assert e.status == -3
                break
            try:
                ctx.components()
            except g.GossGpuError as e:
                assert e.status == -3, str(e)
                refused += 1
                assert current(ctx) == (redges, rcounts)
                assert _status(lambda: ctx.component_labels())[0] == -5
                assert ctx.lint()["missing_rc"] == 0
        finally:
            ctx.close()
    assert refused > 0
