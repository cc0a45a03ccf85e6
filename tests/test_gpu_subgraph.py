"""build-subgraph on the device (goss_gpu_components_grow / _marks / _keep_marked, Context.grow_marks / marks /
keep_marked, `goss build-subgraph`) against the pure-Python model of subgraph_model.py: the marks after the last pass,
what every pass added, the components of the grown marks, and the files of the subgraph against the oracle's
write_graph of the model's edges."""
import os
import random

import pytest

import components_model as cm
import gossamer_amd as g
import subgraph_model as sm
import tips_cases
import tips_model as tm
from test_gpu_components import CLEAN, assert_components
from test_gpu_tips import BUDGET, READS, _status, assert_files, current, graph_files, loaded, run_goss
from test_subgraph_cpu import cycle_graph

pytestmark = pytest.mark.gpu


def text_of(e, length):
    return "".join("ACGT"[(e >> (2 * (length - 1 - i))) & 3] for i in range(length))


def reads_of(edges, K, ranks):
    """a marking text whose forward windows are exactly the edges of these ranks"""
    return "\n".join(text_of(edges[i], K + 1) for i in ranks) + "\n"


def check_grow(ctx, edges, K, text, radius, linear):
    """Marks `text` on a context that holds no marks, grows them and compares everything with the model.
    Returns (info, added, the model's marks); the grown marks stay held."""
    marked = cm.marks(edges, K, text)[0]
    assert ctx.mark_reads(text.encode())["marked_total"] == sum(marked)
    want, wadded = sm.grow(edges, K, marked, radius, linear)
    info, added = ctx.grow_marks(radius, linear_paths=linear)
    assert added == wadded, (K, radius, linear)
    assert ctx.marks().tolist() == want, (K, radius, linear)
    assert info["marked_before"] == sum(marked)
    assert info["mirrored"] == len(sm.start_set(edges, K, marked))
    assert info["marked_total"] == sum(want) == info["mirrored"] + sum(added)
    assert info["passes_run"] <= radius
    assert all(a == 0 for a in added[info["passes_run"]:])
    return info, added, want


# ---- 1: the hand-made graphs ---------------------------------------------------------------------------------------

def test_hand_made_graphs(oracle):
    """One- and two-word keys, an even K + 1; marks in three pieces, on the last edge of the list (the last word of the
    bitmap and its padding bits), a radius beyond every piece's diameter, radius 0, and marks that hit nothing."""
    for K in (15, 27, 30, 31, 55):
        edges, counts, _ = tips_cases.combined_graph(K)
        n = len(edges)
        assert n % 32 != 0 and n > 256                                           # a ragged last word, more than one block
        rng = random.Random(K)
        some = reads_of(edges, K, rng.sample(range(n), 3))
        last = reads_of(edges, K, [n - 1])
        nothing = ("ACGT" * 20)[:K + 9] + "\n"
        assert sum(cm.marks(edges, K, nothing)[0]) == 0
        with loaded(oracle, edges, counts, K) as ctx:
            for linear in (False, True):
                check_grow(ctx, edges, K, some, 3, linear)
                ctx.components_release()
                _, _, want = check_grow(ctx, edges, K, last, 2, linear)
                assert want[n - 1]
                ctx.components_release()
                info, added, want = check_grow(ctx, edges, K, some, 0, linear)
                assert added == [] and info["passes_run"] == 0
                ctx.components_release()
                # beyond the diameter (node mode needs up to 197 passes at K = 55): the pieces lie side by side, so
                # the growth ends inside them
                info, added, want = check_grow(ctx, edges, K, some, 300, linear)
                assert info["passes_run"] < 300 and added[-1] == 0 and sum(want) < n
                ctx.components_release()
                info, added, want = check_grow(ctx, edges, K, nothing, 2, linear)
                assert added == [0, 0] and info["marked_total"] == 0
                ctx.components_release()
            assert current(ctx) == (edges, counts)
            # nothing marked: the empty graph
            ctx.mark_reads(nothing.encode())
            ctx.grow_marks(1)
            assert ctx.keep_marked() == 0
            assert current(ctx) == ([], [])
            assert_files(oracle, ctx.emit(), [], [], K)


# ---- 2: graphs made to break the kernels -----------------------------------------------------------------------------

def crossing(K, seed):
    """a node with four edges in and four out: four paths that cross in one K-mer"""
    rng = random.Random(seed)
    rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    node = rnd(K)
    return tm.graph_of([(rnd(K + 2) + c + node + c + rnd(K + 3), 3) for c in "ACGT"], K), node


def test_crossing_cycle_and_long_path(oracle):
    for K in (27, 32):
        # four in, four out: marked on one entering edge, the first pass takes the four that leave and none of the
        # three siblings, which the second pass reaches from the other side
        (edges, counts), node = crossing(K, K)
        entering = [i for i, e in enumerate(edges) if text_of(e, K + 1)[1:] == node]
        leaving = [i for i, e in enumerate(edges) if text_of(e, K + 1)[:-1] == node]
        assert len(entering) == len(leaving) == 4 and len(edges) % 32 != 0
        with loaded(oracle, edges, counts, K) as ctx:
            for linear in (False, True):
                for radius in (1, 2, 3):
                    _, added, want = check_grow(ctx, edges, K, reads_of(edges, K, entering[:1]), radius, linear)
                    if not linear:
                        assert all(want[i] for i in leaving) and sum(want[i] for i in entering) == (1 if radius == 1 else 4)
                        assert added[0] == 2 * (4 + 1)
                    ctx.components_release()
        # a cycle without a start and its mirror image: whole in the first linear-path pass
        edges, counts = cycle_graph(K, 3 * K + 7, K)
        n = len(edges)
        assert n % 32 != 0
        with loaded(oracle, edges, counts, K) as ctx:
            _, added, want = check_grow(ctx, edges, K, reads_of(edges, K, [5]), 3, True)
            assert all(want) and added == [n - 2, 0, 0]
            ctx.components_release()
            _, added, _ = check_grow(ctx, edges, K, reads_of(edges, K, [5]), 3, False)
            assert added == [4, 4, 4]
    # one path of 5 000 edges marked in the middle (ranks pseudo-random along the path: a deep union-find chain)
    K, n = 27, 5001
    rng = random.Random(13)
    seq = "".join(rng.choice("ACGT") for _ in range(n + K))
    edges, counts = tm.graph_of([(seq, 3)], K)
    assert len(edges) == 2 * n and len(edges) % 32 != 0
    mid = edges.index(tm.encode(seq[n // 2:n // 2 + K + 1]))
    with loaded(oracle, edges, counts, K) as ctx:
        info, added, _ = check_grow(ctx, edges, K, reads_of(edges, K, [mid]), 20, False)
        assert added == [4] * 20 and info["passes_run"] == 20
        ctx.components_release()
        info, added, want = check_grow(ctx, edges, K, reads_of(edges, K, [mid]), 20, True)
        assert added == [2 * n - 2] + [0] * 19 and all(want) and info["passes_run"] < 20
        assert info["launches"] <= 3 + 2 + 3 * 16                                # labels, mirror and count, one round of passes


# ---- 3: reads with substituted bases; components and files of the subgraph ---------------------------------------------

_cache = {}


def read_graph(oracle, K):
    if K not in _cache:
        reads = tips_cases.error_reads(**READS)
        edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
        part = "\n".join(reads.split("\n")[:-1][::10]) + "\n"
        _cache[K] = (reads, edges, counts, part)
    return _cache[K]


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("radius", [1, 2, 5])
def test_reads_with_errors(oracle, radius, linear):
    K = 27
    _, edges, counts, part = read_graph(oracle, K)
    with loaded(oracle, edges, counts, K) as ctx:
        _, added, want = check_grow(ctx, edges, K, part, radius, linear)
        assert all(added) and sum(want) < len(edges)
        assert_components(ctx, edges, counts, K, want)
        assert ctx.marks().tolist() == want                                      # the build left the marks alone
        se = [e for e, m in zip(edges, want) if m]
        sc = [c for c, m in zip(counts, want) if m]
        assert ctx.keep_marked() == len(se)
        assert current(ctx) == (se, sc)
        assert _status(lambda: ctx.marks())[0] == -5                             # given back
        assert ctx.lint() == CLEAN
        assert_files(oracle, ctx.emit(), se, sc, K)


# ---- 4: the command, end to end --------------------------------------------------------------------------------------

def test_cli_end_to_end(oracle, tmp_path):
    K = 27
    reads, edges, counts, part = read_graph(oracle, K)
    (tmp_path / "reads.txt").write_text(reads)
    (tmp_path / "marks.txt").write_text(part)
    (tmp_path / "empty.txt").write_text("")
    (tmp_path / "nothing.txt").write_text("ACGT" * 30 + "\n")
    built = tmp_path / "built"
    rc, _, err = run_goss("build-graph", "-k", K, "-O", built, "--line-in", tmp_path / "reads.txt")
    assert rc == 0, err

    def on_disk(base):
        return {n[len(base.name):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base.name + "-") or n.startswith(base.name + ".")}

    marked = cm.marks(edges, K, part)[0]
    for name, radius, linear in (("node", 3, False), ("paths", 2, True)):
        se, sc, added = sm.subgraph(edges, counts, K, marked, radius, linear)
        out = tmp_path / name
        args = ["build-subgraph", "-v", "-G", built, "-O", out, "--line-in", tmp_path / "marks.txt", "--radius", radius, "-B", 1]
        rc, _, err = run_goss(*(args + (["--linear-paths"] if linear else [])))
        assert rc == 0, err
        lines = [l[l.index("pass "):] for l in err.splitlines() if "pass " in l and " identified " in l]
        assert lines == ["pass %d identified %d additional edges." % (i, a) for i, a in enumerate(added)]
        assert_files(oracle, on_disk(out), se, sc, K)
        rc, _, err = run_goss("lint-graph", "-G", out)
        assert rc == 0 and "warning" not in err, err
    # the default radius is 1
    se, sc, added = sm.subgraph(edges, counts, K, marked, 1)
    rc, _, err = run_goss("build-subgraph", "-G", built, "-O", tmp_path / "one", "--line-in", tmp_path / "marks.txt")
    assert rc == 0 and "identified" not in err, err
    assert_files(oracle, on_disk(tmp_path / "one"), se, sc, K)
    # reads that hit nothing: the empty graph; no read at all: an error
    assert sum(cm.marks(edges, K, "ACGT" * 30)[0]) == 0
    rc, _, err = run_goss("build-subgraph", "-G", built, "-O", tmp_path / "none", "--line-in", tmp_path / "nothing.txt", "--radius", 4)
    assert rc == 0, err
    assert_files(oracle, on_disk(tmp_path / "none"), [], [], K)
    rc, _, err = run_goss("build-subgraph", "-G", built, "-O", tmp_path / "never", "--line-in", tmp_path / "empty.txt")
    assert rc == 1 and err == "error performing build-subgraph:\nNo valid reads."
    assert not os.path.exists(str(tmp_path / "never") + ".header")

    hdr = bytearray((tmp_path / "built.header").read_bytes())
    hdr[16] |= 1
    (tmp_path / "built.header").write_bytes(bytes(hdr))
    rc, _, err = run_goss("build-subgraph", "-G", built, "-O", tmp_path / "never", "--line-in", tmp_path / "marks.txt")
    assert rc == 1 and err.endswith("Asymmetric graphs not yet handled")
    assert not os.path.exists(str(tmp_path / "never") + ".header")


# ---- 5: refusals -------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    K = 15
    edges, counts, _ = tips_cases.combined_graph(K)
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
        ctx.finish()
        for call in (lambda: ctx.grow_marks(1), lambda: ctx.marks(), lambda: ctx.keep_marked()):
            assert _status(call)[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(lambda: ctx.grow_marks(1))[0] == -5                       # before finish
        assert _status(lambda: ctx.keep_marked())[0] == -5
        ctx.finish()
        for call in (lambda: ctx.grow_marks(1), lambda: ctx.marks(), lambda: ctx.keep_marked()):
            assert _status(call)[0] == -5                                        # no marks
        ctx.components()
        assert _status(lambda: ctx.grow_marks(1))[0] == -5                       # a build of all edges leaves no marks
        ctx.mark_reads(reads_of(edges, K, [3]).encode())
        grow = ctx._L.goss_gpu_components_grow
        grow.argtypes = [g.binding.C.c_void_p, g.binding.C.c_uint32, g.binding.C.c_uint32, g.binding.C.c_void_p, g.binding.C.c_void_p]
        assert grow(ctx._h, 1, 2, None, g.binding.C.byref(g.binding.GrowInfo())) == -1      # an unknown flag
        assert grow(ctx._h, 1, 0, None, None) == -1
        assert _status(lambda: ctx.marks(1, len(edges)))[0] == -1                # a range past the end
        assert ctx.marks(len(edges), 0).tolist() == []
        assert ctx.marks(3, 2).tolist() == [True, False]
        info = g.binding.GrowInfo()
        assert grow(ctx._h, 1, 0, None, g.binding.C.byref(info)) == 0            # added may be NULL
        assert info.marked_total == sum(sm.grow(edges, K, [i == 3 for i in range(len(edges))], 1)[0])
        assert current(ctx) == (edges, counts)
        ctx.emit()
        for call in (lambda: ctx.grow_marks(1), lambda: ctx.keep_marked()):
            assert _status(call)[0] == -5                                        # after emit
    # one reverse complement deleted: refused, naming the edge; nothing is held; the result is intact
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        ctx.mark_reads(reads_of(be, K, [0]).encode())
        st, msg = _status(lambda: ctx.grow_marks(1))
        assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
        assert _status(lambda: ctx.marks())[0] == -5
        assert current(ctx) == (be, bc)
    # working memory that does not fit: GOSS_ERR_OOM, the result intact, nothing held.  Walk the arena down until the
    # graph itself is refused (test_refusals of test_gpu_components.py).
    _, redges, rcounts, part = read_graph(oracle, 27)
    files = graph_files(oracle, redges, rcounts, 27)
    refused = 0
    for kb in range(2048, 256, -64):
        ctx = g.Context(27, g.MODE_GRAPH, hbm_budget=kb << 10)
        try:
            try:
                ctx.push_run_graph(files, 2 * 28)
                ctx.finish()
            except g.GossGpuError as e:
                assert e.status == -3
                break
            try:
                ctx.mark_reads(part.encode())
            except g.GossGpuError as e:
                assert e.status == -3                                            # (the marks themselves do not fit)
                continue
            try:
                ctx.grow_marks(2, linear_paths=True)
            except g.GossGpuError as e:
                assert e.status == -3, str(e)
                refused += 1
                assert current(ctx) == (redges, rcounts)
                assert _status(lambda: ctx.marks())[0] == -5
                assert ctx.lint()["missing_rc"] == 0
        finally:
            ctx.close()
    assert refused > 0
