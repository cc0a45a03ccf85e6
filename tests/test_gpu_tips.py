"""trim-graph / prune-tips on the device (goss_gpu_prune_tips, Context.prune_tips, `goss trim-graph`, `goss prune-tips`)
against the pure-Python model of tips_model.py: keys, counts and every report field per iteration, and the emitted
files against the oracle's write_graph of the model's survivors."""
import os
import subprocess

import numpy as np
import pytest

import gossamer_amd as g
import tips_cases
import tips_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
BUDGET = 512 << 20
CLASSES = ("joined_at_begin", "joined_at_end", "too_long", "both_joined", "isolated", "outweighed")
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)


def run_goss(*args):
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode()


def graph_files(oracle, edges, counts, K):
    """{suffix: bytes} of the oracle's Graph::Builder over the list, the exact count as the estimate"""
    return {n[1:]: b for n, b in oracle.write_graph(edges, counts, K, out="x").items()}


def current(ctx):
    """(keys, counts) the context holds now"""
    ctx.counts.distinct = ctx.result_ptrs()[2]
    keys, counts = ctx.result()
    return keys, [int(c) for c in counts]


def loaded(oracle, edges, counts, K):
    ctx = g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET)
    ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
    ctx.finish()
    return ctx


def assert_reports(got, steps):
    assert len(got) == len(steps)
    for it, (rep, (_, _, want)) in enumerate(zip(got, steps)):
        for f in tm.REPORT_FIELDS:
            assert rep[f] == want[f], (it, f, rep, want)


def assert_files(oracle, files, edges, counts, K):
    want = graph_files(oracle, edges, counts, K)
    assert sorted(files) == sorted(want)
    for n in want:
        assert files[n] == want[n], n


# ---- 1: the hand-made graphs ---------------------------------------------------------------------------------------

def test_hand_made_graphs(oracle):
    """Every piece of tips_cases.py (a spur of 2K and of 2K + 1 edges, a source fork 3/5, a spur stronger than its
    path, a source bubble, a lone path; for even K + 1 a lone path and a hairpin spur through an edge that is its own
    reverse complement) side by side, and the 4/4 fork that empties its graph: one- and two-word keys."""
    seen = dict.fromkeys(CLASSES, 0)
    for K in (15, 27, 30, 31, 55):
        edges, counts, expect = tips_cases.combined_graph(K)
        steps = tm.prune(edges, counts, K, 3)
        for f in tips_cases.FIELDS:                      # the model agrees with the construction
            assert steps[0][2][f] == expect[f]
        for f in CLASSES:
            seen[f] += steps[0][2][f]
        if K % 2 == 1:
            assert any(tm.revcomp(e, K + 1) == e for e in edges)
        for iterations in (1, 2, 3):
            with loaded(oracle, edges, counts, K) as ctx:
                reports = ctx.prune_tips(iterations)
                assert_reports(reports, steps[:iterations])
                assert current(ctx) == (steps[iterations - 1][0], steps[iterations - 1][1])
                assert ctx.lint() == {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}
                assert_files(oracle, ctx.emit(), steps[iterations - 1][0], steps[iterations - 1][1], K)
        # a fork of two equally strong branches goes entirely: the empty graph, as the oracle writes it
        fe, fc = tm.graph_of(tips_cases.Pieces(K).fork(4, 4)[0], K)
        fsteps = tm.prune(fe, fc, K, 2)
        assert fsteps[0][0] == [] and fsteps[0][2]["tips"] == 4
        with loaded(oracle, fe, fc, K) as ctx:
            assert_reports(ctx.prune_tips(2), fsteps)
            assert current(ctx) == ([], [])
            assert_files(oracle, ctx.emit(), [], [], K)
    for f in CLASSES:
        assert seen[f] > 0, f


# ---- 2: reads with substituted bases -------------------------------------------------------------------------------

_model_cache = {}


def read_graph(oracle, K):
    """(reads, edges, counts, model steps untrimmed, trimmed edges, counts, model steps): one model run per input"""
    if K not in _model_cache:
        reads = tips_cases.error_reads(**READS)
        edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
        te, tc = tm.trim(edges, counts, 1)
        _model_cache[K] = (reads, edges, counts, tm.prune(edges, counts, K, 5), te, tc, tm.prune(te, tc, K, 5))
    return _model_cache[K]


@pytest.mark.parametrize("K", [27, 33])
def test_reads_with_errors(oracle, K):
    reads, edges, counts, steps, te, tc, tsteps = read_graph(oracle, K)
    assert len(edges) <= 60000
    # what makes the comparison worth something
    assert steps[0][2]["tips"] >= 100 and steps[1][2]["tips"] >= 1
    assert steps[4][2]["tips"] == 0 and steps[4][0] == steps[3][0]
    assert tsteps[0][2]["tips"] >= 1 and tsteps[0][2]["isolated"] >= 1 and len(te) < len(edges)
    for trimmed in (False, True):
        want = tsteps if trimmed else steps
        with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
            ctx.push_host(reads.encode())
            ctx.finish()
            assert current(ctx) == (edges, counts)
            if trimmed:
                ctx.select_counts(2, 0xFFFFFFFF)
                assert current(ctx) == (te, tc)
            got = []
            for it in range(5):
                got += ctx.prune_tips(1)
                assert current(ctx) == (want[it][0], want[it][1]), it
            assert_reports(got, want)
            assert_files(oracle, ctx.emit(), want[4][0], want[4][1], K)


# ---- 3: iterations compose; a fixed point stays ----------------------------------------------------------------------

def test_iterations_compose_and_fixed_point(oracle):
    K = 27
    reads, edges, counts, steps, _, _, _ = read_graph(oracle, K)
    with loaded(oracle, edges, counts, K) as a, loaded(oracle, edges, counts, K) as b:
        ra = a.prune_tips(3)
        rb = b.prune_tips(1) + b.prune_tips(1) + b.prune_tips(1)
        assert ra == rb
        assert_reports(ra, steps[:3])
        assert current(a) == current(b) == (steps[2][0], steps[2][1])
        assert steps[2][2]["tips"] == 0                                   # the fixed point is reached
        assert a.prune_tips(0) == []
        again = a.prune_tips(2)
        for rep in again:
            assert rep["edges_before"] == rep["edges_after"] == len(steps[2][0])
            assert rep["tips"] == rep["zapped"] == rep["joined_at_begin"] == rep["joined_at_end"] == 0
            assert rep["candidates"] == steps[3][2]["candidates"]
        assert current(a) == (steps[2][0], steps[2][1])
        assert a.emit() == b.emit()


# ---- 4: the commands, end to end -----------------------------------------------------------------------------------------

def _log_number(err, text):
    hits = [line for line in err.splitlines() if text in line]
    assert len(hits) == 1, (text, err)
    return int(hits[0].rsplit(" ", 1)[1])


@pytest.mark.parametrize("K", [27, 33])
def test_cli_build_trim_prune(oracle, tmp_path, K):
    reads, edges, counts, _, te, tc, tsteps = read_graph(oracle, K)
    (tmp_path / "reads.txt").write_text(reads)
    built, trimmed, pruned = tmp_path / "built", tmp_path / "trimmed", tmp_path / "pruned"
    rc, _, err = run_goss("build-graph", "-k", K, "-O", built, "--line-in", tmp_path / "reads.txt")
    assert rc == 0, err
    rc, _, err = run_goss("trim-graph", "-v", "-G", built, "-O", trimmed, "-C", 1)
    assert rc == 0, err
    assert "%s had %d" % (built, len(edges)) in err and "%s will have %d" % (trimmed, len(te)) in err
    rc, _, err = run_goss("prune-tips", "-v", "-T", 8, "-G", trimmed, "-O", pruned, "--iterate", 2)
    assert rc == 0, err
    assert _log_number(err, "total number of tips removed: ") == tsteps[0][2]["tips"] + tsteps[1][2]["tips"]
    assert _log_number(err, "total number of edges removed: ") == tsteps[0][2]["zapped"] + tsteps[1][2]["zapped"]
    assert "locating tips (iteration 2)" in err

    def on_disk(base):
        return {n[len(base.name):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base.name + "-") or n.startswith(base.name + ".")}

    assert_files(oracle, on_disk(trimmed), te, tc, K)
    pe, pc = tsteps[1][0], tsteps[1][1]
    assert_files(oracle, on_disk(pruned), pe, pc, K)
    rc, _, err = run_goss("lint-graph", "-G", pruned)
    assert rc == 0 and "warning" not in err, err
    # the output answers queries: 0 for what was removed, the old count for what stayed
    files = {"p" + n: b for n, b in on_disk(pruned).items()}
    was = dict(zip(te, tc))
    kept = set(pe)
    if 2 * (K + 1) <= 62:
        queries = np.array(te, dtype=np.uint64)
    else:
        queries = np.array([[e & 0xFFFFFFFFFFFFFFFF, e >> 64] for e in te], dtype=np.uint64)
    with g.Object.open(files, "p", g.OBJECT_GRAPH) as obj:
        assert obj.count == len(pe)
        got = obj.lookup(queries)
        assert [int(c) for c in got] == [was[e] if e in kept else 0 for e in te]
    assert len(kept) < len(te)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------

def _status(fn):
    with pytest.raises(g.GossGpuError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(oracle, tmp_path):
    K = 15
    edges, counts, _ = tips_cases.combined_graph(K)
    steps = tm.prune(edges, counts, K, 1)
    # a k-mer-set context; a graph context before finish
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
        ctx.finish()
        assert _status(lambda: ctx.prune_tips(1))[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        assert _status(lambda: ctx.prune_tips(1))[0] == -5
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(lambda: ctx.prune_tips(1))[0] == -5
        ctx.finish()
        assert_reports(ctx.prune_tips(1), steps)
        ctx.emit()
        assert _status(lambda: ctx.prune_tips(1))[0] == -5              # after emit
    # one reverse complement deleted: refused, naming the edge; nothing changed; the context goes on working
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        st, msg = _status(lambda: ctx.prune_tips(2))
        assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
        assert current(ctx) == (be, bc)
        assert ctx.lint()["missing_rc"] == 1
        ctx.select_counts(1, 0xFFFFFFFF)
        assert current(ctx) == (be, bc)
        assert_files(oracle, ctx.emit(), be, bc, K)
    # the asymmetric flag of a graph's header: both commands refuse with the reference's text
    files = oracle.write_graph(edges, counts, K, out="gr")
    hdr = bytearray(files["gr.header"])
    hdr[16] |= 1
    files["gr.header"] = bytes(hdr)
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    for cmd, extra in (("trim-graph", ["-C", "1"]), ("prune-tips", [])):
        rc, _, err = run_goss(cmd, "-G", tmp_path / "gr", "-O", tmp_path / "out", *extra)
        assert rc == 1 and err.endswith("Asymmetric graphs not yet handled")
        assert not os.path.exists(str(tmp_path / "out") + ".header")
    # working memory that does not fit: GOSS_ERR_OOM, the result intact.  The link arrays take about as much room as
    # the edge list itself, so below some arena size the graph still loads and the iteration no longer fits: walk
    # the size down in steps of 32 KB until the graph itself is refused.
    _, redges, rcounts, _, _, _, _ = read_graph(oracle, 27)
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
                ctx.prune_tips(1)
            except g.GossGpuError as e:
                assert e.status == -3, str(e)
                refused += 1
                assert current(ctx) == (redges, rcounts)
                assert ctx.lint()["missing_rc"] == 0
        finally:
            ctx.close()
    assert refused > 0
