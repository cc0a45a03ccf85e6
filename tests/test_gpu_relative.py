"""trim-relative / merge-graph-with-reference on the device (goss_gpu_trim_relative, goss_gpu_recount_from,
Context.trim_relative, Context.recount_from, `translucent trim-relative`, `translucent merge-graph-with-reference`)
against the pure-Python model of relative_model.py: the surviving edges, their counts and every report field, and the
emitted files against the oracle's write_graph of the model's survivors under the model's estimate."""
import math
import os
import subprocess

import pytest

import gossamer_amd as g
import relative_cases as rc
import relative_model as rm
import tips_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
TRANSLUCENT = os.path.join(ROOT, "gossamer_amd", "translucent")
BUDGET = 256 << 20
CLEAN = {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}


def run(exe, *args):
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode()


def graph_files(oracle, edges, counts, K, M=None):
    """{suffix: bytes} of the oracle's Graph::Builder over the list under the estimate M (None: the exact count)"""
    return {n[1:]: b for n, b in oracle.write_graph(edges, counts, K, M=M, out="x").items()}


def current(ctx):
    """(keys, counts) the context holds now"""
    ctx.counts.distinct = ctx.result_ptrs()[2]
    keys, counts = ctx.result()
    n = ctx.counts.distinct
    return [int(k) for k in keys][:n], [int(c) for c in counts][:n]


def loaded(oracle, edges, counts, K):
    ctx = g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET)
    ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
    ctx.finish()
    return ctx


def opened(oracle, edges, counts, K):
    return g.Object.open(oracle.write_graph(edges, counts, K, out="r"), "r", g.OBJECT_GRAPH)


def assert_files(files, want):
    assert sorted(files) == sorted(want)
    for n in want:
        assert files[n] == want[n], n


def _status(fn):
    with pytest.raises(g.GossGpuError) as e:
        fn()
    return e.value.status, str(e.value)


def case(name):
    return next(c for c in rc.corpus() if c.name == name)


# ---- 1: every graph of the corpus, through Context -----------------------------------------------------------------------

def _group(c):
    return "dense" if "dense" in c.tags else "straddle" if "straddle" in c.tags else "planted"


@pytest.mark.parametrize("group", ["dense", "straddle", "planted"])
def test_trim_relative_corpus(oracle, group):
    cases = [c for c in rc.corpus() if _group(c) == group]
    assert len(cases) >= 18
    ran = 0
    for c in cases:
        for i, rel in enumerate(c.rels):
            e2, c2, rep, est = rm.trim_relative(c.edges, c.counts, c.K, rel)
            with loaded(oracle, c.edges, c.counts, c.K) as ctx:
                got = ctx.trim_relative(rel)
                assert got == rep, (c.name, rel, got, rep)
                assert current(ctx) == (e2, c2), (c.name, rel)
                if i == 0:
                    assert est == len(e2)
                    assert_files(ctx.emit(), graph_files(oracle, e2, c2, c.K, M=est))
            ran += 1
    assert ran >= len(cases)


def test_default_cutoff_and_a_pass_on_its_own_output(oracle):
    for name in ("planted-k15", "planted-k62", "dense-" + max(rc.dg.corpus(), key=lambda x: len(x[2]))[0]):
        c = case(name)
        e1, c1, r1, _ = rm.trim_relative(c.edges, c.counts, c.K)
        e2, c2, r2, _ = rm.trim_relative(e1, c1, c.K, 0.5)
        e3, c3, r3, _ = rm.trim_relative(e2, c2, c.K, 1.5)
        with loaded(oracle, c.edges, c.counts, c.K) as ctx:
            assert set(ctx.relative_timing().values()) == {0.0}
            assert ctx.trim_relative() == r1 and current(ctx) == (e1, c1)
            ms = ctx.relative_timing()
            assert list(ms) == ["judge", "mirror", "compact"] and all(0 < v < 1000 for v in ms.values()), ms
            assert ctx.trim_relative(0.5) == r2 and current(ctx) == (e2, c2)
            assert ctx.lint() == CLEAN
            assert ctx.trim_relative(1.5) == r3 and current(ctx) == (e3, c3)
            assert ctx.trim_relative(0.0) == dict(r3, edges_before=len(e3), forks=rm.judge(e3, c3, 0.0)[1], below=0, mirror_only=0)
            ms = ctx.relative_timing()
            assert ms["judge"] > 0 and ms["mirror"] == ms["compact"] == 0, ms          # (nothing below: the pass stops there)
            assert_files(ctx.emit(), graph_files(oracle, e3, c3, c.K))
            assert _status(ctx.trim_relative)[0] == -5                                   # after emit


# ---- 2: merge-graph-with-reference ----------------------------------------------------------------------------------------

def test_recount_corpus(oracle):
    cases = rc.merge_corpus()
    for c in cases:
        e, cn, rep, est = rm.merge_with_reference(c.edges, c.counts, c.ref_edges, c.ref_counts)
        with loaded(oracle, c.edges, c.counts, c.K) as ctx, opened(oracle, c.ref_edges, c.ref_counts, c.K) as ref:
            got = ctx.recount_from(ref)
            assert got == rep, (c.name, got, rep)
            assert current(ctx) == (e, cn), c.name
            assert est == len(c.edges) == got["edges_before"]
            assert_files(ctx.emit_estimate(got["edges_before"]), graph_files(oracle, e, cn, c.K, M=est))
            assert ref.count == len(c.ref_edges)          # (only read)
    small = next(c for c in cases if "small_output" in c.tags)
    e, cn, _, est = rm.merge_with_reference(small.edges, small.counts, small.ref_edges, small.ref_counts)
    assert graph_files(oracle, e, cn, small.K, M=est) != graph_files(oracle, e, cn, small.K)      # the estimate decides the bytes


def test_trim_then_recount_then_trim(oracle):
    c = case("planted-k31")
    ref_counts = [x + 500 for x in c.counts]
    e1, c1, r1, _ = rm.trim_relative(c.edges, c.counts, c.K, 0.02)
    e2, c2, r2, _ = rm.merge_with_reference(e1, c1, c.edges[::2], ref_counts[::2])
    e3, c3, r3, _ = rm.trim_relative(e2, c2, c.K, 1.5) if all(tm.revcomp(x, c.K + 1) in set(e2) for x in e2) else (e2, c2, None, None)
    with loaded(oracle, c.edges, c.counts, c.K) as ctx, opened(oracle, c.edges[::2], ref_counts[::2], c.K) as ref:
        assert ctx.trim_relative(0.02) == r1
        assert ctx.recount_from(ref) == r2 and current(ctx) == (e2, c2)
        ms = ctx.relative_timing()
        assert ms["judge"] > 0 and ms["mirror"] == 0 and ms["compact"] > 0, ms
        if r3 is not None:
            assert ctx.trim_relative(1.5) == r3 and current(ctx) == (e3, c3)
        assert ctx.recount_from(ref)["edges_after"] == len(current(ctx)[0])
        ctx.emit()
        assert _status(lambda: ctx.recount_from(ref))[0] == -5                           # after emit


# ---- 3: refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    c = case("exact-1-99")
    K, edges, counts = c.K, c.edges, c.counts
    rep = rm.trim_relative(edges, counts, K, 0.02)[2]
    with opened(oracle, edges, counts, K) as ref:
        with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
            ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
            ctx.finish()
            assert _status(ctx.trim_relative)[0] == -5 and _status(lambda: ctx.recount_from(ref))[0] == -5
        with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
            assert _status(ctx.trim_relative)[0] == -5 and _status(lambda: ctx.recount_from(ref))[0] == -5
            ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
            assert _status(ctx.trim_relative)[0] == -5 and _status(lambda: ctx.recount_from(ref))[0] == -5      # before finish
            ctx.finish()
            for bad in (math.nan, math.inf, -math.inf):
                st, msg = _status(lambda: ctx.trim_relative(bad))
                assert st == -1 and "finite" in msg
                assert current(ctx) == (edges, counts)
            assert ctx.trim_relative(0.02) == rep
    # the minor edge's reverse complement deleted: refused, naming the edge; nothing changed; the context goes on working
    minor = counts.index(1)
    r = edges.index(tm.revcomp(edges[minor], K + 1))
    be, bc = edges[:r] + edges[r + 1:], counts[:r] + counts[r + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        for rel in (0.02, 0.5, 1.5):
            st, msg = _status(lambda: ctx.trim_relative(rel))
            assert st == -1 and ("edge %d has no reverse complement" % minor) in msg, msg
            assert current(ctx) == (be, bc)
        # an edge that is not below its threshold is never looked up: its missing mirror image refuses nothing
        assert ctx.trim_relative(0.0) == {"edges_before": len(be), "edges_after": len(be), "forks": 1, "below": 0, "mirror_only": 0}
        assert ctx.lint()["missing_rc"] == 1
        assert_files(ctx.emit(), graph_files(oracle, be, bc, K))
    # the major edge's reverse complement deleted: the minor one goes with its mirror image, nobody asks for the major's
    r = edges.index(tm.revcomp(edges[counts.index(99)], K + 1))
    me, mc = edges[:r] + edges[r + 1:], counts[:r] + counts[r + 1:]
    with loaded(oracle, me, mc, K) as ctx:
        e2, c2, rep2, _ = rm.trim_relative(me, mc, K, 0.02)
        assert ctx.trim_relative(0.02) == rep2 and current(ctx) == (e2, c2) and len(e2) == 1
    # a reference of another K, of another kind; a multiplicity of 2^32 - 1
    with loaded(oracle, edges, counts, K) as ctx:
        other = case("planted-k31")
        with opened(oracle, other.edges, other.counts, other.K) as ref:
            st, msg = _status(lambda: ctx.recount_from(ref))
            assert st == -1 and "k=15" in msg and "k=31" in msg, msg
        kmers = sorted({min(x, tm.revcomp(x, K)) for x in (e >> 2 for e in edges)})
        with g.Object.open(oracle.write_kmer_set(kmers, K, out="ks"), "ks", g.OBJECT_KMER_SET) as ks:
            st, msg = _status(lambda: ctx.recount_from(ks))
            assert st == -1 and "must be a Graph" in msg, msg
        assert current(ctx) == (edges, counts)
        assert ctx.trim_relative(0.02) == rep
    big = [x if x != 99 else (1 << 32) - 1 for x in counts]
    with loaded(oracle, edges, big, K) as ctx, opened(oracle, edges, counts, K) as ref:
        for fn in (ctx.trim_relative, lambda: ctx.recount_from(ref)):
            st, msg = _status(fn)
            assert st == -1 and "multiplicities of 2^32 - 1 or more" in msg
        assert ctx.result_ptrs()[2] == len(edges)


# ---- 4: the commands ---------------------------------------------------------------------------------------------------------

def _write(oracle, tmp_path, name, edges, counts, K):
    for n, b in oracle.write_graph(edges, counts, K, out=name).items():
        (tmp_path / n).write_bytes(b)
    return tmp_path / name


def _read(tmp_path, base):
    return {n[len(base):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base + "-") or n.startswith(base + ".")}


def _log_number(err, text):
    hits = [line for line in err.splitlines() if text in line]
    assert len(hits) == 1, (text, err)
    return int(hits[0].rsplit(" ", 1)[1])


def test_cli_trim_relative(oracle, tmp_path):
    runs = [("planted-k15", None), ("planted-k15", "0.5"), ("planted-k31", "0.02"), ("planted-k62", "5e-1"), ("exact-1-3", "0.25"),
            ("exact-1-3", "0.26"), ("total-over-32-bits", "0.25"), ("self-complementary-minor", "0.25"), ("straddle-63-4", None),
            ("edges-1", "1.5"), ("equal-counts", "-1")]
    for i, (name, rel) in enumerate(runs):
        c = case(name)
        e2, c2, rep, est = rm.trim_relative(c.edges, c.counts, c.K, rm.DEFAULT_REL if rel is None else float(rel))
        src, dst = _write(oracle, tmp_path, "in%d" % i, c.edges, c.counts, c.K), tmp_path / ("out%d" % i)
        args = ["trim-relative", "-v", "-G", src, "-O", dst, "-T", 1 + i] + ([] if rel is None else ["--relative-cutoff", rel])
        rcode, out, err = run(TRANSLUCENT, *args)
        assert rcode == 0 and out == b"", err
        lines = [line.split("\t")[-1] for line in err.splitlines()]
        assert [line.split(":")[0] for line in lines if not line.startswith(" ")][-4:] == \
            ["locating edges to trim", "number of edges removed", "writing out graph.", "total elapsed time"], err
        assert _log_number(err, "number of edges removed: ") == rep["edges_before"] - rep["edges_after"]
        assert_files(_read(tmp_path, dst.name), graph_files(oracle, e2, c2, c.K, M=est))
    # what was written is a graph to goss: lint-graph accepts it and dump-graph prints the model's survivors
    c = case("planted-k15")
    e2, c2, _, _ = rm.trim_relative(c.edges, c.counts, c.K, 0.5)
    want = _write(oracle, tmp_path, "want", e2, c2, c.K)
    rcode, _, err = run(GOSS, "lint-graph", "-G", tmp_path / "out1")
    assert rcode == 0 and "warning" not in err, err
    got, ref = run(GOSS, "dump-graph", "-G", tmp_path / "out1"), run(GOSS, "dump-graph", "-G", want)
    assert got[0] == ref[0] == 0 and got[1] == ref[1] and got[1].count(b"\n") >= len(e2)


def test_cli_merge_graph_with_reference(oracle, tmp_path):
    names = ("identical-k15", "interleaved-k31", "ref-in-in-k15", "one-edge-less-k31", "estimate-decides", "ref-empty-k15", "zero-count-in-ref-k62")
    by = {c.name: c for c in rc.merge_corpus()}
    for i, name in enumerate(names):
        c = by[name]
        e, cn, rep, est = rm.merge_with_reference(c.edges, c.counts, c.ref_edges, c.ref_counts)
        src, ref, dst = (_write(oracle, tmp_path, "in%d" % i, c.edges, c.counts, c.K), _write(oracle, tmp_path, "ref%d" % i, c.ref_edges, c.ref_counts, c.K),
                         tmp_path / ("out%d" % i))
        rcode, out, err = run(TRANSLUCENT, "merge-graph-with-reference", "-v", "-G", src, "--graph-ref", ref, "-O", dst)
        assert rcode == 0 and out == b"", err
        for text in ("starting graph merge", "finishing graph merge", "total build time: "):
            assert text in err
        assert_files(_read(tmp_path, dst.name), graph_files(oracle, e, cn, c.K, M=est))
    rcode, _, err = run(GOSS, "lint-graph", "-G", tmp_path / "out0")
    assert rcode == 0 and "warning" not in err, err
    c = by["identical-k15"]
    want = _write(oracle, tmp_path, "want", c.ref_edges, c.ref_counts, c.K)
    got, ref = run(GOSS, "dump-graph", "-G", tmp_path / "out0"), run(GOSS, "dump-graph", "-G", want)
    assert got[0] == ref[0] == 0 and got[1] == ref[1]
    # graphs of different K: the reference's text, and nothing written
    rcode, _, err = run(TRANSLUCENT, "merge-graph-with-reference", "-G", tmp_path / "in0", "--graph-ref", tmp_path / "ref1", "-O", tmp_path / "bad")
    assert rcode == 1 and err == ("error performing merge-graph-with-reference:\ngraphs involved in a merge must have the same kmer-size.\n"
                                  "%s has k=15.\n%s has k=31.\n" % (tmp_path / "in0", tmp_path / "ref1"))
    assert _read(tmp_path, "bad") == {}
