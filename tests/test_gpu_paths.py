"""trim-paths / clip-links on the device (goss_gpu_trim_paths, goss_gpu_clip_links, Context.trim_paths,
Context.clip_links, `goss trim-paths`, `goss clip-links`) against the pure-Python model of paths_model.py: the
surviving edges, their counts and every report field, and the emitted files against the oracle's write_graph of the
model's survivors under the model's estimate."""
import os
import subprocess

import pytest

import contigs_model as cm
import gossamer_amd as g
import paths_cases as pc
import paths_model as pm
import tips_cases
import tips_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
BUDGET = 256 << 20
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)


def run_goss(*args):
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode()


def graph_files(oracle, edges, counts, K, M=None):
    """{suffix: bytes} of the oracle's Graph::Builder over the list under the estimate M (None: the exact count)"""
    return {n[1:]: b for n, b in oracle.write_graph(edges, counts, K, M=M, out="x").items()}


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


def assert_files(files, want):
    assert sorted(files) == sorted(want)
    for n in want:
        assert files[n] == want[n], n


_model = {}


def model(cmd, edges, counts, K, cutoff=None, key=None):
    """(edges, counts, report, estimate, undefined) of the serial form; remembered under `key`"""
    if key is None or key not in _model:
        if cmd == "trim":
            out = pm.trim_paths_serial(edges, counts, K, cutoff)
        else:
            out = pm.clip_links_serial(edges, counts, K) + (False,)
        if key is None:
            return out
        _model[key] = out
    return _model[key]


def device(ctx, cmd, cutoff=None):
    return ctx.trim_paths(cutoff) if cmd == "trim" else ctx.clip_links()


def _status(fn):
    with pytest.raises(g.GossGpuError) as e:
        fn()
    return e.value.status, str(e.value)


# ---- 1: every graph of the corpus, through Context ---------------------------------------------------------------------

GROUPS = [(cmd, K) for cmd in ("trim", "clip") for K in pc.KS + ("dense",)]


@pytest.mark.parametrize("cmd,K", GROUPS)
def test_corpus(oracle, cmd, K):
    cases = [c for c in pc.corpus() if c.cmd == cmd and (("dense" in c.tags) if K == "dense" else (c.K == K and "dense" not in c.tags))]
    assert len(cases) >= 20
    ran = 0
    for case in cases:
        if not case.device:
            continue
        e2, c2, rep, _, _ = model(cmd, case.edges, case.counts, case.K, case.cutoff, case.name)
        with loaded(oracle, case.edges, case.counts, case.K) as ctx:
            got = device(ctx, cmd, case.cutoff)
            assert got == rep, (case, got, rep)
            assert current(ctx) == (e2, c2), case
        ran += 1
    assert ran >= 20


def test_multiplicities_the_device_refuses(oracle):
    """2^32 - 1 is kept beside the 32-bit counts: refused like prune-tips refuses it, the result untouched"""
    case = next(c for c in pc.corpus() if c.name == "clip_k15_wrap_zero_big")
    with loaded(oracle, case.edges, case.counts, 15) as ctx:
        for fn in (ctx.clip_links, ctx.trim_paths):
            st, msg = _status(fn)
            assert st == -1 and "multiplicities of 2^32 - 1 or more" in msg
        assert ctx.result_ptrs()[2] == len(case.edges)


# ---- 2: a pass on its own output; both passes; emit ----------------------------------------------------------------------

def _twice_cases():
    names = ["%s_k%d_%s" % (cmd, K, t) for cmd in ("trim", "clip") for K in (15, 32) for t in ("tips_combined", "starts_257")]
    by = {c.name: c for c in pc.corpus()}
    dense = sorted((c for c in pc.corpus() if "dense" in c.tags and c.cmd == "clip"), key=lambda c: -len(c.edges))[:3]
    return [by[n] for n in names] + dense + [c for c in pc.corpus() if c.name in [d.name.replace("clip_", "trim_", 1) for d in dense]]


def test_a_pass_on_its_own_output_and_both_passes(oracle):
    for case in _twice_cases():
        K = case.K
        e1, c1, r1, _, _ = model(case.cmd, case.edges, case.counts, K, None, case.name)
        e2, c2, r2, _, _ = model(case.cmd, e1, c1, K)
        other = "clip" if case.cmd == "trim" else "trim"
        e3, c3, r3, _, _ = model(other, e2, c2, K)
        with loaded(oracle, case.edges, case.counts, K) as ctx:
            assert device(ctx, case.cmd) == r1
            assert device(ctx, case.cmd) == r2, case
            assert current(ctx) == (e2, c2), case
            assert device(ctx, other) == r3, case
            assert current(ctx) == (e3, c3), case
            if e3:
                assert ctx.lint() == {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}
            assert_files(ctx.emit(), graph_files(oracle, e3, c3, K))
            assert _status(lambda: device(ctx, "trim"))[0] == -5             # after emit


def test_emit_under_the_commands_estimates(oracle):
    """the estimates the commands pass, below the number of edges written: z - zapCount of trim-paths (0 included), and
    z of clip-links"""
    K = 15
    p = pc.Pieces(K, 900)
    # every edge goes where no path counts twice: two spurs into each other's... a source bubble's two branches
    for name, cmd, strings in (("spur", "trim", p.spur_in(K)[0]), ("bubble", "trim", p.source_bubble()[0]),
                               ("link", "clip", p.link(K, 1, [3], [3])[0])):
        edges, counts = tm.graph_of(strings, K)
        e2, c2, rep, estimate, undefined = model(cmd, edges, counts, K)
        assert not undefined and len(e2) < len(edges)
        for M in sorted({estimate, 0, 1, len(e2) // 64, len(e2) // 2}):
            with loaded(oracle, edges, counts, K) as ctx:
                assert device(ctx, cmd) == rep
                assert_files(ctx.emit_estimate(M), graph_files(oracle, e2, c2, K, M=M))


def test_phase_times(oracle):
    """goss_gpu_paths_timing: the five phases of the last pass; a pass without starts stops after the flags"""
    K = 15
    for cmd in ("trim", "clip"):
        case = next(c for c in pc.corpus() if c.name == "%s_k15_starts_257" % cmd)
        with loaded(oracle, case.edges, case.counts, K) as ctx:
            assert set(ctx.paths_timing().values()) == {0.0}
            device(ctx, cmd)
            ms = ctx.paths_timing()
            assert list(ms) == ["link", "flag", "gather", "walk", "compact"] and all(0 < v < 1000 for v in ms.values()), ms
        case = next(c for c in pc.corpus() if c.name == "%s_k15_starts_0" % cmd)
        with loaded(oracle, case.edges, case.counts, K) as ctx:
            assert device(ctx, cmd)["candidates"] == 0
            ms = ctx.paths_timing()
            assert ms["link"] > 0 and ms["flag"] > 0 and ms["gather"] == ms["walk"] == ms["compact"] == 0, ms


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    K = 15
    case = next(c for c in pc.corpus() if c.name == "clip_k15_under_a_third")
    edges, counts = case.edges, case.counts
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
        ctx.finish()
        assert _status(ctx.trim_paths)[0] == -5 and _status(ctx.clip_links)[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        assert _status(ctx.trim_paths)[0] == -5 and _status(ctx.clip_links)[0] == -5
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(ctx.trim_paths)[0] == -5 and _status(ctx.clip_links)[0] == -5     # before finish
        ctx.finish()
        assert ctx.clip_links() == model("clip", edges, counts, K, None, case.name)[2]
    # one reverse complement deleted: refused, naming the edge; nothing changed; the context goes on working
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        for fn in (ctx.trim_paths, ctx.clip_links, lambda: ctx.trim_paths(3)):
            st, msg = _status(fn)
            assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
            assert current(ctx) == (be, bc)
        assert ctx.lint()["missing_rc"] == 1
        assert_files(ctx.emit(), graph_files(oracle, be, bc, K))
    # the report's own word for it, and the flags, through the C ABI
    import ctypes as C
    L = g.load()

    class Rep(C.Structure):
        _fields_ = [(n, C.c_uint64) for n in g.binding.LINKS_REPORT_FIELDS]

    with loaded(oracle, be, bc, K) as ctx:
        rep = Rep()
        L.goss_gpu_clip_links.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Rep)]
        assert L.goss_gpu_clip_links(ctx._h, 0, C.byref(rep)) == -1
        assert rep.missing_rc == be.index(beg) and rep.edges_before == 0 and rep.candidates == 0
        assert L.goss_gpu_clip_links(ctx._h, 1, C.byref(rep)) == -1                   # (no flag is defined)
        assert L.goss_gpu_clip_links(ctx._h, 0, None) == -1
        assert current(ctx) == (be, bc)


# ---- 4: the commands --------------------------------------------------------------------------------------------------------

def _log_number(err, text):
    hits = [line for line in err.splitlines() if text in line]
    assert len(hits) == 1, (text, err)
    return int(hits[0].rsplit(" ", 1)[1])


def _command_cases(K):
    p = pc.Pieces(K, 300)
    return [("trim", "len_2K", p.spur_in(2 * K)[0]), ("trim", "isolated", p.isolated(6)[0]), ("trim", "bubble", p.source_bubble()[0]),
            ("trim", "palindrome_and_spur", p.palindrome()[0] + p.spur_out(K)[0]),
            ("clip", "under_a_third", p.link(K, 1, [3], [3])[0]), ("clip", "third", p.link(K, 1, [2], [3])[0]),
            ("clip", "wrap_zero", p.link(3, 4, [pc.BIG_DEVICE] * 2, [9])[0])]


@pytest.mark.parametrize("K", [15, 33])
def test_cli(oracle, tmp_path, K):
    warned = 0
    for cmd, name, strings in _command_cases(K):
        edges, counts = tm.graph_of(strings, K)
        e2, c2, rep, estimate, undefined = model(cmd, edges, counts, K)
        src, dst = tmp_path / ("in_" + name), tmp_path / ("out_" + name)
        for n, b in oracle.write_graph(edges, counts, K, out=src.name).items():
            (tmp_path / n).write_bytes(b)
        if cmd == "trim":
            rc, _, err = run_goss("trim-paths", "-v", "-G", src, "-O", dst, "-C", 3, "-T", 8)
            assert rc == 0, err
            assert "locating low-coverage paths" in err and "writing out graph." in err
            assert _log_number(err, "number of paths removed: ") == rep["paths"]
            assert _log_number(err, "number of edges removed: ") == rep["zapped"]
            # where zapCount > z the reference's estimate is undefined: the exact count, and a warning that says so
            lines = [line for line in err.splitlines() if "warning" in line]
            assert len(lines) == (1 if undefined else 0), err
            if undefined:
                assert estimate == len(e2) and "exact number of edges, %d" % len(e2) in lines[0]
                warned += 1
            else:
                assert estimate == len(edges) - rep["zapped"]
        else:
            rc, _, err = run_goss("clip-links", "-v", "-G", src, "-O", dst)
            assert rc == 0, err
            for text in ("loading graph", "scanning for spurious links", "removing spurious links"):
                assert text in err
            assert _log_number(err, "links removed: ") == rep["links"]
            assert _log_number(err, "edges removed: ") == rep["edges"]
            assert estimate == len(edges)
        got = {n[len(dst.name):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path)
               if n.startswith(dst.name + "-") or n.startswith(dst.name + ".")}
        assert_files(got, graph_files(oracle, e2, c2, K, M=estimate))
    assert warned == 1


def test_cli_pipeline(oracle, tmp_path):
    """trim-graph -C 1 | prune-tips | trim-paths | clip-links | print-contigs over reads with substituted bases"""
    K = 27
    reads = tips_cases.error_reads(**READS)
    edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
    te, tc = tm.trim(edges, counts, 1)
    pe, pcn, _ = tm.prune(te, tc, K, 1)[-1]
    qe, qc, qrep, qest, qundef = model("trim", pe, pcn, K)
    le, lc, lrep, lest, _ = model("clip", qe, qc, K)
    assert not qundef and len(edges) > len(te) > len(pe) and len(le) > 0
    (tmp_path / "reads.txt").write_text(reads)
    names = [tmp_path / n for n in ("built", "trimmed", "pruned", "pathed", "clipped")]
    rc, _, err = run_goss("build-graph", "-k", K, "-O", names[0], "--line-in", tmp_path / "reads.txt")
    assert rc == 0, err
    steps = (("trim-graph", ["-C", 1], te, tc, None), ("prune-tips", [], pe, pcn, None),
             ("trim-paths", ["-C", 1], qe, qc, qest), ("clip-links", [], le, lc, lest))
    for i, (cmd, extra, we, wc, M) in enumerate(steps):
        rc, _, err = run_goss(cmd, "-v", "-G", names[i], "-O", names[i + 1], *extra)
        assert rc == 0, err
        base = names[i + 1].name
        got = {n[len(base):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base + "-") or n.startswith(base + ".")}
        assert_files(got, graph_files(oracle, we, wc, K, M=M))
        if cmd == "trim-paths":
            assert _log_number(err, "number of paths removed: ") == qrep["paths"]
        if cmd == "clip-links":
            assert _log_number(err, "links removed: ") == lrep["links"]
    rc, out, err = run_goss("print-contigs", "-G", names[-1])
    assert rc == 0 and out == cm.render(cm.linear_segments(le, lc, K)[0], K), err
    rc, _, err = run_goss("lint-graph", "-G", names[-1])
    assert rc == 0 and "warning" not in err, err
