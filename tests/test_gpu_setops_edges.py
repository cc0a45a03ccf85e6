"""The entry points on either side of a build (goss_gpu_select_counts / select_normal / emit_estimate / emit_count_bits /
emit_dump / emit_dump_range / lint) over the corpus of setops_edges.py, one context per case through the binding: runs
pushed from host memory with their weights, finish, the operation, the files.  Every file byte for byte the oracle's, the
held result after a selection the model's keys and counts, the text the model's, the lint totals the model's and every
returned example one of the model's offenders.  No tolerance anywhere.  A second, short group runs the commands themselves
on files the oracle wrote (the path through push_run_sparse and the host)."""
import os
import subprocess

import pytest

import gossamer_amd as g
import setops_edges as se
import setops_model as sm

pytestmark = pytest.mark.gpu

BUDGET = 256 << 20
ERR_INVALID_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


def push(ctx, keys, w):
    """one run from host memory: the keys as u64 words, `w` the weight of all or a count per key"""
    if not len(keys):
        return                                           # (an empty set pushes no run, as the commands skip an empty object)
    k = se.host_keys(keys, ctx.key_words)
    c = se.host_counts(w, len(keys))
    ctx.push_run_host(k.ctypes.data, c.ctypes.data, len(keys))


def current(ctx):
    """(keys, counts) the context holds now"""
    ctx.counts.distinct = ctx.result_ptrs()[2]
    keys, counts = ctx.result()
    return keys, [int(c) for c in counts]


def same(got, exp, *what):
    diff = se.first_difference(got, exp)
    assert diff is None, what + (diff,)


# ---- select_counts -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", se.names("select"))
def test_select_counts_keeps_the_models_items(oracle, name):
    c = se.case(name)
    keys, counts = sm.merged(c.runs)
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        for ks, w in c.runs:
            push(ctx, ks, w)
        ctx.finish()
        assert current(ctx) == (keys, counts), (name, "merged")
        for lo, hi in c.windows:
            ctx.select_counts(lo, hi)
            keys, counts = sm.select(keys, counts, lo, hi)
            got = current(ctx)
            assert got[0] == keys, (name, lo, hi, len(got[0]), len(keys), next((i for i, (a, b) in enumerate(zip(got[0], keys)) if a != b), None))
            assert got[1] == counts, (name, lo, hi)
        same(ctx.emit(), se.kmer_set_files(oracle, keys, c.K), name)


def test_select_counts_refuses_lo_above_hi_and_keeps_the_result(oracle):
    c = se.case("win_1_1")
    keys, counts = sm.merged(c.runs)
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        for ks, w in c.runs:
            push(ctx, ks, w)
        ctx.finish()
        for lo, hi in ((2, 1), (sm.U32, 0), (1, 0)):
            with pytest.raises(g.GossGpuError) as e:
                ctx.select_counts(lo, hi)
            assert e.value.status == ERR_INVALID_ARG
            assert current(ctx) == (keys, counts)
        ctx.select_counts(1, 1)
        assert current(ctx)[0] == sm.subtract(c.runs[0][0], c.runs[1][0])


def test_a_selection_that_keeps_nothing_is_the_oracles_empty_object(oracle):
    """select_counts with M reduced to 0, then emit, emit_count_bits and emit_dump: the allocations have minimum sizes and
    the kernels are launched over n"""
    c = se.case(next(n for n in se.names("select") if n.startswith("sel_n4097_all_")))
    keys, counts = sm.merged(c.runs)
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        for ks, w in c.runs:
            push(ctx, ks, w)
        ctx.finish()
        ctx.select_counts(1000, 2000)
        assert current(ctx) == ([], [])
        ctx.select_counts(0, sm.U32)                      # ... and a selection over nothing
        assert current(ctx) == ([], [])
        exp = se.kmer_set_files(oracle, [], c.K)
        same(ctx.emit(), exp, "emit")
        exp[".lhs-bits"] = exp[".rhs-bits"] = sm.words_bytes(sm.wordy_bits([]))
        ctx.emit_count_bits(1, ".lhs-bits")
        same(ctx.emit_count_bits(2, ".rhs-bits"), exp, "emit_count_bits")
        assert ctx.emit_dump() == {".dump": sm.dump_text([], None, c.K, sm.KMERS)}
        assert ctx.emit_dump_range(0, 0, 0) == {".dump": sm.dump_text([], None, c.K, sm.KMERS)}


# ---- the set algebra as the commands compose it ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in se.names("algebra") if not {"A.refused", "A.undefined"} & se.case(n).tags])
def test_the_set_algebra_writes_the_oracles_files(oracle, name):
    c = se.case(name)
    exp, stats = se.algebra_expected(oracle, name)
    runs, window = sm.as_windows(c.op, c.sets)
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        for ks, w in runs:
            push(ctx, ks, w)
        ctx.finish()
        n = ctx.result_ptrs()[2]
        if window:
            ctx.select_counts(*window)
        got = ctx.emit()
        if c.op == "annotate":
            ctx.emit_count_bits(1, ".lhs-bits")
            got = ctx.emit_count_bits(2, ".rhs-bits")
            assert (len(c.sets[0]), len(c.sets[1]), len(c.sets[0]) + len(c.sets[1]) - n) == stats, name
    same(got, exp, name)


# ---- emit_count_bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", se.names("bits"))
def test_count_bits_are_the_models_words(oracle, name):
    c = se.case(name)
    exp = se.kmer_set_files(oracle, c.keys, c.K)
    for mask in (1, 2, 3):
        exp[".bits%d" % mask] = sm.words_bytes(sm.count_bits(c.counts, mask))
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        push(ctx, c.keys, c.counts)
        ctx.finish()
        ctx.emit()
        for mask in (1, 2, 3):
            got = ctx.emit_count_bits(mask, ".bits%d" % mask)
    same(got, exp, name)


@pytest.mark.parametrize("m", [1, 63, 65, 4033, 4097, 16385])
def test_count_bits_take_nothing_from_behind_the_last_item(oracle, m):
    """The last word's bits behind item m - 1 are zero whatever lies behind the counts: the context first holds 20 000 items
    of count 3, is reset (a reset recycles the arena as it is), and then holds the m items, whose counts now lie where keys
    and counts of the first run were."""
    filler = se.drawn_keys(2 * se.BITS_K, 20000, 62)
    c = se.case(next(n for n in se.names("bits") if "B.m=%d" % m in se.case(n).tags and "B.all-common" in se.case(n).tags))
    exp = se.kmer_set_files(oracle, c.keys, c.K)
    for mask in (1, 2, 3):
        exp[".bits%d" % mask] = sm.words_bytes(sm.count_bits(c.counts, mask))
    assert m % 64 and exp[".bits3"][-8:] == ((1 << (m % 64)) - 1).to_bytes(8, "little")
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        push(ctx, filler, 3)
        ctx.finish()
        ctx.emit()
        ctx.reset()
        push(ctx, c.keys, c.counts)
        ctx.finish()
        ctx.emit()
        for mask in (1, 2, 3):
            got = ctx.emit_count_bits(mask, ".bits%d" % mask)
    same(got, exp, m)


def test_count_bits_of_nothing_is_one_zero_word(oracle):
    """m = 0, through the ABI only: the command refuses an empty side"""
    with g.Context(se.BITS_K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.finish()
        exp = se.kmer_set_files(oracle, [], se.BITS_K)
        same(ctx.emit(), exp, "emit")
        exp[".lhs-bits"] = bytes(8)
        same(ctx.emit_count_bits(1, ".lhs-bits"), exp, "bits")
        with pytest.raises(g.GossGpuError) as e:
            ctx.emit_count_bits(0, ".none")
        assert e.value.status == ERR_INVALID_ARG


# ---- select_normal + emit_estimate(edge count) ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", se.names("g2k"))
def test_graph_to_kmer_set_is_the_oracles(oracle, name):
    c = se.case(name)
    exp = se.g2k_expected(oracle, name)
    normal = sm.normal_edges_by_pairs(c.edges, c.K)
    with g.Context(c.K + 1, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        push(ctx, c.edges, 1)
        ctx.finish()
        ctx.select_normal()
        assert current(ctx) == (normal, [1] * len(normal)), name
        same(ctx.emit_estimate(len(c.edges)), exp, name)


@pytest.mark.parametrize("name", se.names("estimate"))
def test_emit_estimate_is_the_oracles_at_every_estimate(oracle, name):
    c = se.case(name)
    for label, M in se.estimates(len(c.keys), c.other):
        with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
            push(ctx, c.keys, 1)
            ctx.finish()
            same(ctx.emit_estimate(M), se.kmer_set_files(oracle, c.keys, c.K, M=M), name, label, M)


# ---- text ------------------------------------------------------------------------------------------------------------------------

def _loaded(c):
    if c.kind == "dumpk":
        ctx = g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET)
        push(ctx, c.keys, 1)
        keys, counts, kind = c.keys, None, sm.KMERS
    else:
        ctx = g.Context(c.K, g.MODE_GRAPH, hbm_budget=BUDGET)
        push(ctx, c.edges, c.counts)
        keys, counts, kind = c.edges, c.counts, sm.EDGES
    ctx.finish()
    return ctx, keys, counts, kind


def _first_text_difference(got, exp):
    if got == exp:
        return None
    n = min(len(got), len(exp))
    off = next((i for i in range(n) if got[i] != exp[i]), n)
    return "%d vs %d bytes, first difference at offset %d: %r vs %r" % (len(got), len(exp), off, got[off:off + 40], exp[off:off + 40])


@pytest.mark.parametrize("name", se.names("dumpk") + se.names("dumpe"))
def test_the_dump_is_the_models_text(oracle, name):
    c = se.case(name)
    ctx, keys, counts, kind = _loaded(c)
    with ctx:
        for flags in ((0,) if kind == sm.KMERS else (0, 1)):
            got = ctx.emit_dump(flags)
            assert list(got) == [".dump"]
            diff = _first_text_difference(got[".dump"], sm.dump_text(keys, counts, c.K, kind, flags))
            assert diff is None, (name, flags, diff)


@pytest.mark.parametrize("name", se.RANGED)
def test_a_dump_cut_into_pieces_is_the_whole(oracle, name):
    c = se.case(name)
    ctx, keys, counts, kind = _loaded(c)
    m = len(keys)
    cuts = se.range_cuts(m)
    with ctx:
        pieces = []
        for a, b in zip(cuts, cuts[1:]):
            got = ctx.emit_dump_range(0, a, b - a)[".dump"]
            diff = _first_text_difference(got, sm.dump_piece(keys, counts, c.K, kind, 0, a, b - a))
            assert diff is None, (name, a, b, diff)
            assert got.startswith(b"#") == (a == 0), (name, a, b)          # the header in front of the piece at 0 only
            pieces.append(got)
        assert b"".join(pieces) == sm.dump_text(keys, counts, c.K, kind), name
        for first, count in ((m + 1, 0), (m, 1), (0, m + 1), (m // 2, m - m // 2 + 1), (sm.M64, 2)):
            with pytest.raises(g.GossGpuError) as e:
                ctx.emit_dump_range(0, first, count)
            assert e.value.status == ERR_INVALID_ARG, (name, first, count)


# ---- lint ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", se.names("lint"))
def test_lint_totals_and_examples_are_the_models(name):
    c = se.case(name)
    with g.Context(c.K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        push(ctx, c.edges, c.counts)
        ctx.finish()
        for asym in (False, True):
            tot, off = sm.lint(c.edges, c.counts, c.K, asym)
            rep = ctx.lint(asymmetric=asym, examples=True)
            assert {k: rep[k] for k in tot} == tot, (name, asym)
            assert rep["nexamples"] == min(32, len(off)) == len(set(rep["examples"])), (name, asym, rep["nexamples"], len(off))
            assert set(rep["examples"]) <= off, (name, asym, sorted(set(rep["examples"]) - off)[:4])
        assert ctx.lint(asymmetric=False) == sm.lint(c.edges, c.counts, c.K, False)[0]


# ---- the commands themselves ---------------------------------------------------------------------------------------------------

def run(args, **kw):
    return subprocess.run([GOSS] + args + ["--hbm-budget", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def write(tmp_path, files):
    for n, b in files.items():
        (tmp_path / n).write_bytes(b)


def disk(tmp_path, base):
    return {n[len(base):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base + ".") or n.startswith(base + "-")}


COMMAND = {"intersect": "intersect-kmer-sets", "subtract": "subtract-kmer-set", "annotate": "merge-and-annotate-kmer-sets"}
COMMAND_CASES = ["intersect_disjoint", "subtract_identical", "subtract_a_empty", "intersect_one_empty_among_full", "intersect_high_word_k63",
                 "subtract_low_word_k32", "annotate_high_word_k32", "annotate_nested"]


@pytest.mark.parametrize("name", COMMAND_CASES)
def test_the_commands_write_the_oracles_files(oracle, tmp_path, name):
    c = se.case(name)
    exp, stats = se.algebra_expected(oracle, name)
    args = [COMMAND[c.op], "-O", str(tmp_path / "out")]
    for i, s in enumerate(c.sets):
        write(tmp_path, oracle.write_kmer_set(s, c.K, out="in%d" % i))
        args += ["-G", str(tmp_path / ("in%d" % i))]
    p = run(args)
    assert p.returncode == 0, p.stderr.decode()
    same(disk(tmp_path, "out"), exp, name)
    if c.op == "annotate":
        assert p.stdout.decode() == "%d\t%d\t%d\n" % stats


def test_the_commands_refusals(oracle, tmp_path):
    """merge-and-annotate-kmer-sets with an empty side throws "nonsense", a bare string no handler names
    (GossCmdMergeAndAnnotateKmerSets.cc:40-43): exit status 1 and nothing written.  intersect-kmer-sets over empty inputs only
    is undefined in the reference (the oracle refuses it); GossMerge.cpp writes the empty set."""
    c = se.case("annotate_b_empty")
    assert isinstance(se.algebra_expected(oracle, c.name)[0], oracle.OracleError)
    for i, s in enumerate(c.sets):
        write(tmp_path, oracle.write_kmer_set(s, c.K, out="in%d" % i))
    p = run(["merge-and-annotate-kmer-sets", "-G", str(tmp_path / "in0"), "-G", str(tmp_path / "in1"), "-O", str(tmp_path / "out")])
    assert p.returncode == 1 and p.stdout == b"" and "caught unknown exception" in p.stderr.decode(), p.stderr.decode()
    assert disk(tmp_path, "out") == {}
    assert isinstance(se.algebra_expected(oracle, "intersect_all_empty")[0], oracle.OracleError)
    p = run(["intersect-kmer-sets", "-G", str(tmp_path / "in1"), "-G", str(tmp_path / "in1"), "-O", str(tmp_path / "none")])
    assert p.returncode == 0, p.stderr.decode()
    same(disk(tmp_path, "none"), se.kmer_set_files(oracle, [], c.K), "all empty")
    p = run(["subtract-kmer-set", "-G", str(tmp_path / "in0"), "-O", str(tmp_path / "out")])
    assert p.returncode == 1 and "Exactly two input k-mer sets required!" in p.stderr.decode()


def test_graph_to_kmer_set_the_command(oracle, tmp_path):
    name = "g2k_long_k62"
    c = se.case(name)
    write(tmp_path, oracle.write_graph(c.edges, [1] * len(c.edges), c.K, out="gr"))
    p = run(["graph-to-kmer-set", "-G", str(tmp_path / "gr"), "-O", str(tmp_path / "out")])
    assert p.returncode == 0, p.stderr.decode()
    same(disk(tmp_path, "out"), se.g2k_expected(oracle, name), name)


def test_dump_kmer_set_above_one_sweep_the_command(oracle, tmp_path):
    c = se.case("dumpk_len63_m65537")
    write(tmp_path, oracle.write_kmer_set(c.keys, c.K, out="ks"))
    p = run(["dump-kmer-set", "-G", str(tmp_path / "ks")])
    assert p.returncode == 0, p.stderr.decode()
    diff = _first_text_difference(p.stdout, sm.dump_text(c.keys, None, c.K, sm.KMERS))
    assert diff is None, diff


@pytest.mark.parametrize("name", se.names("dumpe"))
def test_dump_graph_and_restore_graph_the_commands(oracle, tmp_path, name):
    """every graph case -- the ten-digit counts, 2^32 - 1 among them -- dumped by `goss dump-graph` and restored by `goss
    restore-graph`: the oracle's text, then the oracle's restore_graph bytes, which are the graph's"""
    c = se.case(name)
    files = oracle.write_graph(c.edges, c.counts, c.K, out="gr")
    write(tmp_path, files)
    p = run(["dump-graph", "-G", str(tmp_path / "gr"), "-o", str(tmp_path / "g.txt")])
    assert p.returncode == 0, p.stderr.decode()
    text = (tmp_path / "g.txt").read_bytes()
    diff = _first_text_difference(text, sm.dump_text(c.edges, c.counts, c.K, sm.EDGES))
    assert diff is None, (name, diff)
    assert (b"\t%d\n" % sm.U32 in text) == (sm.U32 in c.counts)
    p = run(["restore-graph", "-f", str(tmp_path / "g.txt"), "-O", str(tmp_path / "back")])
    assert p.returncode == 0, p.stderr.decode()
    exp = se.strip(oracle.restore_graph(text, "back"), "back")
    same(disk(tmp_path, "back"), exp, name)
    same(exp, se.strip(files, "gr"), name, "the restored graph is the graph")
