"""print-contigs (linear segments) on the device (goss_gpu_segments_*, Context.linear_segments, Context.contigs,
`goss print-contigs`) against the pure-Python model of contigs_model.py: the table, the text and the three output
forms; a long path and a cycle whose answers follow by construction."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import contigs_model as cm
import gossamer_amd as g
import tips_cases
import tips_model as tm
from gossamer_amd import binding

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
BUDGET = 512 << 20
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)
FORMS = (dict(), dict(verbose_headers=True, line_breaks=False), dict(sequence=False))
# Ranking launches: the bounded walk is ONE launch of kContigsWalkSteps >= 1 pointers per lane (kernels_contigs.hpp),
# after which every edge at most that far from its start is resolved; doubling round r then resolves every edge up to
# steps * 2^r >= 2^r from its start, so ceil(log2(longest_path)) rounds always suffice, and one more launch may be spent
# finding that nothing new resolves (what is left lies on cycles).  Hence 1 + ceil(log2(longest_path)) + 1, whatever
# the step bound is.
WALK_LAUNCHES = 1


def max_rounds(longest):
    return WALK_LAUNCHES + math.ceil(math.log2(max(longest, 2))) + 1


def run_goss(*args):
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode()


def graph_files(oracle, edges, counts, K):
    return {n[1:]: b for n, b in oracle.write_graph(edges, counts, K, out="x").items()}


def loaded(oracle, edges, counts, K, budget=BUDGET):
    ctx = g.Context(K, g.MODE_GRAPH, hbm_budget=budget)
    ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
    ctx.finish()
    return ctx


def current(ctx):
    ctx.counts.distinct = ctx.result_ptrs()[2]
    keys, counts = ctx.result()
    return keys, [int(c) for c in counts]


def check_against_model(ctx, edges, counts, K, min_length=0, min_coverage=0):
    """table, text and the three forms of the context's graph equal the model's; returns (segments, info, model info)"""
    segs, minfo = cm.linear_segments(edges, counts, K, min_length, min_coverage)
    info = None
    for line_breaks in (True, False):
        table, text, info = ctx.linear_segments(min_length, min_coverage, line_breaks)
        assert info["segments"] == len(table) == len(segs)
        at = 0
        for row, s in zip(table, segs):
            want = cm.body(s.bases, line_breaks).encode()
            flags = (binding.SEGMENT_INCLUDE_FIRST if s.include_fst else 0) | (binding.SEGMENT_INCLUDE_LAST if s.include_lst else 0)
            got = tuple(int(row[f]) for f in ("first_rank", "edges", "min", "max", "s", "s2", "len", "end_rank", "text_offset", "text_bytes"))
            assert got == (s.first_rank, s.edges, s.min, s.max, s.s, s.s2, s.len, s.end_rank, at, len(want)), s.first_rank
            assert int(row["flags"]) & 3 == flags
            assert text[at:at + len(want)] == want, s.first_rank
            at += len(want)
        assert at == len(text) == info["text_bytes"]
        assert text == cm.text_of(segs, line_breaks)
    assert info["paths"] == minfo["starts"] and info["taken_paths"] == minfo["taken"]
    assert info["longest_path"] == minfo["longest"]
    assert info["cycle_edges"] == sum(1 for r in range(len(edges)) if not _on_a_path(minfo, r))
    assert 1 <= info["rounds"] <= max_rounds(info["longest_path"])
    for kw in FORMS:
        assert ctx.contigs(min_length, min_coverage, **kw) == cm.render(segs, K, **kw), kw
    return segs, info, minfo


def _on_a_path(minfo, r):
    # with both strands marked, the bitmap misses exactly the edges of cycles that have no start
    return minfo["seen"][r]


# ---- 1: the hand-made graphs -----------------------------------------------------------------------------------------

def test_hand_made_graphs(oracle):
    kinds = dict(starts=0, segments=0, mirrored=0, no_fst=0, no_lst=0, filtered=0)
    for K in (15, 27, 30, 31, 55):
        edges, counts, _ = tips_cases.combined_graph(K)
        with loaded(oracle, edges, counts, K) as ctx:
            segs, info, minfo = check_against_model(ctx, edges, counts, K)
            some, _, _ = check_against_model(ctx, edges, counts, K, min_length=K + 10, min_coverage=5)
            assert current(ctx) == (edges, counts)
        mirrored = sum(1 for s in segs if s.first_rank == edges.index(tm.revcomp(edges[s.end_rank], K + 1)))
        if K % 2 == 1:
            assert mirrored == 2
        kinds["starts"] += minfo["starts"]
        kinds["segments"] += len(segs)
        kinds["mirrored"] += mirrored
        kinds["no_fst"] += sum(1 for s in segs if not s.include_fst)
        kinds["no_lst"] += sum(1 for s in segs if not s.include_lst)
        kinds["filtered"] += len(segs) - len(some)
    for k, v in kinds.items():
        assert v > 0, k


# ---- 2: reads with substituted bases, raw and cleaned in the same context ---------------------------------------------

@pytest.mark.parametrize("K", [27, 33])
def test_reads_with_errors(oracle, K):
    reads = tips_cases.error_reads(**READS)
    edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
    te, tc = tm.trim(edges, counts, 1)
    ce, cc, _ = tm.prune(te, tc, K, 3)[-1]
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        ctx.push_host(reads.encode())
        ctx.finish()
        segs, info, _ = check_against_model(ctx, edges, counts, K)
        assert len(segs) >= 500
        assert sum(1 for s in segs if s.edges < K and not s.include_fst and not s.include_lst) > 100
        check_against_model(ctx, edges, counts, K, min_length=K + 10, min_coverage=5)
        assert current(ctx) == (edges, counts)
        ctx.select_counts(2, 0xFFFFFFFF)
        ctx.prune_tips(3)
        assert current(ctx) == (ce, cc)
        csegs, cinfo, _ = check_against_model(ctx, ce, cc, K)
        assert cinfo["longest_path"] >= 500 and len(csegs) > 0
        files = ctx.emit()
    want = graph_files(oracle, ce, cc, K)
    assert sorted(files) == sorted(want)
    for n in want:
        assert files[n] == want[n], n


# ---- 3: a long path and a cycle, by construction ---------------------------------------------------------------------

def _rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _keys_of(text, K):
    """the (K+1)-mers of a text as Python ints, in text order (a rolling value instead of tm.encode per window)"""
    codes = np.frombuffer(text.encode(), dtype=np.uint8)
    codes = ((codes >> 1) & 3) ^ (((codes >> 1) & 3) >> 1)            # A C G T -> 0 1 2 3
    vals = [0] * (len(text) - K)
    v = 0
    mask = (1 << (2 * (K + 1))) - 1
    for i, c in enumerate(codes.tolist()):
        v = ((v << 2) | c) & mask
        if i >= K:
            vals[i - K] = v
    return vals


def _long_graph(strings, K):
    got = set()
    for t in strings:
        got.update(_keys_of(t, K))
        got.update(_keys_of(_rc_text(t), K))
    return sorted(got)


@pytest.mark.parametrize("K", [27, 33])
def test_long_path_and_cycle(oracle, K):
    rng = random.Random(77 + K)
    n = 300000
    text = "".join(rng.choice("ACGT") for _ in range(n))
    ring = "".join(rng.choice("ACGT") for _ in range(5000))
    for with_ring in (False, True):
        edges = _long_graph([text] + ([ring + ring[:K]] if with_ring else []), K)
        assert len(edges) == 2 * (n - K) + (2 * 5000 if with_ring else 0)       # no (K+1)-mer twice at these lengths
        counts = [3] * len(edges)
        first = {t: edges.index(tm.encode(t[:K + 1])) for t in (text, _rc_text(text))}
        want = min(first, key=first.get)
        with loaded(oracle, edges, counts, K) as ctx:
            table, got, info = ctx.linear_segments()
            assert info["segments"] == 1 and info["paths"] == 2 and info["taken_paths"] == 1
            assert info["longest_path"] == n - K
            assert info["cycle_edges"] == (2 * 5000 if with_ring else 0)
            assert info["rounds"] <= max_rounds(n - K)
            row = table[0]
            assert (int(row["edges"]), int(row["len"]), int(row["min"]), int(row["max"])) == (n - K, n, 3, 3)
            assert (int(row["s"]), int(row["s2"])) == (3 * (n - K), 9 * (n - K))
            assert int(row["first_rank"]) == first[want]
            assert got == cm.body(want).encode()
            assert ctx.contigs(line_breaks=False, verbose_headers=True) == (">1 %d:3:3:3:0\n%s\n" % (n, want)).encode()
            assert ctx.contigs(min_length=n + 1) == b""


# ---- 4: random graphs -----------------------------------------------------------------------------------------------

def test_random_graphs(oracle):
    for seed in range(20):
        rng = random.Random(900 + seed)
        K = rng.choice((15, 27, 31, 33))
        rnd = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
        shared = [rnd(K) for _ in range(3)]
        strings = []
        for _ in range(rng.randint(3, 8)):
            t = rnd(rng.randint(30, 400))
            for _ in range(rng.randint(0, 2)):                          # planted shared K-mers: branching
                node = rng.choice(shared)
                at = rng.randrange(0, max(1, len(t) - K))
                t = t[:at] + node + t[at + K:]
            strings.append(t)
        ring = rnd(rng.randint(K + 5, 120))
        strings.append(ring + ring[:K])
        got = {}
        for t in strings:
            for i in range(len(t) - K):
                e = tm.encode(t[i:i + K + 1])
                c = got.get(e) or rng.randint(1, 40)
                got[e] = got[tm.revcomp(e, K + 1)] = c
        edges = sorted(got)
        counts = [got[e] for e in edges]
        with loaded(oracle, edges, counts, K) as ctx:
            segs, info, minfo = check_against_model(ctx, edges, counts, K)
            check_against_model(ctx, edges, counts, K, min_length=rng.randint(1, 2 * K), min_coverage=rng.randint(1, 20))
            assert minfo["rule_ok"] and info["cycle_edges"] > 0
            assert current(ctx) == (edges, counts)


# ---- 5: the command, end to end -------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [27, 33])
def test_cli(oracle, tmp_path, K):
    reads = tips_cases.error_reads(**READS)
    edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
    te, tc = tm.trim(edges, counts, 1)
    pe, pc, _ = tm.prune(te, tc, K, 2)[-1]
    (tmp_path / "reads.txt").write_text(reads)
    built, trimmed, pruned = tmp_path / "built", tmp_path / "trimmed", tmp_path / "pruned"
    rc, _, err = run_goss("build-graph", "-k", K, "-O", built, "--line-in", tmp_path / "reads.txt")
    assert rc == 0, err
    rc, _, err = run_goss("trim-graph", "-G", built, "-O", trimmed, "-C", 1)
    assert rc == 0, err
    rc, _, err = run_goss("prune-tips", "-G", trimmed, "-O", pruned, "--iterate", 2)
    assert rc == 0, err
    segs, _ = cm.linear_segments(pe, pc, K)
    some, _ = cm.linear_segments(pe, pc, K, min_length=100, min_coverage=5)
    assert 0 < len(some) < len(segs)
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        ctx.push_host(reads.encode())
        ctx.finish()
        ctx.select_counts(2, 0xFFFFFFFF)
        ctx.prune_tips(2)
        cases = (([], dict(), segs),
                 (["--verbose-headers", "--no-line-breaks"], dict(verbose_headers=True, line_breaks=False), segs),
                 (["--no-sequence"], dict(sequence=False), segs),
                 (["--min-length", 100, "--min-coverage", 5, "--print-rcs", "--print-linear-segments", "-T", 4], dict(), some))
        for i, (args, kw, model) in enumerate(cases):
            want = cm.render(model, K, **kw)
            rc, out, err = run_goss("print-contigs", "-G", pruned, *args)
            assert rc == 0 and out == want, (args, err)
            dst = tmp_path / ("contigs%d.fa" % i)
            rc, out, err = run_goss("print-contigs", "-G", pruned, "-o", dst, *args)
            assert rc == 0 and out == b"" and dst.read_bytes() == want, (args, err)
            if model is segs:
                assert ctx.contigs(**kw) == want
            else:
                assert ctx.contigs(100, 5, **kw) == want
    # a supergraph beside the graph: refused unless --print-linear-segments is given
    (tmp_path / "pruned-supergraph.header").write_bytes(b"")
    rc, out, err = run_goss("print-contigs", "-G", pruned)
    assert rc == 1 and out == b"" and "supergraph contigs are not implemented" in err and "--print-linear-segments" in err
    rc, out, err = run_goss("print-contigs", "-G", pruned, "--print-linear-segments")
    assert rc == 0 and out == cm.render(segs, K)
    # the asymmetric flag of a graph's header: refused with the reference's text
    hdr = bytearray((tmp_path / "pruned.header").read_bytes())
    hdr[16] |= 1
    (tmp_path / "pruned.header").write_bytes(bytes(hdr))
    rc, out, err = run_goss("print-contigs", "-G", pruned, "--print-linear-segments")
    assert rc == 1 and out == b"" and err.endswith("Asymmetric graphs not yet handled")


# ---- 6: refusals and memory ---------------------------------------------------------------------------------------------

def _status(fn):
    with pytest.raises(g.GossGpuError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(oracle):
    K = 15
    edges, counts, _ = tips_cases.combined_graph(K)
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(b"ACGTACGTACGTACGTACGTAAACCCGGGTTT\n")
        ctx.finish()
        assert _status(lambda: ctx.segments_build())[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        assert _status(lambda: ctx.segments_build())[0] == -5
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(lambda: ctx.segments_build())[0] == -5            # before finish
        ctx.finish()
        assert _status(lambda: ctx.segments_table(0, 0))[0] == -5        # without a build
        assert _status(lambda: ctx.segments_text(0, 0))[0] == -5
        info = ctx.segments_build()
        assert info["segments"] > 0
        assert _status(lambda: ctx.segments_table(info["segments"], 1))[0] == -1
        assert _status(lambda: ctx.segments_table(0, info["segments"] + 1))[0] == -1
        assert _status(lambda: ctx.segments_text(info["text_bytes"], 1))[0] == -1
        assert len(ctx.segments_table(info["segments"], 0)) == 0
        # sub-ranges; reading the result and linting keep what is held
        whole = ctx.segments_text(0, info["text_bytes"])
        assert ctx.segments_text(5, 7) == whole[5:12]
        assert current(ctx) == (edges, counts) and ctx.lint()["missing_rc"] == 0
        assert ctx.segments_text(0, info["text_bytes"]) == whole
        # a call that changes the result gives the segments back
        ctx.prune_tips(1)
        assert _status(lambda: ctx.segments_table(0, 0))[0] == -5
        ctx.segments_build()
        ctx.segments_release()
        assert _status(lambda: ctx.segments_text(0, 0))[0] == -5
        ctx.segments_release()                                           # twice is harmless
        ctx.emit()
        assert _status(lambda: ctx.segments_build())[0] == -5           # after emit
    # one reverse complement deleted: refused, naming the edge; nothing changed; the context goes on working
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        st, msg = _status(lambda: ctx.segments_build())
        assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
        assert _status(lambda: ctx.segments_table(0, 0))[0] == -5
        assert current(ctx) == (be, bc)
        assert ctx.lint()["missing_rc"] == 1


def test_out_of_memory(oracle):
    """Working memory that does not fit: GOSS_ERR_OOM, nothing held, the result intact.  The working arrays take more
    room than the edge list itself, so below some arena size the graph still loads and the segments no longer fit:
    walk the size down in steps of 32 KB until the graph itself is refused."""
    K = 27
    reads = tips_cases.error_reads(**READS)
    edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
    step1 = tm.prune(edges, counts, K, 1)[0]
    files = graph_files(oracle, edges, counts, K)
    refused = fitted = 0
    for kb in range(4096, 256, -32):
        ctx = g.Context(K, g.MODE_GRAPH, hbm_budget=kb << 10)
        try:
            try:
                ctx.push_run_graph(files, 2 * (K + 1))
                ctx.finish()
            except g.GossGpuError as e:
                assert e.status == -3
                break
            try:
                info = ctx.segments_build()
                fitted += 1
                assert info["segments"] >= 500
                ctx.segments_release()
            except g.GossGpuError as e:
                assert e.status == -3, str(e)
                refused += 1
                assert _status(lambda: ctx.segments_table(0, 0))[0] == -5
                assert current(ctx) == (edges, counts)
                assert ctx.lint()["missing_rc"] == 0
                if refused == 1:
                    try:
                        reps = ctx.prune_tips(1)
                    except g.GossGpuError as e2:
                        assert e2.status == -3
                    else:
                        assert reps[0]["tips"] == step1[2]["tips"] and current(ctx) == (step1[0], step1[1])
        finally:
            ctx.close()
    assert refused > 0 and fitted > 0
