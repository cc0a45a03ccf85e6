"""Read links on the device (include/goss_gpu_links.h through Context) against links_model.py over the corpus of
links_cases.py: the segment of every edge, the answer per window and the link table, in exact and in carry mode.
Every comparison is exact.  test_links_cpu.py holds the model to hand-worked cases and the corpus to its conditions.

The refusal for 2^32 - 1 edges or more is link_edges' of graph_passes.hpp, which every graph pass shares; no graph a
test can build reaches it, here as in the other passes' tests."""
import random

import numpy as np
import pytest

import gossamer_amd as g
import links_cases as lc
import links_model as lm
import tips_model as tm
from gossamer_amd import LINK_DTYPE, LINK_NONE, READ_LINKS_SYMBOLS  # noqa: F401
from test_gpu_entries import from_keys
from test_gpu_tips import BUDGET, assert_files, current, graph_files, loaded

pytestmark = pytest.mark.gpu

FIGURES = ("reads", "windows", "misses", "carried", "hits", "records")


def enc(batches):
    return [b.encode("latin-1") for b in batches]


def rows(table):
    return [tuple(int(x) for x in r) for r in table.tolist()]


def check_segments(ctx, model):
    """seg_of against the model, and against the device's own entry edge set: as many edges per segment as the
    entry's length says, and every entry edge on its own segment"""
    seg = ctx.segment_of_edges()
    assert seg.dtype == np.uint32 and seg.tolist() == model.seg_of
    files, info = ctx.entry_edge_set()
    assert info["entries"] == model.entries
    if model.entries == 0:
        return
    with g.Object.open({"x" + n: b for n, b in files.items()}, "x-entries", g.OBJECT_ENTRY_EDGE_SET) as obj:
        ranks = np.arange(model.entries, dtype=np.uint64)
        lengths = obj.length(ranks).tolist()
        ekeys = from_keys(obj.select(ranks), obj.key_words)
    assert np.bincount(seg[seg != g.LINK_NONE], minlength=model.entries).tolist() == lengths
    at = {e: i for i, e in enumerate(model.edges)}
    assert [int(seg[at[e]]) for e in ekeys] == list(range(model.entries))


def check_batches(ctx, model, batches, unique, where):
    for carry in (True, False):
        for b in batches:
            got = ctx.thread_windows(b.encode("latin-1"), unique, carry)
            assert got.tolist() == model.thread_windows(b, unique, carry), (where, carry)
        want, _ = model.read_links(batches, unique, carry)
        assert rows(ctx.read_links(enc(batches), unique, carry)) == lm.rows_of(want), (where, carry)


def test_dense_graphs(oracle):
    """the 40 dense graphs, every possible window: segments, windows and tables in both modes, every segment unique and
    every other one"""
    for name, K, edges, counts, batches in lc.dense():
        model = lm.Model(edges, K)
        with loaded(oracle, edges, counts, K) as ctx:
            check_segments(ctx, model)
            check_batches(ctx, model, batches, None, name)
            check_batches(ctx, model, batches[2:], lc.unique_of("alternating", model.entries), name)
            assert current(ctx) == (edges, counts)


@pytest.mark.parametrize("K", lc.PLANTED_K)
def test_planted_graphs(oracle, K):
    """every case of the planted corpus: one- and two-word keys, reads across tiles, the record counts around a wave and
    a sort tile, one link 70 000 times, the unique patterns"""
    graph = lc.planted(K)
    edges, counts = graph["edges"], graph["counts"]
    model = lm.Model(edges, K)
    with loaded(oracle, edges, counts, K) as ctx:
        check_segments(ctx, model)
        for name, batches, pattern, _ in lc.planted_cases(K):
            unique = lc.unique_of(pattern, model.entries, model)
            if sum(map(len, batches)) > 100000:                  # (the large ones: the tables alone)
                for carry in (True, False):
                    want, _ = model.read_links(batches, unique, carry)
                    assert rows(ctx.read_links(enc(batches), unique, carry)) == lm.rows_of(want), (name, carry)
            else:
                check_batches(ctx, model, batches, unique, name)
        # the context's result is what it was: its files are the graph's, byte for byte
        assert_files(oracle, ctx.emit(), edges, counts, K)


def test_batches_finish_twice_and_figures(oracle):
    """One table however the reads are cut into batches; finish twice; batches after a finish; the figures of every
    batch; nothing of the result changes."""
    K = 30
    graph = lc.planted(K)
    edges, counts = graph["edges"], graph["counts"]
    model = lm.Model(edges, K)
    reads = []
    for name, batches, pattern, _ in lc.planted_cases(K):
        if pattern == "all" and sum(map(len, batches)) < 20000:
            reads += [r for b in batches for r in b.split("\n")]
    rng = random.Random(7)
    rng.shuffle(reads)
    whole = "\n".join(reads) + "\n"
    unique = lc.unique_of("alternating", model.entries)
    with loaded(oracle, edges, counts, K) as ctx:
        for carry in (True, False):
            for u in (None, unique):
                want, winfo = model.read_links([whole], u, carry)
                assert winfo["records"] > (100 if u is None else 0)     # (the corpus, not the device)
                one = ctx.read_links([whole.encode()], u, carry)
                assert rows(one) == lm.rows_of(want)
                cuts = sorted(rng.sample(range(1, len(reads)), 9))
                parts = ["".join(r + "\n" for r in reads[a:b]) for a, b in zip([0] + cuts, cuts + [len(reads)])]
                parts.insert(3, "")
                parts[-1] = parts[-1][:-1]                       # (the last read without its newline)
                assert np.array_equal(ctx.read_links(enc(parts), u, carry), one)
                # the same by hand: figures per batch, finish twice, a batch after the finish
                ctx.read_links_begin(u, carry)
                for part in parts[:5]:
                    info = ctx.read_links_add(part.encode())
                    _, minfo = model.read_links([part], u, carry)
                    assert {f: info[f] for f in FIGURES} == minfo, (carry, part[:40])
                first, tinfo = ctx.read_links_table()
                again, tinfo2 = ctx.read_links_table()
                assert np.array_equal(first, again) and tinfo["rows"] == tinfo2["rows"] == len(first)
                assert rows(first) == lm.rows_of(model.read_links(parts[:5], u, carry)[0])
                for part in parts[5:]:
                    ctx.read_links_add(part.encode())
                table, tinfo = ctx.read_links_table()
                assert np.array_equal(table, one) and tinfo["records"] == winfo["records"]
                got, info = ctx.read_links_windows(parts[0].encode())          # (the windows add nothing to the records)
                assert info["records"] == 0 and np.array_equal(ctx.read_links_table()[0], one)
                ctx.read_links_release()
        assert current(ctx) == (edges, counts)
        assert_files(oracle, ctx.emit(), edges, counts, K)


def _status(fn):
    with pytest.raises(g.GossGpuError) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals(oracle):
    K = 15
    edges, counts = tm.graph_of([("ACGTTGCAAGGCTTAACCGGATATTCGCGAATT", 2), ("ACGTTGCAAGGCTTAACCGGTTTTTTTTTTTTTTTTTTTT", 2)], K)
    reads = b"ACGTTGCAAGGCTTAACCGGATATTCGCGAATT\n"
    with g.Context(K, g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
        ctx.push_host(reads)
        ctx.finish()
        assert _status(lambda: ctx.read_links_begin())[0] == -5
    with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
        ctx.push_run_graph(graph_files(oracle, edges, counts, K), 2 * (K + 1))
        assert _status(lambda: ctx.read_links_begin())[0] == -5            # before finish
        ctx.finish()
        for fn in (lambda: ctx.read_links_segments(), lambda: ctx.read_links_add(reads), lambda: ctx.read_links_windows(reads),
                   lambda: ctx.read_links_table()):                         # (finish, then table)
            assert _status(fn)[0] == -5                                     # before begin
        entries = ctx.read_links_begin()["entries"]
        assert entries == lm.Model(edges, K).entries > 0
        ctx.read_links_release()
        ctx.read_links_release()                                            # twice is harmless
        for n in (entries - 1, entries + 1, 0):
            st, msg = _status(lambda: ctx.read_links_begin(unique=[True] * n))
            assert st == -1 and "%d bits" % n in msg and "%d entry edges" % entries in msg
            assert _status(lambda: ctx.read_links_segments())[0] == -5      # nothing is held after a refusal
        ctx.read_links_begin(unique=[True] * entries)
        # before a finish there is no table
        ctx._L.goss_gpu_read_links_table.argtypes = [g.binding.C.c_void_p, g.binding.C.c_uint64, g.binding.C.c_uint64, g.binding.C.c_void_p]
        assert ctx._L.goss_gpu_read_links_table(ctx._h, 0, 0, None) == -5
        ctx.read_links_add(reads)
        assert ctx.read_links_table()[1]["records"] == lm.Model(edges, K).read_links([reads.decode()])[1]["records"]
        ctx.prune_tips(1)                                                   # a call that changes the result gives back what is held
        assert _status(lambda: ctx.read_links_add(reads))[0] == -5
        ctx.read_links_begin()
        ctx.entries_build()                                                 # the entries take the links' place
        assert _status(lambda: ctx.read_links_segments())[0] == -5
        ctx.entries_release()
        ctx.emit()
        assert _status(lambda: ctx.read_links_begin())[0] == -5            # after emit
    # one reverse complement deleted (an asymmetric graph): refused, naming the edge; nothing changed
    beg = next(e for e in edges if tm.revcomp(e, K + 1) != e)
    i = edges.index(tm.revcomp(beg, K + 1))
    be, bc = edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:]
    with loaded(oracle, be, bc, K) as ctx:
        st, msg = _status(lambda: ctx.read_links_begin())
        assert st == -1 and ("edge %d has no reverse complement" % be.index(beg)) in msg
        assert _status(lambda: ctx.read_links_segments())[0] == -5
        assert current(ctx) == (be, bc)
