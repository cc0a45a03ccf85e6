"""The kernels that stage a tile of reads, at the edges the layout gives them (match_edges.py: tile, run and halo
edges, the key widths 31 / 32 / 63, window lengths down to 1, every byte value): Object.match_reads against
match_model.match, Context.mark_reads against components_model.marks, and the 256 byte values through the build path
against the oracle's count.  Every comparison is exact.  test_match_edges_cpu.py holds the corpus to what it claims."""
import numpy as np
import pytest

import components_model as cpm
import dense_graphs as dg
import gossamer_amd as g
import match_edges as me
import tips_cases
from test_gpu_match import check
from test_gpu_rem32 import env
from test_gpu_tips import loaded

pytestmark = pytest.mark.gpu

INFO = ("reads", "windows", "hits", "matched_reads")


def open_object(oracle, keys, K, graph):
    elems = sorted(keys)
    if graph:
        return g.Object.open(oracle.write_graph(elems, [1] * len(elems), K, out="x"), "x", g.OBJECT_GRAPH)
    return g.Object.open(oracle.write_kmer_set(elems, K, out="x"), "x", g.OBJECT_KMER_SET)


# ---- match_reads -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in me.MATCHED])
def test_match_reads_at_the_edges(name, oracle):
    """every input of the length class, both modes, every normalize value the class is run with: from bytes, and from
    a device tensor that begins one byte past an 8-byte boundary (the byte-wise loads of match_load8)"""
    import torch
    _, K, graph = next(c for c in me.MATCHED if c[0] == name)
    L = me.length_of(K, graph)
    objects = {}
    try:
        for run, data, nz, keys in me.runs(K, graph):
            if keys not in objects:
                objects[keys] = open_object(oracle, keys, K, graph)
                assert objects[keys].key_words == (1 if 2 * L <= 62 else 2) and objects[keys].count == len(keys)
            obj = objects[keys]
            want = {a: me.expected(K, graph, run, a) for a in (False, True)}
            try:
                check(obj, data, L, keys, nz, want)
                t = torch.from_numpy(np.frombuffer(b"\n" + data, dtype=np.uint8).copy()).cuda()[1:]
                assert t.data_ptr() % 8 == 1
                for any_mode in (False, True):
                    ew, eh, es, einfo = want[any_mode]
                    w, h, s, info = obj.match_reads(t, normalize=nz, any=any_mode, starts=True)
                    assert w.cpu().numpy().view(np.uint32).tolist() == ew, "windows, unaligned"
                    assert h.cpu().numpy().view(np.uint32).tolist() == eh, "hits, unaligned (any=%s)" % any_mode
                    assert s.cpu().numpy().view(np.uint64).tolist() == es, "starts, unaligned"
                    assert {n: info[n] for n in INFO} == einfo
            except AssertionError as e:
                raise AssertionError("%s / %s: %s" % (name, run, e)) from e
    finally:
        for obj in objects.values():
            obj.close()


# ---- mark_reads ------------------------------------------------------------------------------------------------------

def check_marks(ctx, edges, K, data):
    marked, windows, hits = cpm.marks(edges, K, data)
    info = ctx.mark_reads(data)
    assert (info["windows"], info["hits"]) == (windows, hits)
    assert info["marked_total"] == sum(marked)
    assert ctx.marks().tolist() == marked
    ctx.components_release()
    return windows, hits, sum(marked)


@pytest.mark.parametrize("K", me.GRAPH_KS)
def test_mark_reads_at_the_edges(oracle, K):
    """the graph of the sweep -- the planted edge and its reverse complement -- marked by both sweeps; the hand-made
    graph of the width marked by the byte values within a stretch of its own text and within a foreign one"""
    L = K + 1
    edges = sorted(me.planted_keys(L, True, False))
    with loaded(oracle, edges, [1, 1], K) as ctx:
        assert ctx.counts.key_words == me.key_words(L)
        for phase in me.PHASES:
            windows, hits, marked = check_marks(ctx, edges, K, me.sweep(L, phase, True)[0])
            assert (hits, marked) == (L + 2, 2) and windows > 1900 * (L + 2)
        assert check_marks(ctx, edges, K, me.byte_input(L))[1:] == (0, 0)
    edges, counts, _ = tips_cases.combined_graph(K)
    core = next(s for s, _ in tips_cases.combined(K)[0] if len(s) >= 2 * L + 1)[:2 * L + 1].encode()
    with loaded(oracle, edges, counts, K) as ctx:
        windows, hits, marked = check_marks(ctx, edges, K, me.byte_input(L, core))
        # the core's own middle base, in either case, keeps every window an edge; any other byte leaves the two windows
        # beside it
        assert windows == 8 * (L + 2) + 2 * 248 and hits == 2 * (L + 2) + 2 * 254 and marked == L + 2
        assert check_marks(ctx, edges, K, me.byte_input(L))[0] == windows


@pytest.mark.parametrize("K", [2, 5])
def test_mark_reads_on_dense_graphs(oracle, K):
    """L = 3 and 6 on the two largest graphs of the dense corpus at that K: the complete graph, where every window is
    an edge, and a random one, where some are"""
    L = K + 1
    graphs = sorted((gr for gr in dg.corpus() if gr[1] == K), key=lambda gr: -len(gr[2]))[:2]
    assert len(graphs[0][2]) == 4 ** L > len(graphs[1][2])
    for name, _, edges, counts in graphs:
        with loaded(oracle, edges, counts, K) as ctx:
            for data in (me.small_sweep(L), me.byte_input(L)):
                windows, hits, marked = check_marks(ctx, edges, K, data)
                assert windows > 0 and (hits == windows if len(edges) == 4 ** L else 0 < hits < windows), name


# ---- the extraction kernels ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,graph", [(25, False), (31, True), (3, False)])
def test_every_byte_value_through_the_build_path(oracle, K, graph):
    """The extraction kernels decode the 256 byte values as the oracle does.  With GOSS_GPU_FUSED_MIN=0 the fused path
    samples the input with its own kernels and then declines it: it wants 2^20 keys (the next test brings them)."""
    L = me.length_of(K, graph)
    data = me.byte_input(L)
    ekeys, ecounts, _, nwin = oracle.count([(oracle.LINE, "reads", data)], L, 1 if graph else 0)
    assert nwin == 8 * (L + 2) + 2 * 248
    for fused in ({}, {"GOSS_GPU_FUSED_MIN": 0}):
        with env(**fused):
            with g.Context(K, g.MODE_GRAPH if graph else g.MODE_KMER_SET, hbm_budget=256 << 20) as ctx:
                ctx.push_host(data)
                c = ctx.finish()
                keys, counts = ctx.result()
        assert c.windows == nwin, fused
        assert keys == ekeys and counts.tolist() == ecounts, fused


@pytest.mark.parametrize("K,graph", [(25, False), (31, True)])
def test_every_byte_value_through_the_fused_kernels(oracle, K, graph):
    """The same 256 reads 1 600 times over, 21 and 27 MB: more than 2^20 windows of a few hundred distinct keys, which
    the fused path takes when GOSS_GPU_FUSED_MIN=0 lets it.  Every key comes 1 600 times as often as in one copy."""
    L = me.length_of(K, graph)
    copies = 1600
    data = me.byte_input(L)
    ekeys, ecounts, _, nwin = oracle.count([(oracle.LINE, "reads", data)], L, 1 if graph else 0)
    assert copies * nwin > 1 << 20
    with env(GOSS_GPU_FUSED_MIN=0):
        # (room for the whole input as one chunk: a part of it would be too few keys again)
        with g.Context(K, g.MODE_GRAPH if graph else g.MODE_KMER_SET, hbm_budget=8 << 30) as ctx:
            ctx.push_host(data * copies)
            c = ctx.finish()
            keys, counts = ctx.result()
            assert ctx.stat("fused_chunks") == 1
    assert c.windows == copies * nwin
    assert keys == ekeys and counts.tolist() == [copies * n for n in ecounts]
