"""The writers of the on-disk arrays (kernels_emit.hpp; emit_sparse_index, emit_dense_select, ds_plan / ds_compose,
emit_sparse_low_bits, emit_counts) over the corpus of sparse_edges.py: every file byte for byte the oracle's, at every
threshold that decides a DenseSelect block's or sub-block's form, on both sides of the switch between the two bitmap
kernels, through every branch of the window kernel, for every D that changes a branch of the split and every column
layout, for counts on both sides of every width of the VariableByteArray -- from one context, and cut into ranges
whose edges fall on and beside the blocks' edges.  No tolerance anywhere: equality with the oracle."""
import bisect

import numpy as np
import pytest

import gossamer_amd as g
from gossamer_amd import dist as gd
import sparse_edges as se

pytestmark = pytest.mark.gpu


def _device_keys(keys, words):
    import torch
    return torch.tensor(se.key_tensor_values(keys, words), dtype=torch.int64, device="cuda")


def _host_keys(vals, words):
    if words == 1:
        return np.array([int(v) for v in vals], dtype=np.uint64)
    return np.array([[v & se.MASK64, v >> 64] for v in vals], dtype=np.uint64).reshape(-1, 2)


def _ints(a, words):
    a = np.asarray(a)
    if words == 1:
        return [int(x) for x in a.reshape(-1)]
    a = a.reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[:, 0], a[:, 1])]


def _clean(rep):
    return rep["select"] == 0 and rep["rank"] == 0 and rep["access"] == 0 and rep["failures"] == 0


def _queries(c):
    """(ranks to select, keys to rank): the first and last element of every tagged block and sub-block and the
    elements beside them; for a tagged stretch of zeros the elements around the high parts it stands for; those
    elements as keys, and the keys one below and one above each"""
    marks = se.realised(c)[1]
    highs = [c.high(i) for i in range(c.m)]
    ranks = {0, c.m - 1}
    keys = {0, c.N_end - 1}
    if c.m <= 1000:
        ranks |= set(range(c.m))
    for f, n in marks[1]:
        ranks |= {f - 1, f, f + 1, f + n - 2, f + n - 1, f + n}
    for f, n in marks[0]:
        for j in (f, f + n - 1):
            r = bisect.bisect_right(highs, j)
            ranks |= {r - 1, r, bisect.bisect_left(highs, j)}
            if c.D < 128:
                keys |= {j << c.D, (j << c.D) - 1, ((j + 1) << c.D) - 1, (j + 1) << c.D}
    ranks = sorted(r for r in ranks if 0 <= r < c.m)
    for r in ranks:
        keys |= {c.keys[r], c.keys[r] - 1, c.keys[r] + 1}
    return ranks, sorted(q for q in keys if 0 <= q < c.N_end)


@pytest.mark.parametrize("name", se.BARE)
def test_bare_array_is_the_oracles(oracle, name):
    import torch
    c = se.case(name)
    exp = se.expected(oracle, name)
    t = _device_keys(c.keys, c.words)
    ones = torch.ones(c.m, dtype=torch.int32, device="cuda")
    with g.Context(31 if c.words == 1 else 63, g.MODE_KMER_SET, hbm_budget=512 << 20) as ctx:
        ctx.push_run(t.data_ptr(), ones.data_ptr(), c.m)
        ctx.finish()
        got = ctx.emit_sparse_array(t.data_ptr(), c.words, c.m, c.N, c.M, c.N_end)
        diff = se.first_difference(got, exp)
        assert diff is None, (name, diff)
        for who, files in (("device", got), ("oracle", exp)):
            rep = ctx.check_index(files)
            assert _clean(rep), (name, who, rep)
    ranks, keys = _queries(c)
    with g.Object.open({"sa" + n: b for n, b in got.items()}, "sa", g.OBJECT_SPARSE_ARRAY) as obj:
        assert obj.count == c.m and obj.D == c.D and obj.N == c.N_end, name
        w = obj.key_words
        sel = _ints(obj.select(np.array(ranks, dtype=np.uint64)), w)
        assert sel == [c.keys[r] for r in ranks], (name, next((r, a, c.keys[r]) for r, a in zip(ranks, sel) if a != c.keys[r]))
        r, p = obj.rank(_host_keys(keys, w))
        want = [se.expect_rank(c.keys, q) for q in keys]
        got_rp = list(zip([int(x) for x in r], [bool(x) for x in p]))
        assert got_rp == want, (name, next((q, a, b) for q, a, b in zip(keys, got_rp, want) if a != b))


def test_a_high_part_of_two_to_the_64_is_refused(oracle):
    """where the oracle's push_back refuses ("high bits do not fit 64 bits"), so does the writer"""
    positions, N, M, N_end = se.REFUSED
    with pytest.raises(oracle.OracleError):
        oracle.write_sparse_array(positions, N, M, N_end=N_end)
    t = _device_keys(positions, 2)
    with g.Context(63, g.MODE_KMER_SET, hbm_budget=256 << 20) as ctx:
        with pytest.raises(g.GossGpuError) as e:
            ctx.emit_sparse_array(t.data_ptr(), 2, len(positions), N, M, N_end)
        assert e.value.status == -8, e.value          # GOSS_ERR_TOO_LARGE


@pytest.mark.parametrize("name", se.GRAPHS)
def test_counts_are_written_and_read_back(oracle, name):
    import torch
    c = se.case(name)
    exp = se.expected(oracle, name)
    t = _device_keys(c.keys, 1)
    cnt = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in c.counts], dtype=torch.int32, device="cuda")
    with g.Context(se.K_GRAPH, g.MODE_GRAPH, hbm_budget=256 << 20) as ctx:
        ctx.push_run(t.data_ptr(), cnt.data_ptr(), c.m)
        ctx.finish()
        got = ctx.emit()
    diff = se.first_difference(got, exp)
    assert diff is None, (name, "pushed run", diff)
    # the oracle's files read back on the device (the VariableByteArray's read side) and written again
    with g.Context(se.K_GRAPH, g.MODE_GRAPH, hbm_budget=256 << 20) as ctx:
        ctx.push_run_graph(exp, 2 * se.K_GRAPH + 2)
        ctx.finish()
        again = ctx.emit()
    diff = se.first_difference(again, exp)
    assert diff is None, (name, "read back", diff)
    with g.Object.open({"gr" + n: b for n, b in got.items()}, "gr", g.OBJECT_GRAPH) as obj:
        mult = obj.multiplicity(np.arange(c.m, dtype=np.uint64))
        assert [int(x) for x in mult] == c.counts, name


@pytest.mark.parametrize("name", se.RANGED)
def test_ranges_build_the_oracles_kmer_set(oracle, name):
    """The case as a k-mer set over several contexts, each holding a contiguous slice (group_emit: every range's owner
    builds the blocks inside its own ones and zeros, the assembler those that straddle two ranges, from the bitmap).
    Which blocks come from where is the model's (sparse_edges.ranges_model); the counters must agree with it."""
    import torch
    c = se.case(name)
    k, estimate = se.kmer_universe(c)
    exp = se.strip(oracle.write_kmer_set(c.keys, k, M=estimate, out="ks"), "ks")
    t = _device_keys(c.keys, 1)
    ones = torch.ones(c.m, dtype=torch.int32, device="cuda")
    for label, cuts in se.range_groups(c):
        built, nb, _ = se.ranges_model(c, k, cuts)
        bounds = [0] + cuts + [c.m]
        ctxs = [g.Context(k, g.MODE_KMER_SET, hbm_budget=256 << 20) for _ in bounds[1:]]
        try:
            for ctx, a, b in zip(ctxs, bounds, bounds[1:]):
                if b > a:
                    ctx.push_run(t[a:].data_ptr(), ones.data_ptr(), b - a)
                ctx.finish()
            g.group_emit(ctxs, estimate)
            from_ranges, assembled = ctxs[0].stat("ds_blocks_from_ranges"), ctxs[0].stat("ds_blocks_assembled")
            got = gd.assemble_files([ctx.files() for ctx in ctxs])
        finally:
            for ctx in ctxs:
                ctx.close()
        diff = se.first_difference(got, exp)
        assert diff is None, (name, label, cuts, diff)
        assert from_ranges == len(built[0]) + len(built[1]), (name, label, from_ranges, assembled)
        assert from_ranges + assembled == nb[0] + nb[1], (name, label, from_ranges, assembled, nb)
