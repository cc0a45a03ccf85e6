"""merge_runs at its limits: the segment merge, the table merge and the general path, and the bookkeeping of counts
that do not fit 32 bits, against the model of merge_model.py (a dict of big integers, itself checked against the
oracle's merge in test_merge_model_cpu.py).

Every case: runs from the model's builders, pushed alternately from device tensors and from host memory, one finish;
result keys, counts, big_counts() and the emitted files against the model and the oracle's writers; and the path
taken (seg_merges / hash_merges), since a case that took another path has tested nothing.

All contexts get 256 MB and totals stay below 2^18 entries: the segment merge starts at 8 segment bits (a segment =
a key's top 8 bits, merge_model.segment) and retries at 10 and 12.

Counts: a pushed count 0xFFFFFFFF is the number 2^32 - 1 -- summed as such in a merge, and listed by big_counts() like
any count that large, also when its run is the only one and nothing is merged."""
import os
import subprocess

import numpy as np
import pytest

import gossamer_amd as g
import merge_model as mm

pytestmark = pytest.mark.gpu

U32 = mm.U32
GRAPH, KMER = mm.GRAPH, mm.KMER
BUDGET = 256 << 20
M64 = (1 << 64) - 1
ERR_COUNT_OVERFLOW = -7

# (mode, k): one-word keys, the widest one-word key, 64 bits in two words, the first key with a high word, the widest
KMER_LENGTHS = [(KMER, 4), (KMER, 5), (KMER, 13), (KMER, 31), (KMER, 32), (KMER, 33), (KMER, 63)]
GRAPH_LENGTHS = [(GRAPH, 27), (GRAPH, 31), (GRAPH, 55), (GRAPH, 56), (GRAPH, 62)]
LENGTHS = KMER_LENGTHS + GRAPH_LENGTHS
DENSE_LENGTHS = [v for v in LENGTHS if mm.key_bits(v[1], v[0]) >= 26]          # (a dense layout needs 26 bits)


class env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _suffix_map(files, prefix):
    return {k[len(prefix):]: v for k, v in files.items()}


def _arrays(run, words):
    keys = np.empty(len(run) * words, dtype=np.uint64)
    if words == 1:
        keys[:] = [k for k, _ in run]
    else:
        keys[0::2] = [k & M64 for k, _ in run]
        keys[1::2] = [k >> 64 for k, _ in run]
    return keys, np.array([c for _, c in run], dtype=np.uint32)


def _push(ctx, runs):
    """even runs from device tensors (push_run), odd ones from host memory (push_run_host)"""
    import torch
    words = ctx.key_words
    for i, run in enumerate(runs):
        assert run, "an empty run is not pushed and would change the number of runs"
        keys, counts = _arrays(run, words)
        if i % 2 == 0:
            dk = torch.from_numpy(keys.view(np.int64)).cuda()
            dc = torch.from_numpy(counts.view(np.int32)).cuda()
            ctx.push_run(dk.data_ptr(), dc.data_ptr(), len(run))
        else:
            ctx.push_run_host(keys.ctypes.data, counts.ctypes.data, len(run))


def _check(ctx, oracle, mode, k, runs):
    """the finished context against the model of `runs`"""
    want = mm.merge(runs, mode)
    assert ctx.stat("runs") == 1
    keys, counts = ctx.result()
    assert keys == want.keys
    got = [int(c) for c in counts]
    if got != want.u32:
        bad = [(hex(key), e, c) for key, e, c, w in zip(want.keys, want.exact, got, want.u32) if c != w]
        raise AssertionError("counts differ (key, exact, stored): %s" % bad[:5])
    assert ctx.big_counts() == want.big
    files = ctx.emit()
    if mode == GRAPH:
        exp = _suffix_map(oracle.write_graph(want.keys, want.exact, k, out="o"), "o")
    else:
        exp = _suffix_map(oracle.write_kmer_set(want.keys, k, out="o"), "o")
    assert sorted(files) == sorted(exp)
    for name in exp:
        assert files[name] == exp[name], name
    return want


def _merge(oracle, mode, k, runs, seg_merges=None, hash_merges=None, **e):
    with env(**e):
        with g.Context(k, g.MODE_GRAPH if mode == GRAPH else g.MODE_KMER_SET, hbm_budget=BUDGET) as ctx:
            assert ctx.key_words == mm.key_words(mm.key_bits(k, mode))
            _push(ctx, runs)
            ctx.finish()
            path = (ctx.stat("seg_merges"), ctx.stat("hash_merges"))
            want = _check(ctx, oracle, mode, k, runs)
    if seg_merges is not None:
        assert path[0] == seg_merges, "seg_merges %d, hash_merges %d" % path
    if hash_merges is not None:
        assert path[1] == hash_merges, "seg_merges %d, hash_merges %d" % path
    return want


def _id(v):
    return "%s%d" % v if isinstance(v, tuple) else None


# ---- structure: which path, at which limit ------------------------------------------------------------------------
@pytest.mark.parametrize("total,seg_merges", [(1023, 0), (1024, 1)])
@pytest.mark.parametrize("length", LENGTHS, ids=_id)
def test_smallest_total_of_the_segment_merge(oracle, length, total, seg_merges):
    """total >= 1024 takes the segment merge, 1023 the general path.  Two runs (five at k = 4, whose 256 keys do not
    make 1 024 entries in two)."""
    mode, k = length
    bits = mm.key_bits(k, mode)
    case = mm.build_case(bits, 5 if bits == 8 else 2, total, seed=7 * bits + total)
    _merge(oracle, mode, k, case.runs, seg_merges=seg_merges, hash_merges=0)


@pytest.mark.parametrize("nruns,seg_merges", [(64, 1), (65, 0)])
@pytest.mark.parametrize("length", LENGTHS, ids=_id)
def test_most_runs_of_the_segment_merge(oracle, length, nruns, seg_merges):
    """64 runs (kMergeRuns; one key sits in all 64: ties in every sub-run of its segment) against 65"""
    mode, k = length
    bits = mm.key_bits(k, mode)
    case = mm.build_case(bits, nruns, 4000 + nruns, seed=11 * bits + nruns)
    _merge(oracle, mode, k, case.runs, seg_merges=seg_merges, hash_merges=0)


@pytest.mark.parametrize("layout,seg_merges", [(("cluster", 2048), 1), (("spread", 2049), 1), (("cluster", 2049), 0)])
@pytest.mark.parametrize("length", DENSE_LENGTHS, ids=_id)
def test_fullest_segment_of_the_segment_merge(oracle, length, layout, seg_merges):
    """64 runs x 32 entries under one 8-bit prefix = kMergeCap: taken.  One more, spread over the four 10-bit
    sub-prefixes: the second attempt takes it.  One more in a cluster that shares every bit above its low 12 -- one
    segment at 8, 10 and 12 bits alike: all three attempts decline, the general path merges.  (The 2 048 are such a
    cluster as well: a cap compared one too low would decline them three times.)"""
    mode, k = length
    bits = mm.key_bits(k, mode)
    case = mm.build_case(bits, 64, 6000, seed=13 * bits + layout[1], dense=layout)
    n = layout[1]
    assert mm.segment_totals(case.runs, bits, 8)[mm.DENSE_SEG] == n == max(mm.segment_totals(case.runs, bits, 8).values())
    if layout[0] == "cluster":
        assert max(mm.segment_totals(case.runs, bits, 12).values()) == n
    else:
        assert max(mm.segment_totals(case.runs, bits, 10).values()) <= mm.MERGE_CAP
    _merge(oracle, mode, k, case.runs, seg_merges=seg_merges, hash_merges=0)


@pytest.mark.parametrize("nruns", [5, 64])
@pytest.mark.parametrize("length,e,hash_merges", [
    ((GRAPH, 55), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1),             # 112 bits: the widest key the table takes
    ((GRAPH, 55), {"GOSS_GPU_HASH_MERGE_MIN": 1, "GOSS_GPU_NO_TABLE96": 1}, 0),
    ((GRAPH, 56), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 0),             # 114 bits: too wide
    ((GRAPH, 31), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1),             # 64 bits, high word always 0: 48-bit remainders
    ((KMER, 33), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1),              # 66 bits
    ((KMER, 55), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1),
    ((KMER, 63), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 0),
    ((KMER, 31), {"GOSS_GPU_HASH_MERGE_MIN": 1}, 0),              # one-word keys never go there
], ids=lambda v: _id(v) if isinstance(v, tuple) else ("no_table96" if isinstance(v, dict) and len(v) > 1 else None))
def test_table_merge_taken_and_not(oracle, length, e, hash_merges, nruns):
    """two-word keys of at most 16 + 96 bits are merged by hash inserts (seg_hash_merge96_kernel) when the total reaches
    GOSS_GPU_HASH_MERGE_MIN; everything else, and everything under GOSS_GPU_NO_TABLE96, by the segment merge"""
    mode, k = length
    bits = mm.key_bits(k, mode)
    case = mm.build_case(bits, nruns, 3000, seed=17 * bits + nruns)
    _merge(oracle, mode, k, case.runs, seg_merges=1, hash_merges=hash_merges, **e)


# ---- counts around 2^32 ----------------------------------------------------------------------------------------------
# (path name, k of a graph, runs, total, environment, seg_merges, hash_merges)
SEG = ("segment", 64, 4000, {}, 1, 0)
GENERAL = ("general", 65, 4000, {}, 0, 0)
SMALL = ("general-small", 2, 1000, {}, 0, 0)
TABLE = ("table-declines", 64, 4000, {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1, 0)       # K = 55 only: a sum of 2^31 or more sends it on
COUNT_PATHS = [(27,) + SEG, (62,) + SEG, (27,) + GENERAL, (62,) + GENERAL, (27,) + SMALL, (56,) + SMALL, (55,) + TABLE]


def _path_id(p):
    return "%s-K%d" % (p[1], p[0])


def _stored(want, key):
    i = want.keys.index(key)
    return want.exact[i], want.u32[i]


@pytest.mark.parametrize("path", COUNT_PATHS, ids=_path_id)
def test_sums_around_two_to_the_32(oracle, path):
    """2^32 - 2 is stored as it is; 2^32 - 1 and more are kept exactly beside the run and stored modulo 2^32 -- whether
    the sum is made of two parts or of one from every run, and whether a part is itself the stored count 2^32 - 1"""
    K, _, nruns, total, e, seg_merges, hash_merges = path
    bits = mm.key_bits(K, GRAPH)
    case = mm.build_case(bits, nruns, total, seed=19 * bits + nruns, sums=mm.count_sums(nruns))
    want = _merge(oracle, GRAPH, K, case.runs, seg_merges=seg_merges, hash_merges=hash_merges, **e)
    p = case.placed
    n = min(nruns, 64)
    assert _stored(want, p["2^32-2"]) == (2 ** 32 - 2, 0xFFFFFFFE) and p["2^32-2"] not in want.big
    assert _stored(want, p["2^32-2 in %d parts" % n]) == (2 ** 32 - 2, 0xFFFFFFFE)
    assert _stored(want, p["2^32-1 as 2 + (2^32-3)"]) == (2 ** 32 - 1, 0xFFFFFFFF)
    assert _stored(want, p["2^32-1 in %d parts" % n]) == (2 ** 32 - 1, 0xFFFFFFFF)
    assert _stored(want, p["2^32"]) == (2 ** 32, 0) and _stored(want, p["2^32 as halves"]) == (2 ** 32, 0)
    assert _stored(want, p["2^32+1"]) == (2 ** 32 + 1, 1)
    assert _stored(want, p["literal 2^32-1 alone"]) == (2 ** 32 - 1, 0xFFFFFFFF)
    assert _stored(want, p["literal 2^32-1 plus 1"]) == (2 ** 32, 0)
    if nruns >= 64:
        assert _stored(want, p["64 x (2^32-2)"]) == (64 * (2 ** 32 - 2), (64 * (2 ** 32 - 2)) & U32)
    assert set(want.big) == set(p.values()) - {p["2^32-2"], p["2^32-2 in %d parts" % n]}


@pytest.mark.parametrize("parts", [2, 64])
@pytest.mark.parametrize("path", [(27,) + SEG, (62,) + SEG, (27,) + GENERAL, (62,) + GENERAL, (27,) + SMALL, (56,) + SMALL], ids=_path_id)
def test_one_sum_of_exactly_two_to_the_32_minus_1(oracle, path, parts):
    """the only count of the merge that does not fit: nothing else raises the overflow flag for it, so the comparison
    that does (sum >= 2^32 - 1, in seg_merge_kernel and in run_sums_kernel) is what puts it into big_counts()"""
    K, _, nruns, total, e, seg_merges, hash_merges = path
    bits = mm.key_bits(K, GRAPH)
    form = [2, U32 - 2] if parts == 2 else mm.split(U32, min(nruns, 64))
    case = mm.build_case(bits, nruns, total, seed=59 * bits + nruns + parts, sums=[("edge", form), ("below", [U32 - 2, 1])])
    want = _merge(oracle, GRAPH, K, case.runs, seg_merges=seg_merges, hash_merges=hash_merges, **e)
    assert want.big == {case.placed["edge"]: 2 ** 32 - 1}
    assert _stored(want, case.placed["below"]) == (2 ** 32 - 2, 0xFFFFFFFE)


@pytest.mark.parametrize("path", [(27,) + SEG, (62,) + SEG, (27,) + SMALL, (56,) + SMALL,
                                  (55, "table-declines", 2, 4000, {"GOSS_GPU_HASH_MERGE_MIN": 1}, 1, 0)], ids=_path_id)
def test_pushed_count_of_two_to_the_32_minus_1_beside_a_disjoint_run(oracle, path):
    """an input count 0xFFFFFFFF is that number even when no other run holds its key: two runs without a common key"""
    K, _, _, total, e, seg_merges, hash_merges = path
    bits = mm.key_bits(K, GRAPH)
    case = mm.build_case(bits, 2, total, seed=23 * bits + total, disjoint=True, sums=[("literal", [U32])])
    want = _merge(oracle, GRAPH, K, case.runs, seg_merges=seg_merges, hash_merges=hash_merges, **e)
    assert want.big == {case.placed["literal"]: 2 ** 32 - 1}


@pytest.mark.parametrize("K", [27, 55])
def test_pushed_count_of_two_to_the_32_minus_1_in_a_single_run(oracle, K):
    """one pushed run, no merge at all: the result still lists the count beside the run"""
    bits = mm.key_bits(K, GRAPH)
    case = mm.build_case(bits, 1, 1500, seed=29 * bits, sums=[("literal", [U32]), ("2^32-2", [U32 - 1])])
    want = _merge(oracle, GRAPH, K, case.runs, seg_merges=0, hash_merges=0)
    assert want.big == {case.placed["literal"]: 2 ** 32 - 1}


@pytest.mark.parametrize("what,hash_merges", [("sum 2^31-1", 1), ("sum 2^31", 0), ("count 2^31", 0)])
def test_table_merge_gives_up_at_two_to_the_31(oracle, what, hash_merges):
    """K = 55 through the table: a slot's count may reach 2^31 - 1; a sum of 2^31, or one input count of 2^31, sends
    the merge to the segment merge, which must then be right"""
    sums = {"sum 2^31-1": [("edge", mm.split(2 ** 31 - 1, 64)), ("edge2", [2 ** 31 - 2, 1])],
            "sum 2^31": [("edge", mm.split(2 ** 31, 64))],
            "count 2^31": [("edge", [2 ** 31])]}[what]
    bits = mm.key_bits(55, GRAPH)
    case = mm.build_case(bits, 64, 4000, seed=31 * len(what), sums=sums)
    want = mm.merge(case.runs, GRAPH)
    top = max(want.exact)
    assert top == {"sum 2^31-1": 2 ** 31 - 1, "sum 2^31": 2 ** 31, "count 2^31": 2 ** 31}[what]
    assert sorted(want.exact)[-3] < 2 ** 28          # (nothing else comes near)
    _merge(oracle, GRAPH, 55, case.runs, seg_merges=1, hash_merges=hash_merges, GOSS_GPU_HASH_MERGE_MIN=1)


def _big_sums(n, max_parts):
    forms = [[U32], [2, U32 - 2], [U32, U32], [U32 - 6, 7], [1 << 31, 1 << 31, 5], [U32, 1, 1]]
    forms = [f for f in forms if len(f) <= max_parts]
    return [("big%d" % i, forms[i % len(forms)]) for i in range(n)] + [("2^32-2", [U32 - 2, 1])]


@pytest.mark.parametrize("path", [(27,) + SEG, (62,) + GENERAL, (27,) + SMALL, (55,) + TABLE], ids=_path_id)
def test_256_keys_beyond_32_bits_and_one_more(oracle, path):
    """256 keys at or above 2^32 - 1 (kMaxBig) are all kept; with 257 finish refuses with GOSS_ERR_COUNT_OVERFLOW, and
    after a reset the same context merges an ordinary case"""
    K, _, nruns, total, e, seg_merges, hash_merges = path
    bits = mm.key_bits(K, GRAPH)
    case = mm.build_case(bits, nruns, total, seed=37 * bits, sums=_big_sums(256, min(nruns, 3)))
    want = _merge(oracle, GRAPH, K, case.runs, seg_merges=seg_merges, hash_merges=hash_merges, **e)
    assert len(want.big) == 256 and case.placed["2^32-2"] not in want.big
    over = mm.build_case(bits, nruns, total, seed=41 * bits, sums=_big_sums(257, min(nruns, 3)))
    assert len(mm.merge(over.runs, GRAPH).big) == 257
    plain = mm.build_case(bits, nruns, total, seed=43 * bits)
    with env(**e):
        with g.Context(K, g.MODE_GRAPH, hbm_budget=BUDGET) as ctx:
            _push(ctx, over.runs)
            with pytest.raises(g.GossGpuError) as err:
                ctx.finish()
            assert err.value.status == ERR_COUNT_OVERFLOW, str(err.value)
            ctx.reset()
            _push(ctx, plain.runs)
            ctx.finish()
            _check(ctx, oracle, GRAPH, K, plain.runs)
            assert ctx.big_counts() == {}


@pytest.mark.parametrize("path", [(27,) + SEG, (62,) + SEG, (27,) + GENERAL, (63,) + SMALL], ids=_path_id)
def test_kmer_set_counts_saturate(oracle, path):
    """a k-mer set stores no counts: the same sums saturate at 0xFFFFFFFF, nothing is kept beside the run, no error --
    and 257 keys beyond 32 bits are no error either"""
    k, _, nruns, total, e, seg_merges, hash_merges = path
    bits = mm.key_bits(k, KMER)
    sums = mm.count_sums(nruns) + _big_sums(257, min(nruns, 3))[:-1]
    case = mm.build_case(bits, nruns, total, seed=47 * bits + nruns, sums=sums)
    want = _merge(oracle, KMER, k, case.runs, seg_merges=seg_merges, hash_merges=hash_merges, **e)
    p = case.placed
    assert _stored(want, p["2^32-2"]) == (2 ** 32 - 2, 0xFFFFFFFE)
    assert _stored(want, p["2^32"]) == (2 ** 32, U32) and _stored(want, p["2^32+1"]) == (2 ** 32 + 1, U32)
    assert want.big == {}


# ---- the commands ----------------------------------------------------------------------------------------------------
GOSS = os.path.join(os.path.dirname(os.path.abspath(g.__file__)), "goss")


@pytest.mark.parametrize("length", [(GRAPH, 27), (GRAPH, 55), (KMER, 25)], ids=_id)
def test_merge_commands_on_counts_around_two_to_the_32(oracle, tmp_path, length):
    """goss merge-graphs / merge-kmer-sets over three objects written by the oracle that together carry the sums above
    (an input multiplicity of 2^32 - 1 among them): every output file equal to the oracle's merge.  Three inputs,
    --max-merge 8: one pass, no narrowed intermediate object."""
    mode, k = length
    bits = mm.key_bits(k, mode)
    kind = 1 if mode == GRAPH else 0
    if kind:
        case = mm.build_case(bits, 3, 3000, seed=53 * bits, sums=mm.count_sums(3) + [("2^32+5", [U32 - 1, 7])])
        assert any(c == U32 for run in case.runs for _, c in run)
    else:
        case = mm.build_case(bits, 3, 3000, seed=53 * bits, fill_count=lambda rng: 1)
    files, names = {}, []
    for i, run in enumerate(case.runs):
        name = "in%d" % i
        keys = [key for key, _ in run]
        files.update(oracle.write_graph(keys, [c for _, c in run], k, out=name) if kind else oracle.write_kmer_set(keys, k, out=name))
        names.append(name)
    d = str(tmp_path)
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    exp = oracle.merge(files, names, kind, "out", max_merge=8)
    args = [GOSS, "merge-graphs" if kind else "merge-kmer-sets", "-O", os.path.join(d, "out"), "--max-merge", "8"]
    for name in names:
        args += ["-G", os.path.join(d, name)]
    p = subprocess.run(args + ["--hbm-budget", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-400:]
    got = {n: open(os.path.join(d, n), "rb").read() for n in os.listdir(d) if n.startswith("out.") or n.startswith("out-")}
    assert sorted(got) == sorted(exp)
    for name in exp:
        assert got[name] == exp[name], name
