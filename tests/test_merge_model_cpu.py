"""The merge model (merge_model.py) against the oracle's merge-graphs / merge-kmer-sets, on the CPU: objects written
from the model's runs, merged by the oracle in one pass, byte for byte what the oracle writes from the model's answer.
This is what entitles the device tests (test_gpu_merge_runs.py) to trust the model; the builders' own promises
are checked here too, at the layouts those tests use."""
import pytest

import merge_model as mm

U32 = mm.U32


def _case(mode, K, nruns, total, seed):
    bits = mm.key_bits(K, mode)
    if mode == mm.KMER:          # a k-mer set stores no counts: every entry is worth one
        return mm.build_case(bits, nruns, total, seed, fill_count=lambda rng: 1)
    sums = mm.count_sums(nruns) + [("2^32+5", [U32 - 1, 7])]
    return mm.build_case(bits, nruns, total, seed, sums=sums)


@pytest.mark.parametrize("mode,K", [(mm.GRAPH, 27), (mm.GRAPH, 55), (mm.KMER, 27), (mm.KMER, 55)])
@pytest.mark.parametrize("nruns,total", [(3, 500), (5, 1500), (64, 3000)])
def test_oracle_merge_is_the_model(oracle, mode, K, nruns, total):
    case = _case(mode, K, nruns, total, seed=1000 * K + nruns)
    kind = 1 if mode == mm.GRAPH else 0
    files, names = {}, []
    for i, run in enumerate(case.runs):
        keys = [k for k, _ in run]
        name = "in%d" % i
        if kind:
            files.update(oracle.write_graph(keys, [c for _, c in run], K, out=name))
        else:
            files.update(oracle.write_kmer_set(keys, K, out=name))
        names.append(name)
    got = oracle.merge(files, names, kind, "out", max_merge=max(8, nruns))
    want = mm.merge(case.runs, mode)
    M = mm.total_entries(case.runs)
    if kind:
        exp = oracle.write_graph(want.keys, want.exact, K, M=M, out="out")
        # the sums this is about are there, and an input count that is itself 2^32 - 1
        exact = dict(zip(want.keys, want.exact))
        p = case.placed
        assert exact[p["2^32-2"]] == 2 ** 32 - 2 and p["2^32-2"] not in want.big
        assert exact[p["2^32-1 as 2 + (2^32-3)"]] == 2 ** 32 - 1 and p["2^32-1 as 2 + (2^32-3)"] in want.big
        assert exact[p["2^32"]] == 2 ** 32 and exact[p["2^32+5"]] == 2 ** 32 + 5
        assert exact[p["literal 2^32-1 alone"]] == U32 and exact[p["literal 2^32-1 plus 1"]] == 2 ** 32
        assert any(c == U32 for run in case.runs for _, c in run)
    else:
        exp = oracle.write_kmer_set(want.keys, K, M=M, out="out")
    assert sorted(got) == sorted(exp)
    for name in exp:
        assert got[name] == exp[name], name


def test_model_modes():
    runs = [[(1, 2), (5, U32), (9, U32 - 1)], [(5, 1), (9, 1), (12, 7)], [(1, U32 - 3)]]
    g = mm.merge(runs, mm.GRAPH)
    assert g.keys == [1, 5, 9, 12]
    assert g.exact == [U32 - 1, 2 ** 32, U32, 7]
    assert g.u32 == [U32 - 1, 0, U32, 7]
    assert g.big == {5: 2 ** 32, 9: U32}
    k = mm.merge(runs, mm.KMER)
    assert k.exact == g.exact and k.u32 == [U32 - 1, U32, U32, 7] and k.big == {}
    for bad in ([[(3, 1), (3, 1)]], [[(4, 1), (2, 1)]], [[(1, 0)]], [[(1, 2 ** 32)]]):
        with pytest.raises(AssertionError):
            mm.merge(bad, mm.GRAPH)


@pytest.mark.parametrize("bits", [8, 10, 26, 56, 62, 64, 66, 112, 114, 126])
def test_builder_keeps_its_promises(bits):
    """(build_case asserts them itself; here: the layouts the device tests derive their witnesses from)"""
    for nruns, total in ((2, 400 if bits == 8 else 1023), (64, 4000), (65, 4100)):
        case = mm.build_case(bits, nruns, total, seed=bits * 100 + nruns)
        assert mm.total_entries(case.runs) == total and len(case.runs) == nruns
        assert max(mm.segment_totals(case.runs, bits).values()) <= mm.MERGE_CAP
        for a, b in case.pairs:
            assert a != b
        if bits == 64:               # two words, the high one always 0: the low-word pairs, each in one segment
            assert len(case.pairs) == 2 and all(a >> 64 == b >> 64 == 0 for a, b in case.pairs)
            assert all(mm.segment(a, bits) == mm.segment(b, bits) for a, b in case.pairs)
        if bits >= 64 + 10:          # long enough: both members of every pair meet in one segment
            assert len(case.pairs) == 4
            assert all(mm.segment(a, bits) == mm.segment(b, bits) for a, b in case.pairs)
            assert any((a >> 64) != (b >> 64) and (a & (2 ** 64 - 1)) == (b & (2 ** 64 - 1)) for a, b in case.pairs)
            assert any(a + 1 == b and (a & (2 ** 64 - 1)) == 2 ** 64 - 1 for a, b in case.pairs)
    if bits >= 26:
        for kind, n, at10, at12 in (("cluster", 2048, 2048, 2048), ("cluster", 2049, 2049, 2049), ("spread", 2049, 513, None)):
            case = mm.build_case(bits, 64, 6000, seed=bits, dense=(kind, n))
            assert mm.segment_totals(case.runs, bits, 8)[mm.DENSE_SEG] == n
            assert max(mm.segment_totals(case.runs, bits, 10).values()) == at10
            if at12:
                assert max(mm.segment_totals(case.runs, bits, 12).values()) == at12
        case = mm.build_case(bits, 2, 1500, seed=bits, disjoint=True, sums=[("lit", [U32])])
        assert not set(k for k, _ in case.runs[0]) & set(k for k, _ in case.runs[1])
