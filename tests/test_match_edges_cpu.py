"""The edge corpus of match_edges.py held to what it claims, with the models alone (match_model.py, components_model.py)
and the oracle.  These are conditions on the corpus: an input that fails one of them is wrong."""
import pytest

import components_model as cpm
import match_edges as me
import match_model as mm

LONG = [(K, graph) for _, K, graph in me.MATCHED if me.length_of(K, graph) >= 16]
SMALL = [K for _, K, graph in me.CLASSES if K <= 6]


def test_the_length_classes_reach_both_key_widths():
    lengths = sorted(me.length_of(K, graph) for _, K, graph in me.CLASSES)
    assert lengths == [1, 2, 3, 6, 16, 31, 31, 32, 32, 33, 62, 63, 63]
    assert [me.key_words(L) for L in (31, 32, 63)] == [1, 2, 2]
    assert set(me.NEWLINE_LENGTHS) <= set(lengths) and 32 in me.BYTE_LENGTHS and 3 in me.BYTE_LENGTHS


@pytest.mark.parametrize("K,graph", LONG)
def test_sweep_plants_one_hit_a_read_at_every_residue(K, graph):
    L = me.length_of(K, graph)
    for nz in ((False,) if graph else (False, True)):
        keys = me.planted_keys(L, graph, nz)
        assert len(keys) == (2 if graph else 1)
        for phase in me.PHASES:
            data, where = me.sweep(L, phase, graph or nz)
            spans = mm.read_spans(data)
            assert len(spans) == len(where) == L + 2
            # the planted windows: d = 0 .. L + 1, each at phase - d (mod 2 048), each inside its read
            assert [d for d, _ in where] == list(range(L + 2))
            x, both = me.planted(L)
            for (d, at), (b, e) in zip(where, spans):
                assert at % me.TILE == (phase - d) % me.TILE
                assert b < at and at + L < e and data[at:at + L].upper() in both
                if d % 2:
                    assert data[at - 3] not in mm.CODE and data[at - 3] != 10
            if graph or nz:
                assert {data[at:at + L].upper() for _, at in where} == both
            nwin, nhit, starts, info = mm.match(data, L, keys, normalize=nz)
            assert nhit == [1] * (L + 2), (phase, nz)
            assert min(nwin) > 1900
            assert starts[:-1] == [b for b, _ in spans]
            # the hit is the planted window and nothing else
            assert mm.match(data, L, frozenset(), normalize=nz)[3]["hits"] == 0
            if graph:
                marked, windows, hits = cpm.marks(sorted(keys), K, data)
                assert marked == [True, True] and windows == sum(nwin) and hits == L + 2


@pytest.mark.parametrize("L", SMALL)
def test_small_sweep_has_a_hit_and_a_miss_at_every_residue(L):
    data = me.small_sweep(L)
    assert 20000 <= len(data) < 20400
    lengths = [e - b for b, e in mm.read_spans(data)]
    assert {0, 1, L - 1, L, L + 1} <= set(lengths) and max(lengths) <= 300
    for nz in (False, True):
        keys = me.small_keys(L, nz)
        seen = me.small_residues(L, data, keys, nz)
        assert sorted(seen) == list(range(L + 2))
        for d, (present, absent) in seen.items():
            assert present >= 1 and absent >= 1, (L, nz, d)
        nwin, nhit, _, info = mm.match(data, L, keys, normalize=nz)
        assert any(0 < h < w for w, h in zip(nwin, nhit))
        assert 0 < info["hits"] < info["windows"]


def by_hand(L):
    """{case: (windows, hits, starts)} written out from the construction, for every object of the newline cases"""
    T = me.TILE
    want = {
        # 2 048 bases, then the '\n' at 2 048 .. 4 095 end that read and 2 047 empty ones, then X at 4 096
        "newlines2048": ([T + 1 - L] + [0] * (T - 1) + [1], [1] + [0] * (T - 1) + [1],
                         [0] + list(range(T + 1, 2 * T + 1)) + [2 * T + L]),
        "newline_last_in_tile": ([T - L, 11], [1, 1], [0, T, T + L + 10]),
        "newline_first_in_tile": ([T + 1 - L, 11], [1, 1], [0, T + 1, T + 1 + L + 10]),
        "newlines_across_tiles": ([T - L, 0, 11], [1, 0, 1], [0, T, T + 1, T + 1 + L + 10]),
    }
    for n in me.EXACT:
        want["exact%d" % n] = ([n - L + 1], [1], [0, n])
        want["exact%dnl" % n] = ([n - L], [1], [0, n - 1])
    return want


@pytest.mark.parametrize("L", me.NEWLINE_LENGTHS)
def test_newline_cases_by_hand(L):
    cases = me.newline_cases(L)
    assert len(cases["newlines2048"]) == 2 * me.TILE + L + 1 and cases["newlines2048"][me.TILE:2 * me.TILE] == b"\n" * me.TILE
    assert cases["newline_last_in_tile"][me.TILE - 1] == 10 and cases["newline_first_in_tile"][me.TILE] == 10
    assert [cases[n].find(b"\n") % me.RUN for n in ("newline_at_63", "newline_at_64", "newlines_at_63_64")] == [63, 0, 63]
    assert len(cases["ends_with_tile"]) == me.TILE and cases["ends_with_tile"][-1] != 10
    for n in me.EXACT:
        assert len(cases["exact%d" % n]) == len(cases["exact%dnl" % n]) == n
        assert cases["exact%d" % n][-1] != 10 and cases["exact%dnl" % n][-1] == 10
    want = by_hand(L)
    x, both = me.planted(L)
    for graph, nz in ((False, False), (False, True), (True, False)):
        keys = me.planted_keys(L, graph, nz)
        for name, data in cases.items():
            assert me.occurrences(data, both) == data.count(x) >= 1, name          # X only, forward, upper case
            for any_mode in (False, True):
                nwin, nhit, starts, info = mm.match(data, L, keys, normalize=nz, any=any_mode)
                assert info["hits"] == data.count(x), name
                if name in want:
                    assert (nwin, nhit, starts) == want[name], name
                    assert info == {"reads": len(nwin), "windows": sum(nwin), "hits": sum(nhit), "matched_reads": sum(nhit)}
    # the reads over three tiles: one read, one hit, in the first and in the last tile
    for name, tile in (("three_tiles_hit_in_first", 0), ("three_tiles_hit_in_last", 2)):
        data = cases[name]
        assert data.count(b"\n") == 1 and (len(data) - 2) // me.TILE == 2 and data.find(x) // me.TILE == tile
    assert mm.match(cases["one_base_reads"], L, me.planted_keys(L, False, False))[0].count(0) >= 1170


@pytest.mark.parametrize("L", me.BYTE_LENGTHS)
def test_byte_values_split_as_the_decoder_must(L, oracle):
    data = me.byte_input(L)
    keys = mm.object_keys(data, L, False)
    nwin, nhit, starts, info = mm.match(data, L, keys, normalize=True)
    assert info["reads"] == 257 and nhit == nwin
    # the eight bases keep every window of the core; '\n' makes two reads of L bases; every other byte cuts L windows out
    assert sorted(nwin) == [1, 1] + [2] * 247 + [L + 2] * 8
    at = {b: (b if b < 10 else b + 1) for b in range(256)}                      # (read index of byte b: '\n' adds one)
    assert all(nwin[at[b]] == L + 2 for b in b"ACGTacgt")
    assert nwin[10] == nwin[11] == 1
    assert all(nwin[at[b]] == 2 for b in range(256) if b != 10 and b not in b"ACGTacgt")
    # the oracle reads the same bytes alike: the k-mer set, and the graph of K = L - 1
    for graph in (False, True):
        okeys, _, oreads, owin = oracle.count([(oracle.LINE, "reads", data)], L, 1 if graph else 0)
        assert set(okeys) == mm.object_keys(data, L - 1 if graph else L, graph)
        assert owin == info["windows"]
