"""The corpus of setops_edges.py held to what it claims, and the models of setops_model.py held to the oracle, without a
device: every case has exactly the tags its data shows and every condition occurs; the model's intersect / subtract /
annotate / graph-to-kmer-set give the oracle's file bytes (and the oracle's refusals are the model's); the composition
from weighted runs and a count window, which is what the device is given, gives the model's sets; the bitmap words are
the oracle's WordyBitVector; the text is the oracle's dump, cut anywhere; the restored dump is the graph.  Lint has no
oracle counterpart: the model is held to cases worked out by hand at K = 3."""
import struct

import pytest

import merge_model as mm
import oracle_lib as o
import setops_edges as se
import setops_model as sm


def test_every_case_has_exactly_its_tags_and_every_condition_occurs():
    seen = set()
    for name in se.NAMES:
        c = se.case(name)
        got = se.realised(c)
        assert got == set(c.tags), (name, "claimed only", sorted(set(c.tags) - got), "shown only", sorted(got - set(c.tags)))
        seen |= got
        n = max([len(getattr(c, f)) for f in ("keys", "edges") if hasattr(c, f)] + [len(r[0]) for r in getattr(c, "runs", [])]
                + [len(s) for s in getattr(c, "sets", [])])
        assert n <= 70000, name
    assert seen == set(se.CONDITIONS), (sorted(set(se.CONDITIONS) - seen), sorted(seen - set(se.CONDITIONS)))
    cuts = set()
    for name in se.RANGED:
        c = se.case(name)
        cuts |= se.cut_tags(len(c.keys if c.kind == "dumpk" else c.edges))
    assert cuts == set(se.RANGE_CONDITIONS), sorted(cuts ^ set(se.RANGE_CONDITIONS))


def test_a_planned_selection_keeps_the_planned_items():
    for name in se.names("select"):
        c = se.case(name)
        if not name.startswith("sel_"):
            continue
        (keys, counts), = c.runs
        n = len(keys)
        patterns = [t[len("S.keep="):] for t in c.tags if t.startswith("S.keep=")]
        assert patterns, name
        got_keys, got_counts = sm.select(keys, counts, *se.WINDOW)
        for p in patterns:
            assert got_keys == [keys[i] for i in range(n) if se.PATTERNS[p](i, n)], (name, p)
        assert set(got_counts) <= set(se.KEPT_COUNTS) and keys == sorted(set(keys)) and max(keys) < 1 << (2 * c.K), name


def test_merged_is_merge_models_merge_where_that_is_defined():
    for name in se.names("select"):
        c = se.case(name)
        keys, counts = sm.merged(c.runs)
        assert keys == sorted(keys) and all(0 <= v <= sm.U32 for v in counts), name
        runs = [list(zip(k, w if isinstance(w, list) else [w] * len(k))) for k, w in c.runs]
        if all(v >= 1 for r in runs for _, v in r):
            m = mm.merge(runs, mm.KMER)
            assert (m.keys, m.u32) == (keys, counts), name
    w = se.case("win_1_1")
    assert sm.select(*sm.merged(w.runs), 1, 1)[0] == sm.subtract(w.runs[0][0], w.runs[1][0])
    t = se.case("win_twice")
    k1, c1 = sm.select(*sm.merged(t.runs), *t.windows[0])
    k2, c2 = sm.select(k1, c1, *t.windows[1])
    assert 0 < len(k2) < len(k1) < len(sm.merged(t.runs)[0]) and set(c2) == {3}


def _model_files(c):
    """what the model says the command writes: {suffix: bytes}, stats"""
    if c.op == "intersect":
        r = sm.intersect(c.sets)
        return se.kmer_set_files(o, r, c.K), None
    if c.op == "subtract":
        return se.kmer_set_files(o, sm.subtract(*c.sets), c.K), None
    union, lw, rw, stats = sm.annotate(*c.sets)
    f = se.kmer_set_files(o, union, c.K)
    f[".lhs-bits"], f[".rhs-bits"] = sm.words_bytes(lw), sm.words_bytes(rw)
    return f, stats


def test_the_set_algebra_is_the_oracles_and_so_are_its_refusals():
    empty = 0
    for name in se.names("algebra"):
        c = se.case(name)
        exp, stats = se.algebra_expected(o, name)
        if isinstance(exp, Exception):
            with pytest.raises((sm.Undefined, sm.Refused)):
                _model_files(c)
            assert {"A.refused", "A.undefined"} & c.tags, name
            continue
        assert not {"A.refused", "A.undefined"} & c.tags, name
        got, gstats = _model_files(c)
        assert se.first_difference(got, exp) is None, (name, se.first_difference(got, exp))
        assert gstats == stats, name
        # ... and what the device is given -- weighted runs and one count window -- is the same set
        runs, window = sm.as_windows(c.op, c.sets)
        keys, counts = sm.merged(runs)
        if window:
            keys, counts = sm.select(keys, counts, *window)
        result = sm.intersect(c.sets) if c.op == "intersect" else sm.subtract(*c.sets) if c.op == "subtract" else sm.annotate(*c.sets)[0]
        assert keys == result, name
        if c.op == "annotate":
            assert (sm.count_bits(counts, 1), sm.count_bits(counts, 2)) == sm.annotate(*c.sets)[1:3], name
        empty += not result
    assert empty >= 3          # disjoint sets, a - a, the empty lhs: results that are then emitted


def test_wordy_bits_is_the_oracles_bit_vector():
    assert sm.wordy_bits([]) == [0] and sm.wordy_bits([True] * 64) == [sm.M64] and sm.wordy_bits([False] * 64 + [True]) == [0, 1]
    for name in se.names("bits"):
        c = se.case(name)
        m = len(c.keys)
        for mask in (1, 2, 3):
            flags = [(v & mask) != 0 for v in c.counts]
            words = sm.count_bits(c.counts, mask)
            assert len(words) == (m - 1) // 64 + 1 and (m % 64 == 0 or words[-1] >> (m % 64) == 0), (name, mask)
            ones = [i for i, f in enumerate(flags) if f]
            f = o.write_bits_sparse(ones, vname="x")          # (the oracle's builder stops at the word of the last one)
            got = list(struct.unpack("<%dQ" % (len(f["x"]) // 8), f["x"]))
            assert o.BitsReader(f, "x").words() == len(got), (name, mask)
            assert got == words[:len(got)] and not any(words[len(got):]), (name, mask)
        # a case without an item in neither set and with both sides taken is merge-and-annotate's own output
        if 4 not in c.counts and any(v & 1 for v in c.counts) and any(v & 2 for v in c.counts):
            a = [k for k, v in zip(c.keys, c.counts) if v & 1]
            b = [k for k, v in zip(c.keys, c.counts) if v & 2]
            files = dict(o.write_kmer_set(a, c.K, out="a"))
            files.update(o.write_kmer_set(b, c.K, out="b"))
            exp, stats = o.merge_and_annotate(files, "a", "b", "u")
            assert exp["u.lhs-bits"] == sm.words_bytes(sm.count_bits(c.counts, 1)), name
            assert exp["u.rhs-bits"] == sm.words_bytes(sm.count_bits(c.counts, 2)), name
            assert stats == (len(a), len(b), sum(1 for v in c.counts if v == 3)), name


def test_normal_edges_stated_twice_and_the_oracles_graph_to_kmer_set():
    kept_some = dropped_some = 0
    for name in se.names("g2k"):
        c = se.case(name)
        normal = sm.normal_edges(c.edges, c.K, o.normalize)
        assert normal == sm.normal_edges_by_pairs(c.edges, c.K), name
        present = set(c.edges)
        for e in c.edges:
            r = sm.revcomp(e, c.K + 1)
            assert r == o.revcomp(e, c.K + 1) and sm.fnv(e) == o.fnv(e)
            if r in present:
                assert (e in normal) + (r in normal) == 1 if r != e else e in normal, (name, e)
        exp = se.g2k_expected(o, name)
        got = se.kmer_set_files(o, normal, c.K + 1, M=len(c.edges))
        assert se.first_difference(got, exp) is None, (name, se.first_difference(got, exp))
        kept_some += 0 < len(normal)
        dropped_some += len(normal) < len(c.edges)
    assert kept_some and dropped_some
    asym = se.case("g2k_asymmetric_k31")
    lone = [e for e in asym.edges if sm.revcomp(e, 32) not in set(asym.edges)]
    normal = set(sm.normal_edges(asym.edges, 31, o.normalize))
    assert any(e in normal for e in lone) and any(e not in normal for e in lone)          # kept or dropped by normalize alone


def test_the_estimates_move_d():
    for name in se.names("estimate"):
        c = se.case(name)
        ds = set()
        for label, M in se.estimates(len(c.keys), c.other):
            assert M <= 64 * len(c.keys)
            ds.add(struct.unpack("<8Q", o.write_kmer_set(c.keys, c.K, M=M, out="ks")["ks.kmers.header"][:64])[1])
        assert len(ds) >= 3, (name, sorted(ds))


def test_the_text_is_the_oracles_dump_and_restores_to_the_graph():
    for name in se.names("dumpk"):
        c = se.case(name)
        text = sm.dump_text(c.keys, None, c.K, sm.KMERS)
        assert text == o.dump(o.write_kmer_set(c.keys, c.K, out="ks"), "ks", 0), name
    for name in se.names("dumpe"):
        c = se.case(name)
        files = o.write_graph(c.edges, c.counts, c.K, out="gr")
        text = sm.dump_text(c.edges, c.counts, c.K, sm.EDGES)
        assert text == o.dump(files, "gr", 1), name
        back = o.restore_graph(text, "gr")
        assert se.first_difference(back, files) is None, (name, se.first_difference(back, files))
    for name in se.RANGED:
        c = se.case(name)
        kind = sm.KMERS if c.kind == "dumpk" else sm.EDGES
        keys, counts = (c.keys, None) if kind == sm.KMERS else (c.edges, c.counts)
        whole = sm.dump_text(keys, counts, c.K, kind)
        cuts = se.range_cuts(len(keys))
        pieces = [sm.dump_piece(keys, counts, c.K, kind, 0, a, b - a) for a, b in zip(cuts, cuts[1:])]
        assert b"".join(pieces) == whole, name
        assert [p.startswith(b"#") for p in pieces] == [a == 0 for a in cuts[:-1]], name
        assert pieces[-1] == b"" and cuts[-2:] == [len(keys)] * 2, name


# ---- lint by hand, K = 3: edges of four bases, two bits each, A=0 C=1 G=2 T=3 -----------------------------------------------
# AAAC (1) <-> GTTT (191); AACC (5) <-> GGTT (175); ACGT (27) is its own reverse complement.

E = {s: o.kmer_value(s) for s in ("AAAC", "GTTT", "AACC", "GGTT", "ACGT")}
CLEAN = {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}


def _lint(pairs, asymmetric=False):
    return sm.lint([E[s] for s, _ in pairs], [c for _, c in pairs], 3, asymmetric)


def test_lint_by_hand_clean_and_self_complementary():
    assert [E[s] for s in ("AAAC", "AACC", "ACGT", "GGTT", "GTTT")] == [1, 5, 27, 175, 191]
    assert sm.revcomp(1, 4) == 191 and sm.revcomp(5, 4) == 175 and sm.revcomp(27, 4) == 27
    g = [("AAAC", 2), ("AACC", 3), ("ACGT", 9), ("GGTT", 3), ("GTTT", 2)]
    assert _lint(g) == (CLEAN, set()) and _lint(g, True) == (CLEAN, set())
    # the self-complementary edge with a zero count is its own partner: symmetric, zero but no mismatch; asymmetric, "both" are zero
    g[2] = ("ACGT", 0)
    assert _lint(g) == (dict(CLEAN, zero_count=1), {(2, 3, 2)})
    assert _lint(g, True) == (dict(CLEAN, count_mismatch=1), {(2, 2, 2)})


def test_lint_by_hand_missing_partner():
    g = [("AAAC", 2), ("AACC", 3), ("GGTT", 3)]                      # GTTT is gone: AAAC at index 0 has no partner
    for asym in (False, True):
        assert _lint(g, asym) == (dict(CLEAN, missing_rc=1), {(0, 1, sm.NONE)})
    g = [("AACC", 3), ("GGTT", 3), ("GTTT", 0)]                      # ... at the end, and a zero count is not looked at without a partner
    assert _lint(g) == (dict(CLEAN, missing_rc=1), {(2, 1, sm.NONE)})


def test_lint_by_hand_mismatch_and_zero():
    g = [("AAAC", 2), ("AACC", 3), ("GGTT", 4), ("GTTT", 2)]
    assert _lint(g) == (dict(CLEAN, count_mismatch=2), {(1, 2, 2), (2, 2, 1)})          # both partners
    assert _lint(g, True) == (CLEAN, set())                                            # an asymmetric graph may differ
    g = [("AAAC", 0), ("AACC", 3), ("GGTT", 3), ("GTTT", 0)]                            # zero on both strands
    assert _lint(g) == (dict(CLEAN, zero_count=2), {(0, 3, 3), (3, 3, 0)})
    assert _lint(g, True) == (dict(CLEAN, count_mismatch=2), {(0, 2, 3), (3, 2, 0)})
    g = [("AAAC", 0), ("AACC", 3), ("GGTT", 3), ("GTTT", 2)]                            # zero on one strand: kind 2 wins over kind 3
    assert _lint(g) == (dict(CLEAN, count_mismatch=2, zero_count=1), {(0, 2, 3), (3, 2, 0)})
    assert _lint(g, True) == (CLEAN, set())


def test_lint_by_hand_an_equal_neighbour():
    g = [("AAAC", 2), ("AAAC", 2), ("GTTT", 2)]                      # the second copy does not exceed the first; GTTT finds the first
    assert _lint(g) == (dict(CLEAN, order_violation=1), {(1, 4, 2)})
    g = [("AAAC", 2), ("AAAC", 5), ("GTTT", 2)]                      # kind 4 overwritten by 2
    assert _lint(g) == (dict(CLEAN, order_violation=1, count_mismatch=1), {(1, 2, 2)})
    g = [("AAAC", 2), ("AAAC", 2)]                                   # ... by 1
    assert _lint(g) == (dict(CLEAN, order_violation=1, missing_rc=2), {(0, 1, sm.NONE), (1, 1, sm.NONE)})
    g = [("AAAC", 0), ("AAAC", 0), ("GTTT", 0)]                      # kind 3 only where no other applies: the copy stays kind 4
    assert _lint(g) == (dict(CLEAN, order_violation=1, zero_count=3), {(0, 3, 2), (1, 4, 2), (2, 3, 0)})


def test_lint_over_the_corpus_totals_and_offenders_agree():
    for name in se.names("lint"):
        c = se.case(name)
        for asym in (False, True):
            tot, off = sm.lint(c.edges, c.counts, c.K, asym)
            assert len({i for i, _, _ in off}) == len(off), name          # an edge offends once
            assert sum(tot.values()) >= len(off), name
            assert all(o_ == sm.NONE or c.edges[o_] == sm.revcomp(c.edges[i], c.K + 1) for i, _, o_ in off), name
