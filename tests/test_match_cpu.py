"""The model of match_reads and of extract-reads / filter-reads (match_model.py) against hand-worked cases, and the
generated inputs of the GPU tests against vacuity.  No GPU, no library."""
import pytest

import match_cases as mc
import match_model as mm
import oracle_lib as o


def kv(s):
    return o.kmer_value(s)


def test_entry_points_are_exported_and_check_their_arguments():
    import ctypes as C
    import gossamer_amd as g
    L = g.load()
    assert g.MATCH_SYMBOLS == ["goss_gpu_object_match_reads", "goss_gpu_object_match_reads_host"]
    for n in g.MATCH_SYMBOLS:
        assert hasattr(L, n), n
    assert (g.MATCH_NORMALIZE, g.MATCH_ANY) == (1, 4)
    for n in g.MATCH_SYMBOLS:
        f = getattr(L, n)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert f(None, None, 0, 0, 0, None, None, None, None) == -1          # no object


def test_reads_and_starts():
    assert mm.read_spans(b"") == []
    assert mm.read_spans(b"\n") == [(0, 0)]
    assert mm.read_spans(b"\n\n") == [(0, 0), (1, 1)]
    assert mm.read_spans(b"AC\n\nGT") == [(0, 2), (3, 3), (4, 6)]
    assert mm.read_spans(b"AC\nGT\n") == [(0, 2), (3, 5)]
    assert mm.read_starts(b"AC\n\nGT") == [0, 3, 4, 6]
    assert mm.read_starts(b"AC\nGT\n") == [0, 3, 5]          # past the last base: the final '\n' itself
    assert mm.read_starts(b"A\n\n") == [0, 2, 2]
    assert mm.read_starts(b"") == [0]
    # '\r' and NUL end no read; they end windows
    assert mm.read_spans(b"AC\rGT\x00A") == [(0, 7)]


def test_three_window_read_with_a_known_hit():
    # ACGTA, L = 3: ACG CGT GTA
    ws = mm.windows(b"ACGTA", 3)
    assert [(p, x) for p, x, _ in ws] == [(0, kv("ACG")), (1, kv("CGT")), (2, kv("GTA"))]
    assert kv("ACG") == 0b000110 and kv("GTA") == 0b101100
    w, h, s, info = mm.match(b"ACGTA\n", 3, {kv("CGT")})
    assert (w, h, s) == ([3], [1], [0, 5])
    assert info == {"reads": 1, "windows": 3, "hits": 1, "matched_reads": 1}
    # every window counts, repeats included
    w, h, _, _ = mm.match(b"AAAAA\nCC\n", 3, {kv("AAA")})
    assert (w, h) == ([3, 0], [3, 0])
    assert mm.match(b"AAAAA\nCC\n", 3, {kv("AAA")}, any=True)[1] == [1, 0]


def test_n_splits_and_case():
    # acgNtacg, L = 3: acg | tac acg
    ws = mm.windows(b"acgNtacg", 3)
    assert [(p, x) for p, x, _ in ws] == [(0, kv("ACG")), (4, kv("TAC")), (5, kv("ACG"))]
    assert mm.windows(b"ACNGT", 3) == []
    # a window never crosses a read
    w, _, _, info = mm.match(b"AC\nGT", 3, set())
    assert w == [0, 0] and info["reads"] == 2
    # reads of L - 1, L, L + 1
    assert mm.match(b"AC\nACG\nACGT\n", 3, set())[0] == [0, 1, 2]


def test_reverse_strand_needs_normalisation():
    L = 5
    x = kv("AACCG")
    assert mm.revcomp(x, L) == kv("CGGTT")
    assert [r for _, _, r in mm.windows(b"AACCG", L)] == [kv("CGGTT")]
    c = mm.canonical(x, L)
    assert c in (x, kv("CGGTT")) and c == o.normalize(x, L) and mm.fnv(x) == o.fnv(x)
    assert mm.canonical_many([(x, kv("CGGTT")), (kv("CGGTT"), x)]) == [c, c]
    other = kv("CGGTT") if c == x else x                  # the strand the set does not store
    text = o.kmer_string(other, L).encode() + b"\n"
    assert mm.match(text, L, {c})[1] == [0]
    assert mm.match(text, L, {c}, normalize=True)[1] == [1]
    # two-word keys
    L = 40
    s = "ACGTTGCAAGCTTAGCCGATATCGGATCCAGTTACGGATCA"[:L]
    x = kv(s)
    assert mm.revcomp(x, L) == kv(mm.rc_text(s)) == o.revcomp(x, L)
    assert mm.canonical(x, L) == o.normalize(x, L)
    assert [(a, b) for _, a, b in mm.windows(s.encode(), L)] == [(x, kv(mm.rc_text(s)))]


def test_object_keys():
    reads = b"ACGTAC\n"
    assert mm.object_keys(reads, 3, True) == {kv(s) for s in ("ACGT", "CGTA", "GTAC", "TACG")}
    assert mm.object_keys(reads, 3, False) == {o.normalize(kv(s), 3) for s in ("ACG", "CGT", "GTA", "TAC")}


def test_commands_model():
    assert mm.pair_files("a.b.fq") == ("a.b_1.fq", "a.b_2.fq")
    assert mm.pair_files("out/m.txt") == ("out/m_1.txt", "out/m_2.txt")
    reads = [b"ACGTA", b"TTTNTT", b"ggtac"]
    assert mm.parse_fasta(mm.as_fasta(reads, width=4)) == reads
    assert mm.parse_fastq(mm.as_fastq(reads)) == reads
    assert mm.parse_lines(b"AC\n\nGT") == [b"AC", b"", b"GT"]
    # item order: line files, then FASTA, then FASTQ, whatever the command line's order
    items = [("fastq", mm.as_fastq([b"ACGTA"])), ("fasta", mm.as_fasta([b"ggtac"])), ("line", b"TTACG\nCCCCC\n")]
    out, m, n = mm.extract_reads(items, 2, {kv("ACG"), kv("GTA")})
    assert (out, m, n) == (b"TTACG\nggtac\nACGTA\n", 3, 4)
    # filter-reads: either strand of a K-mer; CGT is the reverse strand of ACG
    c = o.normalize(kv("ACG"), 3)
    got = mm.filter_reads([("line", b"TTACG\nCCCCC\nACGTT\n")], 3, {c})
    assert got == {"m.txt": b"TTACG\nACGTT\n", "n.txt": b"CCCCC\n"}
    got = mm.filter_reads([("line", b"TTACG\nCCCCC\n"), ("line", b"GGGGG\nAAAAA\n")], 3, {c}, pairs=True)
    assert got == {"m_1.txt": b"TTACG\n", "m_2.txt": b"GGGGG\n", "n_1.txt": b"CCCCC\n", "n_2.txt": b"AAAAA\n"}
    with pytest.raises(ValueError):
        mm.filter_reads([("line", b"A\n")], 3, {c}, pairs=True)


@pytest.mark.parametrize("name", [c[0] for c in mc.CASES])
def test_generated_inputs_are_not_vacuous(name):
    K, graph, normalize, L, built, keys, query = mc.fixture(name)
    w, h, s, info = mc.expected(name, False)
    share = info["matched_reads"] / info["reads"]
    assert 0.2 <= share <= 0.8, share
    assert any(0 < b < a for a, b in zip(w, h))
    spans = mm.read_spans(query)
    lens = {e - b for b, e in spans}
    assert {0, L - 1, L, L + 1} <= lens and max(lens) >= 200000
    assert any(c in query for c in b"acgt") and b"N" in query and b"\n\n" in query
    assert (query[-1:] != b"\n") == (name in ("graph40", "kmers33n"))
    assert mc.expected(name, True)[1] == [1 if x else 0 for x in h]
    # the long read has windows in and out of the object
    r = max(range(len(spans)), key=lambda i: spans[i][1] - spans[i][0])
    assert 0 < h[r] < w[r]
