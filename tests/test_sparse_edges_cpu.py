"""The corpus of sparse_edges.py against itself and against the oracle, without a GPU: every case really has the
conditions it is there for (by the model of DenseSelect::Builder that sparse_edges.ds_blocks restates from the rules
alone), the corpus as a whole has every condition of ALL_TAGS, and the oracle's files agree with the model -- header
statistics of both DenseSelect images, every block's type bits, every internal pointer of an intermediate block, D,
count, bitmap length, column files -- and its readers give every position and count back."""
import random
import struct

import pytest

import sparse_edges as se


@pytest.mark.parametrize("name", se.NAMES)
def test_case_has_its_conditions(oracle, name):
    c = se.case(name)
    assert c.tags, name
    tags, marks = se.realised(c)
    assert c.tags <= tags, sorted(c.tags - tags)
    assert c.D == oracle.lib().go_sparse_d(oracle.key(c.N), c.M)
    if c.kind == "bare" and c.tags & set(t for t in se.ALL_TAGS if t[0] in "AB"):
        assert marks[0] or marks[1]


def test_corpus_has_every_condition():
    assert len(set(se.ALL_TAGS)) == len(se.ALL_TAGS)
    claimed = set()
    for name in se.NAMES:
        claimed |= se.case(name).tags
    assert claimed == set(se.ALL_TAGS), (sorted(set(se.ALL_TAGS) - claimed), sorted(claimed - set(se.ALL_TAGS)))


def test_range_cuts_have_every_condition():
    """the cuts of the ranges path (test_gpu_sparse_edges.py): on 8 191 / 8 192 / 8 193, inside tagged blocks and
    sub-blocks, with a "-d0" block edge on the cut and beside it, an empty range between two full ones -- and tagged
    blocks built by a range's owner in one group, by the assembler in another"""
    seen = set()
    for name in se.RANGED:
        c = se.case(name)
        k, estimate = se.kmer_universe(c)
        assert 4 ** k >= c.N_end and se.sparse_d(4 ** k, estimate) == c.D
        groups = se.range_groups(c)
        assert len(groups) == 2
        for label, cuts in groups:
            assert cuts == sorted(cuts) and 0 < cuts[0] and cuts[-1] < c.m
            seen |= se.ranges_model(c, k, cuts)[2]
    assert seen == set(se.RANGE_TAGS), sorted(set(se.RANGE_TAGS) - seen)


def _check_dense_select(img, blocks, invert, name):
    h, types, offs = se.ds_parse(img)
    assert h[0] == 2012092701 and h[1] == invert and h[4:8] == (13, 8192, 6, 64), name
    assert h[8] == len(blocks) and h[9] == 16 * len(blocks), (name, h[8], len(blocks))
    assert tuple(h[10:16]) == se.ds_stats(blocks), (name, h[10:16], se.ds_stats(blocks))
    rank = struct.unpack("<%dQ" % h[8], img[h[3]:h[3] + 8 * h[8]])
    at = 4096
    for b, t, off, r in zip(blocks, types, offs, rank):
        assert t == se.FORM_BITS[b.form] and off == at and r == b.lo, (name, b, t, off, at)
        at += (b.bytes + 7) & ~7
        if b.form != "inter":
            continue
        ptrs = struct.unpack("<128H", img[off + 512:off + 768])
        base = 768
        for s in range(128):
            want = (base | se.SUB_BITS[b.subs[s]]) if b.subs[s] else 0
            assert ptrs[s] == want, (name, b, s, ptrs[s], want)
            base += se.SUB * b.subs[s] // 8
    assert h[2] == (at + 15) & ~15 and h[3] == h[2] + 8 * len(blocks) and len(img) == h[3] + 8 * len(blocks), name


@pytest.mark.parametrize("name", se.BARE)
def test_oracle_files_agree_with_the_model(oracle, name):
    c = se.case(name)
    files = se.expected(oracle, name)
    hdr = struct.unpack("<8Q", files[".header"])
    qD = 8 * ((c.D + 7) // 8)
    assert hdr[0] == 2012030501 and hdr[1] == c.D and hdr[2] == qD and hdr[7] == c.m
    assert hdr[3] | (hdr[4] << 64) == (1 << c.D) - 1 and hdr[5] | (hdr[6] << 64) == c.N_end
    assert len(files[".high-bits"]) == 8 * c.nwords
    cols = se.ia_columns(qD)
    assert sorted(files) == sorted([".header", ".high-bits", "-d0", "-d1"] + [".low-bits" + s for s, _, _ in cols])
    for suffix, nbytes, shift in cols:
        assert len(files[".low-bits" + suffix]) == c.m * nbytes
    # the bitmap itself, from the positions of the ones
    words = struct.unpack("<%dQ" % c.nwords, files[".high-bits"])
    ones = c.ones()
    assert sum(bin(w).count("1") for w in words) == c.m
    for p in (int(ones[0]), int(ones[-1]), int(ones[c.m // 2])):
        assert words[p >> 6] >> (p & 63) & 1
    _check_dense_select(files["-d1"], c.blocks(1), 0, name)
    _check_dense_select(files["-d0"], c.blocks(0), 1, name)


@pytest.mark.parametrize("name", se.GRAPHS)
def test_oracle_counts_agree_with_the_model(oracle, name):
    c = se.case(name)
    files = se.expected(oracle, name)
    cs = c.counts
    big = [(i, v) for i, v in enumerate(cs) if v > 255]
    big2 = [(j, v) for j, (i, v) in enumerate(big) if v > 65535]
    assert files["-counts.ord0"] == bytes(v & 255 for v in cs)
    assert files["-counts.ord1"] == bytes(v >> 8 & 255 for _, v in big)
    assert files["-counts.ord2"] == struct.pack("<%dH" % len(big2), *[v >> 16 for _, v in big2])
    assert struct.unpack("<8Q", files["-counts.ord1p.header"])[7] == len(big)
    assert struct.unpack("<8Q", files["-counts.ord2p.header"])[7] == len(big2)
    full = {"gr" + n: b for n, b in files.items()}
    rd1, rd2 = oracle.SparseReader(full, "gr-counts.ord1p"), oracle.SparseReader(full, "gr-counts.ord2p")
    assert [rd1.select(j) for j in range(len(big))] == [i for i, _ in big]
    assert [rd2.select(j) for j in range(len(big2))] == [j for j, _ in big2]


@pytest.mark.parametrize("name", se.NAMES)
def test_oracle_readers_return_the_case(oracle, name):
    """SparseReader.select of every position, vba_get of every count -- sampled, with every marked element and both
    ends among the sample, where a case has more than a few thousand"""
    c = se.case(name)
    full = {("gr" if c.kind == "graph" else "sa") + n: b for n, b in se.expected(oracle, name).items()}
    rd = oracle.SparseReader(full, "gr-edges" if c.kind == "graph" else "sa")
    assert rd.count() == c.m and rd.size() == c.N_end
    idx = range(c.m)
    if c.m > 4000:
        rng = random.Random(3)
        marks = se.realised(c)[1]
        idx = sorted(set(rng.sample(range(c.m), 2000)) | {0, c.m - 1} | {i for f, n in marks[1] for i in (f, f + n - 1)})
    for i in idx:
        assert rd.select(i) == c.keys[i], (name, i)
    if c.kind == "graph":
        for i in range(c.m):
            assert oracle.vba_get(full, "gr-counts", i) == c.counts[i], (name, i)


def test_oracle_refuses_a_high_part_of_two_to_the_64(oracle):
    positions, N, M, N_end = se.REFUSED
    D = se.sparse_d(N, M)
    assert positions[-1] < N and positions[-1] >> D == 1 << 64
    with pytest.raises(oracle.OracleError):
        oracle.write_sparse_array(positions, N, M, N_end=N_end)
