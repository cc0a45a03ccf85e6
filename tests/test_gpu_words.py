"""The words between the levels of the 32-bit-remainder form (gossamer_amd/csrc/goss_words.hpp): the first level of the
squeeze form stores the key's low word and a 10-bit field and no longer clears the high word above the key's bits, the
second level squeezes the remainder and writes its IMAGE (the counting kernel's mix, turned), the counting kernel
counts images and turns them back when it orders a segment.  Keys and counts against the oracle, on inputs made for the
bits and paths that changed."""
import os
import random

import pytest

import gossamer_amd as g
import words_model as wm

pytestmark = pytest.mark.gpu

SLOTS = (2048, 4096, 8192, 16384)
STATS = ("fused_chunks", "rem32_chunks", "narrow_chunks", "segment_retries", "rem32_bits", "rem32_split", "overflow_units")


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


def count_on_device(txt, k, mode, **e):
    with env(GOSS_GPU_FUSED_MIN=0, **e):
        with g.Context(k, mode, hbm_budget=4 << 30) as ctx:
            ctx.push_host(txt)
            c = ctx.finish()
            keys, counts = ctx.result()
            st = {n: ctx.stat(n) for n in STATS}
    return c.windows, keys, [int(x) for x in counts], st


def same_as_oracle(got, exp, what):
    nwin, keys, counts, st = got
    ek, ec, _, enwin = exp
    assert nwin == enwin, what
    assert len(keys) == len(ek), (what, len(keys), len(ek))
    assert keys == ek, what
    assert counts == ec, what


def rnd_bases(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


# ---- 2. k = 25 k-mer set: the bits around the squeeze and the junk above the key ----------------------------------

@pytest.fixture(scope="module")
def planted(oracle):
    """300 000 reads of 150 bp from a 1.5 Mbp genome with poly-A, poly-T, alternating and palindromic stretches planted
    (key bits 24, 25, 31, 32, 33 in every combination); reads whose bases before and behind a window are all T / all A
    (what the first level no longer clears above the key); an N directly behind a window."""
    rng = random.Random(2501)
    G = 1_500_000
    genome = list(rnd_bases(rng, G))
    stretches = ["A" * 70, "T" * 70, "AC" * 40, "GT" * 40, "AG" * 40, "CT" * 40, "AT" * 40, "CG" * 40]
    for _ in range(8):
        h = rnd_bases(rng, 45)
        stretches.append(h + revcomp(h))
    for rep in range(12):
        for s in stretches:
            p = rng.randrange(G - len(s))
            genome[p:p + len(s)] = s
    genome = "".join(genome)
    reads = []
    for _ in range(300_000 - 6_000):
        p = rng.randrange(G - 150)
        reads.append(genome[p:p + 150])
    for i in range(1_000):
        core = rnd_bases(rng, 26 + i % 40)
        pad = 150 - len(core)
        reads += [core + "T" * pad, core + "A" * pad, "T" * pad + core, "A" * pad + core]
        # an N directly behind a window: every offset of a thread's sixteen windows in turn
        r = rnd_bases(rng, 150)
        q = 25 + i % 125
        reads.append(r[:q] + "N" + r[q + 1:])
        q = i % 125
        reads.append(r[:q] + "N" + r[q + 1:q + 26] + "N" + r[q + 27:])
    rng.shuffle(reads)
    txt = ("\n".join(reads) + "\n").encode()
    return txt, oracle.count([(oracle.LINE, "r", txt)], 25, 0)


@pytest.mark.parametrize("slots", SLOTS)
def test_k25_against_the_oracle_in_every_table(planted, slots):
    txt, exp = planted
    got = count_on_device(txt, 25, 0, GOSS_GPU_REM32_SLOTS=slots)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["narrow_chunks"] == 1, st
    assert st["rem32_bits"] == 9 and st["rem32_split"] == 0 and st["segment_retries"] == 0, st
    same_as_oracle(got, exp, slots)


# ---- 3. sentinels: 25-mers whose stored word is a bucket's empty marker, 0, all ones ---------------------------------

@pytest.fixture(scope="module")
def sentinels(oracle):
    """25-mers between N's, each with a multiplicity of its own, all under one 17-bit prefix.  For the buckets b = 3, 300,
    509 (all sizes), 1 021 and 4 092 (the larger tables): the k-mers stored as the empty marker of b, of b ^ 1 and of
    b ^ 2 -- the first is at home in b ^ 1 and moves on to b ^ 2 -- and ten more that are at home in each of b, b ^ 1,
    b ^ 2 whatever the table's size, so that those buckets fill up and the chains walk over them; the k-mers stored as
    0 and as all ones."""
    rng = random.Random(77)
    prefix = 0x0B2D7
    words = [0, 0xFFFFFFFF]
    for b in (3, 300, 509, 1021, 4092):
        for bb in (b, b ^ 1, b ^ 2):
            words.append(wm.r32_image_marker(bb))
            for _ in range(10):
                # (home bb in every table: the twelve bits at bit 4; everything else random)
                words.append((rng.getrandbits(32) & ~(0xFFF << 4)) | (bb << 4))
    words = list(dict.fromkeys(words))
    for w in words[:5]:
        assert wm.r32_image(wm.r32_unimage(w)) == w
    pieces = []
    for i, w in enumerate(words):
        pieces += [wm.kmer25_with_word(w, prefix)] * (1 + i % 7)
    rng.shuffle(pieces)
    lines = ["N".join(pieces[i:i + 5]) for i in range(0, len(pieces), 5)]
    # (and reads of a random genome around them: a chunk of ordinary size, keys in the other segments)
    txt = ("\n".join(lines) + "\n").encode() + g.synth_reads_host(20_000, 100, 200_000, seed=78)
    return txt, oracle.count([(oracle.LINE, "r", txt)], 25, 0)


@pytest.mark.parametrize("slots", SLOTS)
def test_marker_words_are_counted_as_keys(sentinels, slots):
    txt, exp = sentinels
    got = count_on_device(txt, 25, 0, GOSS_GPU_REM32_SLOTS=slots)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["segment_retries"] == 0, st
    same_as_oracle(got, exp, slots)


# ---- 4. the paths that read the sub-regions again -----------------------------------------------------------------------

def test_table_ladder_recounts_from_the_same_sub_regions(oracle):
    """Eight segments of 5 000 distinct 25-mers each (one nine-base prefix per segment; base 12 an A or a G: the forward
    strand is the representative), thirty copies of every one (the fused path wants a million windows).  The estimate says one key per segment: the 2 048-slot
    tables are taken, overflow (limit 1 536), the counting alone is redone in 4 096 slots (limit 3 072), overflows again,
    and the 8 192-slot tables count -- three tables over the same stored words.  (GOSS_GPU_OVERFLOW_BY_SORT=0: eight
    overflowed segments would otherwise be counted by sort, below.)"""
    rng = random.Random(9)
    reads = []
    for _ in range(8):
        p9 = rnd_bases(rng, 9)
        tails = set()
        while len(tails) < 5000:
            t = rnd_bases(rng, 16)
            tails.add(t[:3] + rng.choice("AG") + t[4:])
        reads += [p9 + t for t in tails] * 30
    rng.shuffle(reads)
    txt = ("\n".join(reads) + "\n").encode()
    exp = oracle.count([(oracle.LINE, "r", txt)], 25, 0)
    got = count_on_device(txt, 25, 0, GOSS_GPU_OVERFLOW_BY_SORT=0, GOSS_GPU_EST_SCALE=0.05)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["rem32_split"] == 0 and st["segment_retries"] == 2, st
    assert st["overflow_units"] == 0, st
    same_as_oracle(got, exp, "ladder")


def test_overflow_by_sort_reads_images(oracle):
    """200 000 reads of a 1.5 Mbp genome, a sixth of them with a run of 30 T's written over their bases: every window that
    begins with nine T's lies in one 17-bit segment (hundreds of thousands of distinct keys): its table overflows, the
    segment is expanded from its sub-region into full keys and counted by sort; the chunk keeps its form."""
    import numpy as np
    rng = np.random.default_rng(31)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1_500_000)]
    starts = rng.integers(0, genome.size - 150, size=200_000)
    rows = np.empty((200_000, 151), dtype=np.uint8)
    rows[:, :150] = genome[starts[:, None] + np.arange(150)[None, :]]
    rows[:, 150] = ord("\n")
    at = 40 + np.arange(0, 200_000, 6) % 41                      # where the run starts, read by read
    cols = np.arange(151)[None, :]
    rows[::6][(cols >= at[:, None]) & (cols < at[:, None] + 30)] = ord("T")
    txt = rows.tobytes()
    exp = oracle.count([(oracle.LINE, "r", txt)], 25, 0)
    got = count_on_device(txt, 25, 0)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["rem32_split"] == 0 and st["segment_retries"] == 0, st
    assert st["overflow_units"] >= 1, st
    same_as_oracle(got, exp, "by sort")


@pytest.fixture(scope="module")
def plain_reads(oracle):
    txt = g.synth_reads_host(100_000, 150, 500_000, seed=4242)
    return txt, oracle.count([(oracle.LINE, "r", txt)], 25, 0), oracle.count([(oracle.LINE, "r", txt)], 25, 1)


@pytest.mark.parametrize("e,want", [({"GOSS_GPU_REM32_SPLIT": 2}, {"rem32_bits": 9, "rem32_split": 2, "narrow_chunks": 1}),
                                    ({"GOSS_GPU_REM32_BITS": 10}, {"rem32_bits": 10, "rem32_split": 0, "narrow_chunks": 1}),
                                    ({"GOSS_GPU_NARROW": 0}, {"rem32_bits": 9, "rem32_split": 0, "narrow_chunks": 0})],
                         ids=["split2-plain-remainders", "ten-bits-no-squeeze", "eight-byte-second-level"])
def test_other_forms_of_k25(plain_reads, e, want):
    txt, exp, _ = plain_reads
    got = count_on_device(txt, 25, 0, **e)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["segment_retries"] == 0, st
    assert {n: st[n] for n in want} == want, st
    same_as_oracle(got, exp, e)


@pytest.mark.parametrize("e,bits", [({}, 9), ({"GOSS_GPU_NO_GRAPH_REP": 1}, 10)], ids=["representatives", "both-strands"])
def test_graph_k24(plain_reads, e, bits):
    """build-graph k = 24, 25-mers.  By default a graph chunk is counted as ONE strand representative per window, i.e. as
    a k-mer-set chunk of 25-mers in representative space (fused_path.hpp: rep_graph; graph_mode is then false and the
    form is the squeezed one with nine bits), and expanded into both strands afterwards.  GOSS_GPU_NO_GRAPH_REP=1: both
    strands of every window through the first level (MODE 1), 33 bits and no bit to squeeze: ten second-level bits,
    narrow chunks, images."""
    txt, _, exp = plain_reads
    got = count_on_device(txt, 24, 1, **e)
    st = got[3]
    assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["rem32_split"] == 0 and st["segment_retries"] == 0, st
    assert st["rem32_bits"] == bits and st["narrow_chunks"] == 1, st
    same_as_oracle(got, exp, "graph k = 24")
