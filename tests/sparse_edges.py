"""The corpus that holds the on-disk array writers (kernels_emit.hpp: the Elias-Fano split of a SparseArray, the two
DenseSelect images over its high-bits bitmap, the VariableByteArray of the counts) to the oracle at every integer
threshold that decides a byte of the files.  Plain Python and numpy: no GPU, and the oracle only where a test hands it
to expected().  At the end: the same cases as k-mer sets cut into ranges (range_groups, ranges_model).

A case is built from the BITMAP it is meant to produce.  The i-th one of a SparseArray's high-bits bitmap sits at
h_i = (key_i >> D) + i; "-d1" indexes the ones (count m), "-d0" the zeros (count nd + 2, nd = N_end >> D).  From a strictly
increasing list of h_i and a D, from_ones() makes keys ((h_i - i) << D) | (number of earlier keys with the same high
part), and N, M, N_end for which sparse_d() -- SparseArray::Builder::d restated, asserted for every case -- yields
that D.  At most 2^D keys share a high part, so a run of ones is at most 2^D long: the cases that control the zeros
use D = 12.

ds_blocks() is the model: from the indexed positions of one sense alone it gives every block's form and byte size and,
for an intermediate block, the form of every sub-block -- DenseSelect::Builder::flush's rules as DESIGN.md states
them (block of 8 192: last - first >= 2^24 or a partial block -> 32-bit offsets, 64-bit positions from 2^32;
>= 2^16 -> intermediate; else small.  Sub-block of 64 with r = last - first: r <= 128 nothing stored, < 256 8-bit,
< 65 536 16-bit, else 32-bit).  realised() turns a case's models into the set of condition tags the case really
has; a case's own `tags` must be among them, and ALL_TAGS must be the union over the corpus (test_sparse_edges_cpu.py).

Left out on purpose, not shrunk into something that no longer takes the branch:
  * the 64-bit large block (last - first >= 2^32 inside one block): a 512 MB bitmap, and 2^32 zeros in "-d0";
  * the 2^24 threshold in "-d0": 8 192 zeros spread over 2^24 positions are 1.7 * 10^7 ones, that many keys.
A high part of 2^64 - 1 beside one of 2^64: sparse_d allows both (D = 10 for N = 1.25 * 2^74 with M = 2^64 - 1), but a
high part h puts h zeros in front of its one -- the accepted side would be a bitmap of 2^64 bits.  Only the refused
side is a case (REFUSED: the writer must answer GOSS_ERR_TOO_LARGE where the oracle refuses too).
"""
import bisect
import functools
import math
import random

import numpy as np

LOG2E = 1.4426950408889634
MASK64 = (1 << 64) - 1
BLOCK, SUB = 8192, 64
EF_CHUNK, EF_WORDS, EF_SWITCH = 2048, 1024, 65536          # keys per workgroup of the window kernel, its window, where it takes over


# ---- SparseArray::Builder::d, IntegerArray::builder's columns -------------------------------------------------------

def sparse_d_raw(N, M):
    n = float(N >> 64) * 18446744073709551616.0 + float(N & MASK64)
    d0 = math.log2(n / ((1.0 + float(M)) * LOG2E))
    assert d0 > 0, "the reference converts a negative double to unsigned here"
    return int(math.ceil(d0))


def sparse_d(N, M):
    return min(128, max(8, sparse_d_raw(N, M)))


def find_m(N, D):
    """an M with sparse_d(N, M) == D, unclamped"""
    target = N / ((1 << D) * LOG2E)
    c = int(target)
    for M in range(max(0, c - 2), c + 4):
        if sparse_d_raw(N, M) == D:
            return M
    raise AssertionError("no M gives D = %d for N = %d" % (D, N))


_SPLIT = {24: (8, 16), 40: (8, 32), 48: (16, 32), 56: (8, 48), 72: (8, 64), 80: (16, 64), 88: (8, 80), 96: (32, 64),
          104: (8, 96), 112: (16, 96), 120: (24, 96), 128: (64, 64)}


def ia_columns(bits, prefix="", shift=0):
    """[(file suffix, bytes, shift)] of an IntegerArray of `bits` bits"""
    if bits in (8, 16, 32, 64):
        return [(prefix, bits // 8, shift)]
    ub, lb = _SPLIT[bits]
    return ia_columns(ub, prefix + ".upr", shift + lb) + ia_columns(lb, prefix + ".lwr", shift)


# ---- the model of DenseSelect::Builder ------------------------------------------------------------------------------

class Block:
    __slots__ = ("first", "cnt", "lo", "span", "form", "bytes", "subs", "r")

    def __repr__(self):
        return "Block(first=%d cnt=%d span=%d %s %d B)" % (self.first, self.cnt, self.span, self.form, self.bytes)


def ds_blocks(P):
    """P: the indexed positions of one sense, ascending (numpy int64).  form: small / inter / large32 / large64;
    bytes: the block's body as the header statistics count it; subs: bits per stored offset of every sub-block
    (0 = none stored), r: their ranges."""
    out = []
    for first in range(0, len(P), BLOCK):
        blk = P[first:first + BLOCK]
        b = Block()
        b.first, b.cnt, b.lo, b.span, b.subs, b.r = first, len(blk), int(blk[0]), int(blk[-1]) - int(blk[0]), None, None
        if b.span >= 1 << 24 or b.cnt < BLOCK:
            b.form, b.bytes = ("large32", 4 * b.cnt) if b.span < 1 << 32 else ("large64", 8 * b.cnt)
        elif b.span >= 1 << 16:
            b.r = (blk[SUB - 1::SUB] - blk[0::SUB]).tolist()
            b.subs = [0 if r <= 128 else 8 if r < 256 else 16 if r < 65536 else 32 for r in b.r]
            b.form, b.bytes = "inter", 128 * 6 + sum(SUB * s // 8 for s in b.subs)
        else:
            b.form, b.bytes = "small", 256
        out.append(b)
    return out


def ds_stats(blocks):
    """(smallBlocks, smallBlocksSize, intermediateBlocks, intermediateBlocksSize, largeBlocks, largeBlocksSize)"""
    s = [0] * 6
    for b in blocks:
        i = {"small": 0, "inter": 2}.get(b.form, 4)
        s[i] += 1
        s[i + 1] += b.bytes
    return tuple(s)


# ---- cases -----------------------------------------------------------------------------------------------------------

class Case:
    """keys (python ints, ascending), N and M for the builder, N_end for its end(); tags the case is there for.
    kind "bare": a SparseArray; "graph": edges of K = 27 with `counts`."""

    def __init__(self, name, keys, N, M, N_end, tags, kind="bare", counts=None):
        self.name, self.keys, self.N, self.M, self.N_end, self.tags = name, keys, N, M, N_end, frozenset(tags)
        self.kind, self.counts = kind, counts
        self.D = sparse_d(N, M)
        self.m = len(keys)
        self.nd = 0 if self.D >= 128 else N_end >> self.D
        self.words = 2 if max(N, N_end) > 1 << 62 else 1
        self.nwords = (self.nd + self.m + 3) // 64 + 1
        assert all(a < b for a, b in zip(keys, keys[1:])) and (not keys or keys[-1] < N_end <= N), name

    def high(self, i):
        return 0 if self.D >= 128 else self.keys[i] >> self.D

    @functools.lru_cache(maxsize=None)
    def ones(self):
        return np.array([self.high(i) + i for i in range(self.m)], dtype=np.int64)

    def zeros(self):
        bits = np.ones(self.nd + self.m + 2, dtype=bool)
        bits[self.ones()] = False
        z = np.flatnonzero(bits)
        assert len(z) == self.nd + 2
        return z

    @functools.lru_cache(maxsize=None)
    def blocks(self, sense):
        return ds_blocks(self.ones() if sense else self.zeros())


def from_ones(name, h, D, tags, tail=3, clamp=False, pick_tail=None):
    """The SparseArray whose bitmap has its ones at h (ascending numpy int64) and `tail` >= 3 zeros behind the last one."""
    h = np.asarray(h, dtype=np.int64)
    m = len(h)
    idx = np.arange(m, dtype=np.int64)
    assert (np.diff(h) > 0).all() and h[0] >= 0, name
    hi = h - idx
    start = np.ones(m, dtype=bool)
    start[1:] = hi[1:] != hi[:-1]
    low = idx - np.maximum.accumulate(np.where(start, idx, 0))
    assert int(low.max()) < 1 << D, (name, "a run of %d ones needs a larger D" % (int(low.max()) + 1))
    keys = ((hi << D) | low).tolist()
    if pick_tail is not None:          # the first tail for which the bitmap ends as the case wants it
        tail = next(t for t in range(3, 3 + 128) if pick_tail(int(hi[-1]) + t - 2, m, int(h[-1])))
    nd = int(hi[-1]) + tail - 2
    N = nd << D
    M = N // 2 if clamp else find_m(N, D)
    c = Case(name, keys, N, M, N, tags)
    assert c.D == D and c.nd == nd and (c.ones() == h).all(), name
    return c


def from_zeros(name, z, D, tags):
    """... whose bitmap has its zeros at z (ascending, from 0) and three more behind them; every other position is a one."""
    z = np.asarray(z, dtype=np.int64)
    assert z[0] == 0
    z = np.concatenate([z, z[-1] + 1 + np.arange(3)])
    bits = np.ones(int(z[-1]) + 1, dtype=bool)
    bits[z] = False
    h = np.flatnonzero(bits)
    c = from_ones(name, h, D, tags, tail=len(bits) - 1 - int(h[-1]))
    assert c.nd + 2 == len(z)
    return c


def spread(n, span):
    """n offsets 0 .. span, strictly ascending, evenly spread"""
    assert span >= n - 1
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    return (np.arange(n, dtype=np.int64) * span) // (n - 1)


def chain(pieces, gap=2):
    """pieces of offsets laid behind one another, `gap` positions from the last of one to the first of the next"""
    out, at = [], 0
    for p in pieces:
        out.append(p + at)
        at += int(p[-1]) + gap
    return np.concatenate(out)


SMALL = 20000          # the span of a block that is there to be small (2.4 positions per element)
SMALL_Z = 9000         # ... of zeros: what lies between zeros are ones, and every one is a key


def _blocks(spans, partial=0):
    return chain([spread(BLOCK, s) for s in spans] + ([spread(partial, 3 * partial)] if partial else []))


def _subs(rs, gap):
    """a block of 128 sub-blocks of 64 with the given ranges"""
    assert len(rs) == 128
    return chain([spread(SUB, r) for r in rs], gap)


# ---- A and B: DenseSelect block and sub-block forms --------------------------------------------------------------------

def _case_d1_subblocks():
    mixed = [63, 128, 129, 255, 256, 65535, 65536] + [100, 200, 300] * 40 + [63]
    blocks = [spread(BLOCK, SMALL), _subs(mixed, 5),
              _subs([65536] * 128, 2),                              # every sub-block 32-bit: 33 536 bytes
              spread(BLOCK, SMALL),
              _subs([200] * 128, 400),                              # every sub-block 8-bit
              _subs([100] * 128, 600),                              # none stored: 768 bytes, the span made by the gaps
              _subs([300] + [100] * 127, 600), _subs([100] * 127 + [300], 600),
              _subs([100, 200, 1000, 70000] * 32, 7),               # the four forms in turn: every base another sum
              spread(77, 300)]
    tags = ["B.d1.r=%d" % r for r in (63, 128, 129, 255, 256, 65535, 65536)]
    tags += ["B.all-32bit", "B.all-8bit", "B.none-stored", "B.only-sub0", "B.only-sub127", "B.cycle"]
    return from_ones("d1_subblocks", chain(blocks), 8, tags)


def _case_d0_subblocks(big):
    # one block of zeros; the ones fill what lies between them (a sub-block of range 65 536: runs of 1 040 ones)
    rs = [128, 129, 255, 256, big] + [63] * 123
    z = chain([spread(BLOCK, SMALL_Z), _subs(rs, 2), spread(BLOCK, SMALL_Z), spread(500, 1500)])
    return from_zeros("d0_subblocks_%d" % big, z, 12, ["B.d0.r=%d" % r for r in (128, 129, 255, 256, big)])


def _ab_cases():
    T24 = 1 << 24
    yield "d1_span_65535_between", lambda: from_ones("d1_span_65535_between", _blocks([SMALL, 65535, SMALL]), 8,
                                                     ["A.d1.span=65535", "A.threshold-between-small"])
    yield "d1_span_65536_first", lambda: from_ones("d1_span_65536_first", _blocks([65536, SMALL, SMALL], 1), 8,
                                                   ["A.d1.span=65536", "A.threshold-first"])
    yield "d1_span_2p24m1_last", lambda: from_ones("d1_span_2p24m1_last", _blocks([SMALL, SMALL, T24 - 1]), 8,
                                                   ["A.d1.span=2^24-1", "A.threshold-last-full"])
    yield "d1_span_2p24_between", lambda: from_ones("d1_span_2p24_between", _blocks([SMALL, T24, SMALL], 100), 8,
                                                    ["A.d1.span=2^24", "A.threshold-between-small"])
    for s in (65535, 65536):
        yield "d0_span_%d" % s, (lambda s=s: from_zeros("d0_span_%d" % s, _blocks([SMALL_Z, s, SMALL_Z], 40), 12, ["A.d0.span=%d" % s]))
    for n in (1, 8191, 8192, 8193, 16384):
        yield "count_%d" % n, (lambda n=n: from_ones("count_%d" % n, spread(n, 3 * n), 8, ["A.count=%d" % n]))
    yield "d1_subblocks", _case_d1_subblocks
    for big in (65535, 65536):
        yield "d0_subblocks_%d" % big, (lambda big=big: _case_d0_subblocks(big))


# ---- C: the bitmap, from 65 536 keys on built by an LDS window per 2 048 keys -------------------------------------------

def _bitmap(m, tail_mod=None):
    """m ones in chunks of 2 048 (the window kernel's workgroups), the first 32 chunks holding every situation of a
    window: the chunk's last key in the window's last word and in the first word behind it, more than half of a chunk
    behind the window, a bit behind the window in the word of the next chunk's first key, two dense chunks that meet
    in the middle of a word."""
    dense = spread(EF_CHUNK, 76 * 64 + 52)                              # ends at bit 52 of its last word

    def ends_at(word, bit):                                            # dense, but the last key far away
        return np.concatenate([spread(EF_CHUNK - 1, 4900), [word * 64 + bit]])
    half = np.concatenate([spread(900, 2200), 70000 + 100 * np.arange(EF_CHUNK - 900)])
    plan = [("align", dense), ("join", dense), ("align", ends_at(EF_WORDS - 1, 5)), ("align", ends_at(EF_WORDS, 5)),
            ("align", half), ("align", ends_at(1280, 10)), ("follow", dense), ("align", dense)]
    out, last, left, i = [], -64, m, 0
    while left:
        how, p = plan[i % len(plan)]
        p = p[:left]
        at = {"align": (last + 2 + 63) // 64 * 64, "join": last + 2, "follow": last + 3}[how]
        out.append(p + at)
        last = at + int(p[-1])
        left -= len(p)
        i += 1
    h = np.concatenate(out).astype(np.int64)
    if tail_mod is None:
        return h, (lambda nd, m, last: last // 64 == (nd + m + 3) // 64)          # the last one in the bitmap's last word
    return h, (lambda nd, m, last: (nd + m + 3) % 64 == tail_mod)


_C_CHUNK_TAGS = ["C.last-key-at-w0+1023", "C.last-key-at-w0+1024", "C.more-than-half-outside", "C.outside-bit-in-next-chunks-first-word",
                 "C.dense-boundary-mid-word"]


def _c_cases():
    def make(name, m, tags, tail_mod=None):
        def f():
            h, pick = _bitmap(m, tail_mod)
            return from_ones(name, h, 8, tags, pick_tail=pick)
        return name, f
    yield make("bitmap_65535", 65535, ["C.m=65535"])
    yield make("bitmap_65536", 65536, ["C.m=65536", "C.last-one-in-last-word"] + _C_CHUNK_TAGS)
    yield make("bitmap_65537", 65537, ["C.m=65537", "C.tail%64=0"] + _C_CHUNK_TAGS, 0)
    yield make("bitmap_67583", 67583, ["C.m=67583", "C.tail%64=63"] + _C_CHUNK_TAGS, 63)
    yield make("bitmap_67584", 67584, ["C.m=67584"] + _C_CHUNK_TAGS)


# ---- D: every D that changes a branch of the split, every column layout ----------------------------------------------

D_VALUES = sorted(set(range(8, 129, 8)) | set(range(9, 129, 8)) | {63, 127})
_D_EACH = ["D.low=ones", "D.low=zeros", "D.high=0", "D.high=max"]


def _d_case(D, clamp=False, name=None):
    """A few hundred keys of a universe 2^(D + 12) (as far as 128 bits go: 2^128 - 1): low D bits all ones and all zeros,
    the high part 0 and the largest the universe has."""
    name = name or "D_%d" % D
    rng = random.Random(1000 + D)
    N = min(1 << (D + 12), (1 << 128) - 1)
    top = (N - 1) >> D if D < 128 else 0
    ones = (1 << D) - 1
    keys = {0, 1, ones, ones - 1, min(N - 1, (top << D) | ones)}
    if top:
        keys |= {top << D, (top << D) | 1, (1 << D) | ones, 1 << D}
    for _ in range(500):
        hp = rng.choice([0, top, rng.randint(0, top), rng.randint(0, top)])
        low = rng.choice([0, ones, rng.getrandbits(D), rng.getrandbits(D), 1 << (D - 1), (1 << (D - 1)) - 1, (1 << 64) - 1 & ones,
                          (1 << min(D, 64)) % (ones + 1)])
        keys.add(min(N - 1, (hp << D) | low))
    keys = {k for k in keys if k < N}
    M = N // 2 if clamp else find_m(N, D)
    tags = [t for t in _D_EACH if D < 128 or t != "D.low=ones"]          # (2^128 - 1 is the largest universe: no key of it is all ones)
    if clamp:
        tags.append("D.clamped8")
    else:
        tags.append("D.D=%d" % D)
        if D == 8:
            tags.append("D.unclamped8")
    if N > 1 << 62:
        tags.append("D.two-word.D<64" if D < 64 else "D.two-word.D=64" if D == 64 else "D.two-word.D>64")
    c = Case(name, sorted(keys), N, M, N, tags)
    assert c.D == D, (name, c.D)
    return c


def _d_cases():
    for D in D_VALUES:
        yield "D_%d" % D, (lambda D=D: _d_case(D))
    yield "D_8_clamped", lambda: _d_case(8, clamp=True, name="D_8_clamped")


# A high part of 2^64: (positions, N, M, N_end) the writer must refuse, as the oracle does
REFUSED = ([5, 1 << 74], (1 << 74) + (1 << 72), (1 << 64) - 1, 1 << 30)


# ---- E: the counts -------------------------------------------------------------------------------------------------

K_GRAPH = 27
SPECIAL = [1, 255, 256, 257, 65535, 65536, 65537, 1 << 24, (1 << 32) - 1]
SPECIAL_BIG = [v for v in SPECIAL if v > 255]


def _edges(n, seed):
    rng = random.Random(seed)
    e = set()
    while len(e) < n:
        e.add(rng.getrandbits(2 * K_GRAPH + 2))
    return sorted(e)


def _graph(name, counts, tags, seed):
    keys = _edges(len(counts), seed)
    N = 1 << (2 * K_GRAPH + 2)
    return Case(name, keys, N, len(keys), N, tags, kind="graph", counts=counts)


def _counts_case(j):
    """3 000 edges: a special count at the first edge, at the last, and at entries 255, 256, 257 of the list of counts
    above 255 (every seventh edge of the background is one, every 35th above 65 535)"""
    rng = random.Random(500 + j)
    n = 3000
    counts = [rng.randint(1, 255) for _ in range(n)]
    for i in range(3, n, 7):
        counts[i] = rng.randint(65536, (1 << 32) - 1) if i % 5 == 0 else rng.randint(256, 65535)
    first, last = SPECIAL[j], SPECIAL[(j + 4) % 9]
    counts[0], counts[-1] = first, last
    big = [i for i, c in enumerate(counts) if c > 255]
    tags = ["E.%d@first" % first, "E.%d@last" % last]
    for s, slot in enumerate((255, 256, 257)):
        v = SPECIAL_BIG[(j + s) % 7]
        counts[big[slot]] = v
        tags.append("E.%d@big%d" % (v, slot))
    return _graph("counts_%d" % j, counts, tags, 600 + j)


def _e_cases():
    for j in range(9):
        yield "counts_%d" % j, (lambda j=j: _counts_case(j))
    def drawn(name, values, tag, seed):
        def f():
            rng = random.Random(seed)
            return _graph(name, [rng.choice(values) for _ in range(2000)], [tag], seed)
        return name, f
    yield drawn("counts_none_above_255", [1, 2, 254, 255], "E.ord1p-empty", 701)
    yield drawn("counts_none_above_65535", [1, 255, 256, 257, 40000, 65535], "E.ord2p-empty", 702)
    # (2^32 - 1 stands for "2^32 - 1 or more", which a context keeps for 256 keys at the most: 2^32 - 2 here)
    yield drawn("counts_all_above_65535", [65536, 65537, 1 << 24, (1 << 32) - 2, 1 << 31], "E.all-above-65535", 703)
    yield "counts_single_edge", lambda: _graph("counts_single_edge", [65536], ["E.single-edge"], 704)


# ---- the corpus ------------------------------------------------------------------------------------------------------

_BUILDERS = dict(list(_ab_cases()) + list(_c_cases()) + list(_d_cases()) + list(_e_cases()))
NAMES = list(_BUILDERS)
BARE = [n for n in NAMES if not n.startswith("counts_")]
GRAPHS = [n for n in NAMES if n.startswith("counts_")]
RANGED = [n for n in NAMES if n.startswith(("d1_", "d0_", "bitmap_"))]          # the A, B and C cases that go through ranges as k-mer sets


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    assert c.name == name
    return c


ALL_TAGS = (["A.d1.span=65535", "A.d1.span=65536", "A.d1.span=2^24-1", "A.d1.span=2^24", "A.d0.span=65535", "A.d0.span=65536"]
            + ["A.count=%d" % n for n in (1, 8191, 8192, 8193, 16384)]
            + ["A.threshold-first", "A.threshold-last-full", "A.threshold-between-small"]
            + ["B.d1.r=%d" % r for r in (63, 128, 129, 255, 256, 65535, 65536)]
            + ["B.d0.r=%d" % r for r in (128, 129, 255, 256, 65535, 65536)]
            + ["B.all-32bit", "B.all-8bit", "B.none-stored", "B.only-sub0", "B.only-sub127", "B.cycle"]
            + ["C.m=%d" % m for m in (65535, 65536, 65537, 67583, 67584)] + _C_CHUNK_TAGS
            + ["C.last-one-in-last-word", "C.tail%64=0", "C.tail%64=63"]
            + ["D.D=%d" % D for D in D_VALUES] + ["D.clamped8", "D.unclamped8"] + _D_EACH
            + ["D.two-word.D<64", "D.two-word.D=64", "D.two-word.D>64"]
            + ["E.%d@%s" % (v, p) for v in SPECIAL for p in ("first", "last")]
            + ["E.%d@big%d" % (v, s) for v in SPECIAL_BIG for s in (255, 256, 257)]
            + ["E.ord1p-empty", "E.ord2p-empty", "E.all-above-65535", "E.single-edge"])

THRESHOLD_SPANS = {65535: "65535", 65536: "65536", (1 << 24) - 1: "2^24-1", 1 << 24: "2^24"}
_FORM_OF_SPAN = {65535: "small", 65536: "inter", (1 << 24) - 1: "inter", 1 << 24: "large32"}
_SUB_OF_R = {63: 0, 128: 0, 129: 8, 255: 8, 256: 16, 65535: 16, 65536: 32}


def realised(c):
    """(the condition tags the case has, by its models; marks = {sense: (first index, length) of every
    block and sub-block that gave a tag})"""
    tags, marks = set(), {0: set(), 1: set()}
    if c.kind == "graph":
        cs = c.counts
        big = [v for v in cs if v > 255]
        for v in SPECIAL:
            if cs[0] == v:
                tags.add("E.%d@first" % v)
            if cs[-1] == v:
                tags.add("E.%d@last" % v)
            for slot in (255, 256, 257):
                if v > 255 and len(big) > slot and big[slot] == v:
                    tags.add("E.%d@big%d" % (v, slot))
        if not big:
            tags.add("E.ord1p-empty")
        elif max(cs) <= 65535:
            tags.add("E.ord2p-empty")
        if min(cs) > 65535:
            tags.add("E.all-above-65535")
        if len(cs) == 1:
            tags.add("E.single-edge")
        return tags, marks

    def mark(sense, first, n):
        marks[sense].add((first, n))

    for sense in (1, 0):
        bl = c.blocks(sense)
        full = [b for b in bl if b.cnt == BLOCK]
        for i, b in enumerate(full):
            if b.span in THRESHOLD_SPANS and (sense or b.span < 1 << 24):
                assert b.form == _FORM_OF_SPAN[b.span]
                tags.add("A.d%d.span=%s" % (sense, THRESHOLD_SPANS[b.span]))
                mark(sense, b.first, b.cnt)
                if i == 0:
                    tags.add("A.threshold-first")
                if i == len(full) - 1 and len(full) > 1:
                    tags.add("A.threshold-last-full")
                if 0 < i < len(full) - 1 and full[i - 1].form == "small" and full[i + 1].form == "small":
                    tags.add("A.threshold-between-small")
            if b.form != "inter":
                continue
            for s, r in enumerate(b.r):
                if r in _SUB_OF_R and (sense or r != 63):
                    assert b.subs[s] == _SUB_OF_R[r]
                    tags.add("B.d%d.r=%d" % (sense, r))
                    mark(sense, b.first + SUB * s, SUB)
            if sense:
                stored = [s for s in range(128) if b.subs[s]]
                what = ("B.all-32bit" if b.subs == [32] * 128 and b.bytes == 33536 and 1 << 23 <= b.span else
                        "B.all-8bit" if b.subs == [8] * 128 else
                        "B.none-stored" if not stored and b.bytes == 768 else
                        "B.only-sub0" if stored == [0] else "B.only-sub127" if stored == [127] else
                        "B.cycle" if b.subs == [0, 8, 16, 32] * 32 else None)
                if what:
                    tags.add(what)
                    mark(1, b.first, b.cnt)
                    for s in (0, 1, 126, 127):
                        mark(1, b.first + SUB * s, SUB)
    if c.m in (1, 8191, 8192, 8193, 16384):
        tags.add("A.count=%d" % c.m)
        for b in c.blocks(1):
            mark(1, b.first, b.cnt)
    # the bitmap
    h = c.ones()
    if c.m in (65535, 65536, 65537, 67583, 67584):
        tags.add("C.m=%d" % c.m)
    if c.m >= EF_SWITCH:
        w = h >> 6
        nchunks = (c.m + EF_CHUNK - 1) // EF_CHUNK
        for k in range(nchunks):
            i0, i1 = k * EF_CHUNK, min(c.m, (k + 1) * EF_CHUNK)
            rel = w[i0:i1] - w[i0]
            outside = rel >= EF_WORDS
            if i1 - i0 == EF_CHUNK and rel[-1] == EF_WORDS - 1:
                tags.add("C.last-key-at-w0+1023")
            if i1 - i0 == EF_CHUNK and rel[-1] == EF_WORDS:
                tags.add("C.last-key-at-w0+1024")
            if 2 * int(outside.sum()) > i1 - i0:
                tags.add("C.more-than-half-outside")
            if i1 < c.m:
                if outside.any() and (w[i0:i1][outside] == w[i1]).any():
                    tags.add("C.outside-bit-in-next-chunks-first-word")
                nxt = w[i1:min(c.m, i1 + EF_CHUNK)] - w[i1]
                if not outside.any() and (nxt < EF_WORDS).all() and w[i1 - 1] == w[i1] and h[i1] & 63:
                    tags.add("C.dense-boundary-mid-word")
        if int(h[-1]) >> 6 == c.nwords - 1:
            tags.add("C.last-one-in-last-word")
        if (c.nd + c.m + 3) % 64 in (0, 63):
            tags.add("C.tail%%64=%d" % ((c.nd + c.m + 3) % 64))
    # D and the columns
    raw = sparse_d_raw(c.N, c.M)
    if c.name.startswith("D_"):
        tags.add("D.clamped8" if raw < 8 else "D.D=%d" % c.D)
        if raw == 8:
            tags.add("D.unclamped8")
        ones = (1 << c.D) - 1
        lows = {k & ones for k in c.keys}
        highs = {c.high(i) for i in range(c.m)}
        if ones in lows:
            tags.add("D.low=ones")
        if 0 in lows:
            tags.add("D.low=zeros")
        if 0 in highs:
            tags.add("D.high=0")
        if ((c.N_end - 1) >> c.D if c.D < 128 else 0) in highs:
            tags.add("D.high=max")
        if c.words == 2 and c.keys[-1] >> 64:
            tags.add("D.two-word.D<64" if c.D < 64 else "D.two-word.D=64" if c.D == 64 else "D.two-word.D>64")
    return tags, {s: sorted(v) for s, v in marks.items()}


# ---- what the tests share ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def expected(oracle, name):
    """{suffix: bytes} the oracle writes for a case (oracle: the oracle_lib module), computed once"""
    c = case(name)
    if c.kind == "graph":
        return strip(oracle.write_graph(c.keys, c.counts, K_GRAPH, out="gr"), "gr")
    return strip(oracle.write_sparse_array(c.keys, c.N, c.M, base="sa", N_end=c.N_end), "sa")


def strip(files, base):
    """{suffix: bytes} of {base + suffix: bytes}"""
    return {n[len(base):]: b for n, b in files.items()}


def ds_parse(img):
    """A DenseSelect image: (header as 16 u64, [type bits of every block's index entry], [offset of every block])"""
    import struct
    h = struct.unpack("<16Q", img[:128])
    idx = struct.unpack("<%dQ" % h[8], img[h[2]:h[2] + 8 * h[8]])
    return h, [e & 7 for e in idx], [e & ~7 for e in idx]


FORM_BITS = {"small": 0, "large64": 1, "large32": 2, "inter": 5}
SUB_BITS = {0: 0, 8: 4, 16: 3, 32: 2}


def first_difference(got, exp):
    """A readable account of how two file sets differ: the first differing file, in it the first differing offset
    and, for a DenseSelect image, the block the offset lies in.  None when they are equal."""
    if sorted(got) != sorted(exp):
        return "file names differ: %s vs %s" % (sorted(got), sorted(exp))
    for name in sorted(exp):
        a, b = got[name], exp[name]
        if a == b:
            continue
        n = min(len(a), len(b))
        off = next((i for i in range(n) if a[i] != b[i]), n)
        where = ""
        if name.endswith(("-d0", "-d1")) and len(b) >= 128:
            h, types, offs = ds_parse(b)
            if off < 128:
                where = " (header word %d)" % (off // 8)
            elif off >= h[2]:
                where = " (%s array, entry %d)" % (("index", (off - h[2]) // 8) if off < h[3] else ("rank", (off - h[3]) // 8))
            else:
                blk = bisect.bisect_right(offs, off) - 1
                where = " (block %d of type %d, byte %d of it)" % (blk, types[blk], off - offs[blk])
        elif name.endswith(".high-bits"):
            where = " (word %d)" % (off // 8)
        return "%s: %d vs %d bytes, first difference at offset %d%s: %s vs %s" % (
            name, len(a), len(b), off, where, a[off:off + 8].hex(), b[off:off + 8].hex())
    return None


def key_tensor_values(keys, words):
    """the keys as the ABI lays them out: a flat list of signed 64-bit values (lo[, hi] per key)"""
    flat = []
    for p in keys:
        flat.append(p & MASK64)
        if words == 2:
            flat.append(p >> 64)
    return [x - (1 << 64) if x >= 1 << 63 else x for x in flat]


def expect_rank(keys, q):
    """(rank, present) of q among the ascending keys"""
    r = bisect.bisect_left(keys, q)
    return r, r < len(keys) and keys[r] == q


# ---- the ranges path: a case as a k-mer set cut into contiguous ranges ------------------------------------------------

RANGE_TAGS = ["R.cut=8191", "R.cut=8192", "R.cut=8193", "R.cut-in-tagged-block", "R.cut-in-tagged-sub-block", "R.cut-in-tagged-d0-block",
              "R.d0-edge-on-cut", "R.d0-edge-before-cut", "R.d0-edge-behind-cut", "R.empty-range-between-full",
              "R.tagged-block-assembled", "R.tagged-block-from-a-range"]


def kmer_universe(c):
    """(k, estimate): the smallest k-mer universe 4^k that holds the case, and an estimate that gives the case's D there"""
    k = next(k for k in range(1, 32) if 4 ** k >= c.N_end)
    return k, find_m(4 ** k, c.D)


def range_groups(c):
    """[(label, cuts)]: ascending key indices at which the case is cut into ranges, one context each (a cut twice: an
    empty range).  "edges": 8 191 / 8 192 / 8 193 and the keys whose high parts put an edge of a "-d0" block on the cut,
    one before it and one behind it; "inside": the middle of tagged blocks of both senses, inside tagged sub-blocks,
    an empty range between two full ones, and -- the window kernel starting in the middle of a chunk -- an odd index."""
    highs = [c.high(i) for i in range(c.m)]
    marks = realised(c)[1]
    edges = [8191, 8192, 8193]
    for delta in (0, -1, 1):
        for b in range(1, (highs[-1] >> 13) + 1):
            i = bisect.bisect_right(highs, BLOCK * b + delta)
            if 8193 < i < c.m and highs[i - 1] == BLOCK * b + delta and i not in edges:
                edges.append(i)
                break
    inside = []
    blocks1 = sorted(f for f, n in marks[1] if n == BLOCK)[:2]
    subs1 = sorted(f for f, n in marks[1] if n == SUB)
    inside += [f + BLOCK // 2 + 17 for f in blocks1]
    inside += [f + 31 for f in subs1[:1] + subs1[-1:]]
    for f, n in sorted(marks[0])[:2]:
        inside.append(bisect.bisect_right(highs, f + n // 2))
    inside += [c.m // 3 + 1001, c.m // 3 + 1001]
    return [("edges", sorted(edges)), ("inside", sorted(i for i in inside if 0 < i < c.m))]


def ranges_model(c, k, cuts):
    """Which DenseSelect blocks the ranges' owners build (those wholly inside a range's own ones, or zeros) -- the others
    are the assembler's: ({sense: set of blocks from ranges}, {sense: number of blocks}, tags of RANGE_TAGS realised)"""
    highs = [c.high(i) for i in range(c.m)]
    nd = 4 ** k >> c.D
    nb = {1: (c.m + BLOCK - 1) // BLOCK, 0: (nd + 2 + BLOCK - 1) // BLOCK}
    bounds = [0] + list(cuts) + [c.m]
    ranges = [(a, b - a) for a, b in zip(bounds, bounds[1:])]
    last = max(i for i, (f, n) in enumerate(ranges) if n)
    built, prev_high = {0: set(), 1: set()}, 0
    for i, (f, n) in enumerate(ranges):
        if not n:
            continue
        built[1].update(range((f + BLOCK - 1) // BLOCK, nb[1] if i == last else (f + n) // BLOCK))
        built[0].update(range((prev_high + BLOCK - 1) // BLOCK, nb[0] if i == last else highs[f + n - 1] // BLOCK))
        prev_high = highs[f + n - 1]
    marks = realised(c)[1]
    tags = set()
    for x in cuts:
        if x in (8191, 8192, 8193):
            tags.add("R.cut=%d" % x)
        if any(f < x < f + n for f, n in marks[1] if n == BLOCK):
            tags.add("R.cut-in-tagged-block")
        if any(f < x < f + n for f, n in marks[1] if n == SUB):
            tags.add("R.cut-in-tagged-sub-block")
        if any(f < highs[x - 1] < f + n for f, n in marks[0]):
            tags.add("R.cut-in-tagged-d0-block")
        tags |= {"R.d0-edge-on-cut"} if highs[x - 1] and highs[x - 1] % BLOCK == 0 else set()
        tags |= {"R.d0-edge-before-cut"} if highs[x - 1] % BLOCK == 1 else set()
        tags |= {"R.d0-edge-behind-cut"} if highs[x - 1] % BLOCK == BLOCK - 1 else set()
    if any(n == 0 and 0 < i < len(ranges) - 1 and ranges[i - 1][1] and ranges[i + 1][1] for i, (f, n) in enumerate(ranges)):
        tags.add("R.empty-range-between-full")
    for sense in (0, 1):
        tagged = {f // BLOCK for f, n in marks[sense]}
        if tagged - built[sense]:
            tags.add("R.tagged-block-assembled")
        if tagged & built[sense]:
            tags.add("R.tagged-block-from-a-range")
    return built, nb, tags
