"""The corpus of the classify tests: annotated k-mer sets and the reads classified against them.  Plain Python over
match_model.py and match_edges.py; nothing here knows the library.  test_classify_cpu.py holds every case to the claims
made here, so that test_gpu_classify.py cannot pass on an empty case.

  sixteen<K>   K = 25, 32.  Four random genomes of 300 bases whose canonical K-mer sets are pairwise disjoint; genome j
               carries the bits of class j: (lhs, rhs) = (0,0), (0,1), (1,0), (1,1).  For every mask m = 0 .. 15 three
               reads made of one 2K-base piece of every genome whose bit is set in m, on either strand, joined by N,
               with foreign bases around them (m = 0: foreign bases only).  Between them empty reads and reads of
               K - 1, K and K + 1 bases.
  dense        K = 5: every canonical 5-mer with random bits; 2 000 reads of 5 .. 9 bases, so that several reads with
               different masks share one run of 64 positions.
  long         K = 31: one read of 3 x 2 048 + 500 bases with one piece of each class, each in a tile of its own,
               foreign bases elsewhere; a short read before it and one after it.
  edges<L>p<phase>  L = 25, 31, 32, 63: the reads of match_edges.sweep(L, phase, rc_half=True) against the one planted
               key with bits (1, 0): every read holds the planted window, so its mask is 4.
  edges<L>p<phase>miss  the same reads against the set of the strand that no canonical lookup finds: every mask is 0.
               Together the two give both values at every d.
  ranks<n>     n = 1, 63, 64, 65, 129: the first n keys of sixteen25; the key at rank j has class j % 4, and read j is
               exactly that key's K bases, so its mask is 1 << (j % 4).
  pairs        two files of 40 reads drawn from sixteen25 (for the command)."""
import functools
import random

import classify_model as cm
import match_edges as me
import match_model as mm

TILE = 2048
BITS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (lhs, rhs) of class j


def key_text(x, K):
    return "".join("ACGT"[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def canonical_set(text, K):
    return set(mm.canonical_many([(x, r) for _, x, r in mm.windows(text.encode(), K)]))


@functools.lru_cache(maxsize=None)
def genomes(K):
    """(four genomes, their canonical K-mer sets, the sorted union, lhs bits, rhs bits)"""
    rng = random.Random(100 + K)
    gens = [mm.genome(rng, 300) for _ in range(4)]
    sets = [canonical_set(g, K) for g in gens]
    keys = sorted(set().union(*sets))
    cls = {x: j for j, s in enumerate(sets) for x in s}
    return gens, sets, keys, [BITS[cls[x]][0] for x in keys], [BITS[cls[x]][1] for x in keys]


def piece(rng, gen, K):
    p = rng.randrange(len(gen) - 2 * K)
    s = gen[p:p + 2 * K]
    return s if rng.random() < 0.5 else mm.rc_text(s)


@functools.lru_cache(maxsize=None)
def sixteen_reads(K):
    """[(the mask the read was made for, or None for the short reads, read text)]"""
    gens = genomes(K)[0]
    rng = random.Random(200 + K)
    reads = []
    for rep in range(3):
        for m in range(16):
            parts = [mm.genome(rng, rng.randrange(5, 40))]
            for j in range(4):
                if m >> j & 1:
                    parts.append(piece(rng, gens[j], K))
            rng.shuffle(parts)
            text = "N".join(parts) + mm.genome(rng, rng.randrange(0, 30))
            if m % 5 == 2:
                text = text.lower()
            reads.append((m, text))
            if (m + rep) % 4 == 1:
                reads.append((None, ""))
            if (m + rep) % 6 == 3:
                p = rng.randrange(200)
                g = gens[(m + rep) % 4]
                reads += [(None, g[p:p + K - 1]), (None, g[p:p + K]), (None, g[p:p + K + 1])]
    return tuple(reads)


def _case(K, keys, lhs, rhs, data):
    return {"K": K, "keys": list(keys), "lhs": list(lhs), "rhs": list(rhs), "data": data}


def sixteen(K):
    _, _, keys, lhs, rhs = genomes(K)
    return _case(K, keys, lhs, rhs, ("\n".join(t for _, t in sixteen_reads(K)) + "\n").encode())


def dense():
    K = 5
    rng = random.Random(300)
    keys = sorted({mm.canonical(x, K) for x in range(4 ** K)})
    lhs = [rng.randrange(2) for _ in keys]
    rhs = [rng.randrange(2) for _ in keys]
    reads = [mm.genome(rng, rng.randrange(5, 10)) for _ in range(2000)]
    return _case(K, keys, lhs, rhs, ("\n".join(reads) + "\n").encode())


LONG_PIECE_AT = 300                              # the offset of class j's piece in the long read: j * TILE + this


@functools.lru_cache(maxsize=None)
def long_parts():
    """(the read before, the long read, the read after, the four pieces)"""
    K = 31
    gens = genomes(K)[0]
    rng = random.Random(400)
    body = list(mm.genome(rng, 3 * TILE + 500))
    pieces = []
    for j in range(4):
        s = piece(rng, gens[j], K)
        pieces.append(s)
        at = j * TILE + LONG_PIECE_AT
        body[at:at + len(s)] = s
    before = mm.genome(rng, 20) + gens[2][40:40 + K + 3] + mm.genome(rng, 9)
    after = mm.genome(rng, 90)
    return before, "".join(body), after, tuple(pieces)


def long():
    K = 31
    _, _, keys, lhs, rhs = genomes(K)
    before, body, after, _ = long_parts()
    return _case(K, keys, lhs, rhs, (before + "\n" + body + "\n" + after + "\n").encode())


EDGE_LENGTHS = (25, 31, 32, 63)


def edges(L, phase, miss=False):
    data, _ = me.sweep(L, phase, True)
    x = me.key_of(me.planted(L)[0])
    c = mm.canonical(x, L)
    key = (mm.revcomp(c, L) if miss else c)
    return _case(L, [key], [1], [0], data)


RANK_SIZES = (1, 63, 64, 65, 129)


def ranks(n):
    K = 25
    keys = genomes(K)[2][:n]
    reads = [key_text(x, K) for x in keys]
    return _case(K, keys, [BITS[j % 4][0] for j in range(n)], [BITS[j % 4][1] for j in range(n)], ("\n".join(reads) + "\n").encode())


@functools.lru_cache(maxsize=None)
def pairs():
    """(file 1, file 2) as lists of 40 reads of sixteen25, and the masks the halves were made for"""
    by_mask = {}
    for m, t in sixteen_reads(25):
        if m is not None:
            by_mask.setdefault(m, []).append(t)
    rng = random.Random(500)
    want = [(0, 0), (1, 8), (2, 0), (4, 1), (2, 4), (8, 2), (0, 4), (3, 12)]
    while len(want) < 40:
        want.append((rng.randrange(16), rng.randrange(16)))
    a = [rng.choice(by_mask[x]).encode() for x, _ in want]
    b = [rng.choice(by_mask[y]).encode() for _, y in want]
    return a, b, tuple(want)


CASES = ([("sixteen%d" % K, lambda K=K: sixteen(K)) for K in (25, 32)] + [("dense", dense), ("long", long)]
         + [("edges%dp%d%s" % (L, ph, "miss" if miss else ""), lambda L=L, ph=ph, miss=miss: edges(L, ph, miss))
            for L in EDGE_LENGTHS for ph in me.PHASES for miss in (False, True)]
         + [("ranks%d" % n, lambda n=n: ranks(n)) for n in RANK_SIZES])
NAMES = [n for n, _ in CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return dict(CASES)[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(classes, windows, counts) of the model, computed once"""
    c = fixture(name)
    return cm.classify(c["data"], c["K"], c["keys"], c["lhs"], c["rhs"])
