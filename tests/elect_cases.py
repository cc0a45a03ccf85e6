"""The corpus of the elect tests: k-mer sets with a colour word per rank and the reads looked up in them.  Plain Python
over match_model.py, match_edges.py, classify_cases.py (its genomes and reads) and pool_model.py; nothing here knows the
library.  test_elect_cpu.py holds every case to the claims made here, so that test_gpu_elect.py cannot pass on an empty
case.

  every_rank     K = 5: every canonical 5-mer; colours[r] cycles through the zero word, the all-ones word, bit 0, bit 31,
                 bit 32, bit 63 and a random word; 1 500 reads of 5 .. 20 bases, so that several reads with different
                 words share one run of 64 positions.
  uniform, mixed, both, both_swapped
                 K = 5, the same 512 keys.  U: 24 bases whose 20 windows all bring the word W_U.  M: 24 bases whose
                 windows alternate between two words that differ only in the high half.  Alone, and the two in one run
                 of 64 positions in either order.
  tiles          K = 31, the long read of classify_cases: one read over four 2 048-byte tiles with one piece per tile;
                 the piece of tile j brings bit TILE_BITS[j], two of them >= 32.
  tile_newlines  K = 31: a read whose last base is byte 2 046, a '\\n' at byte 2 047 (the last of tile 0) and one at byte
                 2 048 (the first of tile 1), then a read that starts at byte 2 049; both reads end / begin with a piece.
  ranks<n>       n = 1, 63, 64, 65, 129: the reads of classify_cases.ranks(n) with colours[r] = 1 << (r % 64).
  edges<L>p<phase>[miss]   the reads of classify_cases.edges against the one planted key with the word EDGE_WORD; miss:
                 the strand no lookup finds.
  pool<S>        S = 1, 2, 30, 31, 33, 64: a planned pool of tiny sets over every third canonical 5-mer: one S-bit mask
                 per key, never zero, so that the key's colour word is its mask.
  command        three references over the genomes of classify_cases (K = 25): reference 0 = genomes 0 and 3, reference
                 1 = genomes 1 and 3, reference 2 = genome 2; the reads of sixteen25, and the two pair files."""
import functools
import random

import classify_cases as cc
import elect_model as em
import match_edges as me
import match_model as mm
import pool_model as pm

ONES = (1 << 64) - 1
SPECIAL = (0, ONES, 1 << 0, 1 << 31, 1 << 32, 1 << 63)
TILE_BITS = (3, 17, 40, 63)
EDGE_WORD = (1 << 37) | (1 << 2)
W_U = (1 << 5) | (1 << 44)
W_A, W_B = (1 << 9) | (1 << 35), (1 << 9) | (1 << 50)
W_REST = 1 << 7
POOL_SIZES = (1, 2, 30, 31, 33, 64)


def _case(K, keys, colours, data, ncolours=64):
    return {"K": K, "keys": list(keys), "colours": list(colours), "data": data, "ncolours": ncolours}


@functools.lru_cache(maxsize=None)
def all5():
    return tuple(sorted({mm.canonical(x, 5) for x in range(4 ** 5)}))


def every_rank():
    rng = random.Random(700)
    keys = all5()
    colours = [SPECIAL[r % 7] if r % 7 < 6 else rng.getrandbits(64) for r in range(len(keys))]
    reads = [mm.genome(rng, rng.randrange(5, 21)) for _ in range(1500)]
    return _case(5, keys, colours, ("\n".join(reads) + "\n").encode())


@functools.lru_cache(maxsize=None)
def or_reads():
    """(U, M, the colours of all5()): two reads of 24 bases with 20 distinct canonical 5-mers each, none shared"""
    rng = random.Random(710)
    while True:
        u, m = mm.genome(rng, 24), mm.genome(rng, 24)
        ku, km = (mm.canonical_many([(x, r) for _, x, r in mm.windows(t.encode(), 5)]) for t in (u, m))
        if len(set(ku)) == len(set(km)) == 20 and not set(ku) & set(km):
            break
    word = {x: W_U for x in ku}
    word.update({x: (W_A, W_B)[i % 2] for i, x in enumerate(km)})
    return u, m, tuple(word.get(x, W_REST) for x in all5())


def or_case(which):
    u, m, colours = or_reads()
    text = {"uniform": u + "\n", "mixed": m + "\n", "both": u + "\n" + m + "\n", "both_swapped": m + "\n" + u + "\n"}[which]
    return _case(5, all5(), colours, text.encode())


def _class_of(lhs, rhs):
    return [2 * a + b for a, b in zip(lhs, rhs)]


def tiles():
    c = cc.fixture("long")
    return _case(31, c["keys"], [1 << TILE_BITS[j] for j in _class_of(c["lhs"], c["rhs"])], c["data"])


@functools.lru_cache(maxsize=None)
def tile_newline_parts():
    """(first read, second read): the first has 2 047 bases and ends with a piece of genome 1, the second begins with a
    piece of genome 2"""
    gens = cc.genomes(31)[0]
    rng = random.Random(720)
    first = mm.genome(rng, cc.TILE - 1 - 62) + gens[1][100:162]
    second = gens[2][50:112] + mm.genome(rng, 40)
    return first, second


def tile_newlines():
    c = cc.fixture("long")
    first, second = tile_newline_parts()
    return _case(31, c["keys"], [1 << TILE_BITS[j] for j in _class_of(c["lhs"], c["rhs"])], (first + "\n\n" + second + "\n").encode())


def ranks(n):
    c = cc.fixture("ranks%d" % n)
    return _case(25, c["keys"], [1 << (r % 64) for r in range(n)], c["data"])


def edges(L, phase, miss=False):
    c = cc.fixture("edges%dp%d%s" % (L, phase, "miss" if miss else ""))
    return _case(L, c["keys"], [EDGE_WORD], c["data"])


@functools.lru_cache(maxsize=None)
def pool(S):
    """(keys, masks): every third canonical 5-mer with a non-zero S-bit mask; every sample holds at least one key"""
    rng = random.Random(730 + S)
    keys = all5()[::3]
    masks = [rng.randrange(1, 1 << S) for _ in keys]
    for i in range(S):
        masks[(7 * i) % len(keys)] |= 1 << i
    return keys, tuple(masks)


def pool_case(S):
    rng = random.Random(740 + S)
    keys, masks = pool(S)
    reads = [mm.genome(rng, rng.randrange(5, 12)) for _ in range(300)]
    return _case(5, keys, masks, ("\n".join(reads) + "\n").encode(), ncolours=S)


def pool_samples(S):
    keys, masks = pool(S)
    return pm.planned_samples(keys, masks, S)


REF_GENOMES = ((0, 3), (1, 3), (2,))


@functools.lru_cache(maxsize=None)
def command_refs():
    """(the references as texts, their canonical 25-mer sets, the sorted union, its colours)"""
    gens, sets = cc.genomes(25)[:2]
    texts = ["N".join(gens[j] for j in js) for js in REF_GENOMES]
    ref_sets = [set().union(*(sets[j] for j in js)) for js in REF_GENOMES]
    keys, colours = em.references(ref_sets)
    return tuple(texts), tuple(frozenset(s) for s in ref_sets), tuple(keys), tuple(colours)


def command():
    _, _, keys, colours = command_refs()
    return _case(25, keys, colours, cc.fixture("sixteen25")["data"], ncolours=3)


@functools.lru_cache(maxsize=None)
def command_pairs():
    """two files of 40 reads: classify_cases.pairs(), then mates without a window and mates that hit one reference only"""
    a, b, _ = cc.pairs()
    gens = cc.genomes(25)[0]
    only0, only1, only2 = (gens[j][30:90].encode() for j in (0, 1, 2))
    short = b"ACGTACGTAC"
    extra = [(short, only1), (short, only0), (only1, short), (short, short), (only2, only0), (only0, only1)]
    return list(a) + [x for x, _ in extra], list(b) + [y for _, y in extra]


CASES = ([("every_rank", every_rank)] + [(w, lambda w=w: or_case(w)) for w in ("uniform", "mixed", "both", "both_swapped")]
         + [("tiles", tiles), ("tile_newlines", tile_newlines)]
         + [("ranks%d" % n, lambda n=n: ranks(n)) for n in cc.RANK_SIZES]
         + [("edges%dp%d%s" % (L, ph, "miss" if miss else ""), lambda L=L, ph=ph, miss=miss: edges(L, ph, miss))
            for L in cc.EDGE_LENGTHS for ph in me.PHASES for miss in (False, True)]
         + [("pool%d" % S, lambda S=S: pool_case(S)) for S in POOL_SIZES]
         + [("command", command)])
NAMES = [n for n, _ in CASES]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return dict(CASES)[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(words, windows, by_count) of the model, computed once"""
    c = fixture(name)
    return em.colour_reads(c["data"], c["K"], c["keys"], c["colours"])
