"""The edge corpus of the kernels that stage a tile of reads (match_reads, the mark kernel of mark_reads): inputs whose
windows lie where the layout has an edge, and the keys of the objects they are matched against.  Plain Python over
match_model.py; nothing here knows the library.

The layout: a tile is 2 048 byte positions, a run 64, the halo behind a tile 64 positions for windows of up to 63 bases;
a key is one word up to 31 bases and two words from 32.

  length classes   k-mer sets at K = L of KMER_LENGTHS, graphs at K of GRAPH_KS (L = K + 1 = 31, 32, 63): the widest
                   one-word key, the narrowest and the widest two-word key, and the lengths at which almost every window
                   is a hit
  sweep (L >= 16)  for every d in 0 .. L + 1 a read of 2 046 bases with one planted L-mer X -- the object's one key; a
                   graph holds X and its reverse complement -- that starts at an absolute position = phase - d
                   (mod 2 048): phase 0 is the tile's edge, where the window ends in the halo, phase 1 024 a run's edge
                   inside a tile.  Everything else in the read is foreign: no window of it is X or rc(X).  For odd d a
                   non-base byte sits three positions before the planted window, so that the windows it forbids straddle
                   the same edge.  With rc_half every other pair of reads holds rc(X) instead (for graphs, and for
                   k-mer sets matched with normalize, where the object holds the canonical form of X)
  small sweep      L <= 6, where planting cannot work: a random half of all keys (of the canonical keys for normalize),
                   random bases in reads of 0 .. 300 bases (every tenth of 0, 1, L - 1, L or L + 1), about 20 000 bytes
  newline cases    L of NEWLINE_LENGTHS: a tile of nothing but '\\n', a '\\n' as a tile's last and as its first byte and
                   at positions 63 and 64 of a run, reads of one base, a read that ends with its tile, inputs of exactly
                   2 047, 2 048, 2 049 and 4 096 bytes with and without the last '\\n', reads over three tiles whose
                   only hit lies in the first and in the last
  byte values      L of BYTE_LENGTHS: a core of 2 L + 1 bases 256 times, its middle byte replaced by every byte value;
                   the object is what build-kmer-set / build-graph makes of these very bytes

test_match_edges_cpu.py holds the corpus to these claims; test_gpu_match_edges.py runs the device over it.

How SMALL_SEEDS were chosen: find_small_seeds() (by hand, a second) takes for every L the first seed at which the small
sweep meets its condition for both key sets: at every d = 0 .. L + 1, among the valid windows that start at a position
= -d (mod 2 048), one is in the object and one is not."""
import functools
import random

import match_model as mm

TILE, RUN = 2048, 64
KMER_LENGTHS = (1, 2, 3, 6, 16, 31, 32, 33, 62, 63)
GRAPH_KS = (30, 31, 62)
CLASSES = [("kmers%d" % K, K, False) for K in KMER_LENGTHS] + [("graph%d" % K, K, True) for K in GRAPH_KS]
NEWLINE_LENGTHS = (3, 31, 32)
BYTE_LENGTHS = (3, 25, 32)
# what match_reads is run over: the length classes, and K = 25 for the sake of its byte values
MATCHED = CLASSES + [("kmers25", 25, False)]
PHASES = (0, 1024)
# what stands three positions before every other planted window: letters next to the bases' in either case, IUPAC
# codes, bytes that differ from a base in one bit (0xC1 = 'A' | 0x80, '!' = 'a' ^ 0x40), a blank, NUL and 0xFF
NON_BASES = (ord("N"), ord("n"), 0, ord("U"), 0xC1, ord(" "), ord("u"), 0xFF, ord("B"), ord("!"), ord("d"), ord("@"))
BODY, AT = 2046, 1024           # the sweep's reads: bases per read, the planted window's offset in its read
SMALL_SEEDS = {1: 0, 2: 0, 3: 0, 6: 0}

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def length_of(K, graph):
    return K + 1 if graph else K


def key_words(L):
    return 1 if 2 * L <= 62 else 2


def rc_bytes(s):
    return s[::-1].translate(_COMP)


def key_of(text):
    v = 0
    for ch in text:
        v = (v << 2) | mm.CODE[ch]
    return v


# ---- foreign sequence ----------------------------------------------------------------------------------------------

def occurrences(text, avoid):
    """how many windows of `text`, compared without case, are one of `avoid` (upper-case texts of one length)"""
    if not avoid:
        return 0
    L = len(next(iter(avoid)))
    up = text.upper()
    return sum(1 for i in range(len(up) - L + 1) if up[i:i + L] in avoid)


def foreign(rng, n, avoid, before=b""):
    """n random bases, one in ten in lower case, that may follow `before`: no base completes a window of `avoid`"""
    L = len(next(iter(avoid)))
    up = bytearray(before.upper()[-(L - 1):] if L > 1 else b"")
    skip = len(up)
    while len(up) - skip < n:
        ch = rng.choice(b"ACGT")
        if bytes(up[max(0, len(up) - (L - 1)):]) + bytes([ch]) not in avoid:
            up.append(ch)
    return bytes(c | 0x20 if rng.random() < 0.1 else c for c in up[skip:])


def lead(rng, n, avoid, plant):
    """n foreign bases that `plant` may follow: no window across the joint is one of `avoid` either"""
    L = len(plant)
    while True:
        s = foreign(rng, n, avoid)
        if not occurrences(s[len(s) - min(len(s), L - 1):] + plant[:L - 1], avoid):
            return s


@functools.lru_cache(maxsize=None)
def planted(L):
    """(X, {X, rc(X)}) as upper-case texts: the key the sweep and the newline cases of a length plant.  X begins with T,
    so that the key's top two bits are set, and is not its own reverse complement"""
    rng = random.Random(4000 + L)
    while True:
        x = b"T" + bytes(rng.choice(b"ACGT") for _ in range(L - 1))
        if rc_bytes(x) != x:
            return x, frozenset((x, rc_bytes(x)))


def planted_keys(L, graph, normalize):
    """the object of the sweep and of the newline cases"""
    x = key_of(planted(L)[0])
    if graph:
        return frozenset((x, mm.revcomp(x, L)))
    return frozenset((mm.canonical(x, L) if normalize else x,))


# ---- the sweep for L >= 16 -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sweep(L, phase, rc_half):
    """(the input, [(d, absolute position of the planted window)]), one read per d = 0 .. L + 1.  Every read has BODY
    bases and its '\\n', so every read begins one position earlier in its tile than the read before, and the planted
    window, AT bases into its read, with it; the first read of phase 0 has 1 024 bases more in front."""
    assert 16 <= L <= 63 and phase in PHASES
    x, avoid = planted(L)
    rng = random.Random(10 * L + (1 if phase else 0) + (2 if rc_half else 0))
    out, where, at = [], [], 0
    for d in range(L + 2):
        text = rc_bytes(x) if rc_half and (d // 2) % 2 else x
        if d % 5 == 4:
            text = text.lower()
        n = AT + (TILE - AT - phase if d == 0 else 0)
        a = bytearray(lead(rng, n, avoid, text.upper()))
        if d % 2:
            a[-3] = NON_BASES[(d // 2) % len(NON_BASES)]
        where.append((d, at + n))
        read = bytes(a) + text + foreign(rng, BODY - AT - L, avoid, before=text) + b"\n"
        out.append(read)
        at += len(read)
    data = b"".join(out)
    return (data[:-1] if phase else data), where           # (the second sweep ends without its '\n')


# ---- the sweep for L <= 6 --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_sweep(L, seed=None):
    rng = random.Random(100 * L + (SMALL_SEEDS[L] if seed is None else seed))
    out, n = [], 0
    while n < 20000:
        # (every tenth read has 0, 1, L - 1, L or L + 1 bases)
        length = (0, 1, L - 1, L, L + 1)[len(out) // 10 % 5] if len(out) % 10 == 9 else rng.randint(0, 300)
        r = bytes(rng.choice(b"ACGT") | (0x20 if rng.random() < 0.1 else 0) for _ in range(length))
        out.append(r)
        n += len(r) + 1
    return b"\n".join(out) + b"\n"


@functools.lru_cache(maxsize=None)
def small_keys(L, normalize):
    """a random half of all 4^L keys; for normalize a random half of the canonical ones"""
    rng = random.Random(200 + L)
    every = sorted({mm.canonical(x, L) for x in range(4 ** L)}) if normalize else list(range(4 ** L))
    return frozenset(rng.sample(every, len(every) // 2))


def small_residues(L, data, keys, normalize):
    """{d: (present, absent)} over the valid windows that start at a position = -d (mod 2 048), d = 0 .. L + 1"""
    seen = {d: [0, 0] for d in range(L + 2)}
    for b, e in mm.read_spans(data):
        ws = mm.windows(data[b:e], L)
        ks = mm.canonical_many([(x, r) for _, x, r in ws]) if normalize else [x for _, x, _ in ws]
        for (p, _, _), x in zip(ws, ks):
            d = -(b + p) % TILE
            if d in seen:
                seen[d][0 if x in keys else 1] += 1
    return {d: tuple(v) for d, v in seen.items()}


def find_small_seeds(limit=200):
    """by hand only: see the module's comment"""
    out = {}
    for L in (L for L in KMER_LENGTHS if L <= 6):
        out[L] = next(s for s in range(limit) if all(min(v) > 0 for nz in (False, True) for v in
                                                     small_residues(L, small_sweep(L, s), small_keys(L, nz), nz).values()))
    return out


# ---- newline and length edges ----------------------------------------------------------------------------------------

EXACT = (2047, 2048, 2049, 4096)


@functools.lru_cache(maxsize=None)
def newline_cases(L):
    """{name: input}; X = planted(L)[0] is the only window of any of them that is X or rc(X)"""
    x, avoid = planted(L)
    rng = random.Random(7000 + L)

    def P(n):
        return lead(rng, n, avoid, x)

    def F(n, before=b""):
        return foreign(rng, n, avoid, before)

    cases = {
        # a read of 2 048 bases whose last window is X, a tile of 2 048 '\n' (it touches 2 049 reads), X alone
        "newlines2048": P(TILE - L) + x + b"\n" * TILE + x + b"\n",
        # the '\n' of a matching read as the last byte of its tile; the next read begins with the next tile
        "newline_last_in_tile": P(TILE - 1 - L) + x + b"\n" + x + F(10, x) + b"\n",
        # a matching read that ends with its tile: its '\n' is the first byte of the next
        "newline_first_in_tile": P(TILE - L) + x + b"\n" + x + F(10, x) + b"\n",
        "newlines_across_tiles": P(TILE - 1 - L) + x + b"\n\n" + x + F(10, x) + b"\n",
        "newline_at_63": F(5 * RUN + 63) + b"\n" + x + F(20, x) + b"\n",
        "newline_at_64": F(5 * RUN + 64) + b"\n" + x + F(20, x) + b"\n",
        "newlines_at_63_64": F(5 * RUN + 63) + b"\n\n" + x + F(20, x) + b"\n",
        "one_base_reads": b"".join(bytes([c]) + b"\n" for c in b"ACGTNacgt" * 130) + x + b"\n" + b"G\nt\n" * 20 + b"C",
        # the input ends with a matching read and with its tile, no '\n'
        "ends_with_tile": F(100) + b"\n" + P(TILE - 101 - L) + x,
        "three_tiles_hit_in_first": P(100) + x + F(5000, x) + b"\n",
        "three_tiles_hit_in_last": P(2 * TILE + 104) + x + F(100, x) + b"\n",
    }
    for n in EXACT:
        cases["exact%d" % n] = P(n - L) + x
        cases["exact%dnl" % n] = P(n - 1 - L) + x + b"\n"
    return cases


# ---- every byte value ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def byte_input(L, core=None):
    """256 reads: read b is the core (2 L + 1 bases, random unless given) with its middle byte replaced by byte b"""
    if core is None:
        rng = random.Random(256 + L)
        core = bytes(rng.choice(b"ACGT") for _ in range(2 * L + 1))
    assert len(core) == 2 * L + 1
    return b"".join(core[:L] + bytes([b]) + core[L + 1:] + b"\n" for b in range(256))


# ---- what is run -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def runs(K, graph):
    """[(name, input, normalize, keys of the object)]: every input of a length class under every normalize value it is
    run with -- both for a k-mer set, none for a graph, as the commands match them"""
    L = length_of(K, graph)
    out = []
    for nz in ((False,) if graph else (False, True)):
        tag = "-normalize" if nz else ""
        if L >= 16:
            for phase in PHASES:
                out.append(("sweep%d%s" % (phase, tag), sweep(L, phase, graph or nz)[0], nz, planted_keys(L, graph, nz)))
        else:
            out.append(("small%s" % tag, small_sweep(L), nz, small_keys(L, nz)))
        if L in NEWLINE_LENGTHS:
            for name, data in newline_cases(L).items():
                out.append((name + tag, data, nz, planted_keys(L, graph, nz)))
        if L in BYTE_LENGTHS:
            data = byte_input(L)
            out.append(("bytes%s" % tag, data, nz, frozenset(mm.object_keys(data, K, graph))))
    return out


@functools.lru_cache(maxsize=None)
def expected(K, graph, name, any_mode):
    """match_model.match of one run, computed once for the tests that share it"""
    _, data, nz, keys = next(r for r in runs(K, graph) if r[0] == name)
    return mm.match(data, length_of(K, graph), keys, normalize=nz, any=any_mode)
