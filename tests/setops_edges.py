"""The corpus that holds the set algebra, the annotation bitmaps, graph-to-kmer-set, the text forms and lint to their
models (tests/setops_model.py) and the oracle at the edges of the kernels behind them: select_count_kernel /
select_write_kernel / mark_normal_kernel / count_bits_kernel (kernels_runs.hpp), dump_kmers_kernel / dump_line_len_kernel
/ dump_edges_kernel / lint_edges_kernel (kernels_text.hpp).  Plain Python: no reads, no genome, no device, and the oracle
only where a test hands it in.  Every key list is explicit and sorted; where keys are drawn they come from a seeded
random.Random.  No case holds more than about 70 000 keys.

A case is a name, its inputs, and the condition tags it is there for.  realised(case) derives the tags from the DATA
(never from the name); test_setops_cpu.py demands realised(case) == case.tags for every case and that every tag of
CONDITIONS occurs.

The geometry the selection cases are laid on: select_* works in tiles of 4 096 items; item i of a tile is row i // 256
(of 16), wave (i % 256) // 64 (of 4), lane i % 64.  A planned selection case is ONE run of n items whose counts are chosen
so that the items kept by the window 5 .. 9 are exactly a planned index set: kept items carry 5, 7, 9 in turn (both bounds
are taken), dropped ones 4, 10, 1, 2^32 - 1 in turn (the values next to both bounds).

Left out on purpose:
  * lint on a list that goes DOWN somewhere: the kernel finds the reverse complement by binary search, which has no
    defined answer there.  goss_gpu_push_run_host takes a run as it is (a lone run is not sorted by finish), so a list
    with an equal neighbour -- non-decreasing, the search still defined -- is a case: kind 4 comes from there.
  * estimates above 64 m (emit_estimate): the high-bits bitmap grows with the estimate.
  * a key list above 70 000 keys, --tmp-dir spills, the distributed set algebra, the merge paths (merge_model.py).
"""
import functools
import random

import setops_model as sm

U32 = sm.U32
M64 = sm.M64
TILE, ROW, WAVE = 4096, 256, 64


class Case:
    def __init__(self, name, kind, tags, **kw):
        self.name, self.kind, self.tags = name, kind, frozenset(tags)
        self.__dict__.update(kw)

    def __repr__(self):
        return "Case(%s)" % self.name


def words_of(K):
    return 1 if 2 * K <= 62 else 2


@functools.lru_cache(maxsize=None)
def drawn_keys(bits, n, seed):
    """n distinct keys of `bits` bits, ascending"""
    rng = random.Random(seed * 7919 + bits * 131 + n)
    assert n <= 1 << bits
    if n * 2 > 1 << bits:
        return tuple(sorted(rng.sample(range(1 << bits), n)))
    s = set()
    while len(s) < n:
        s.add(rng.getrandbits(bits))
    return tuple(sorted(s))


# ---- selection: planned kept sets ---------------------------------------------------------------------------------------

SEL_N = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193]
SEL_N_THREE_TILES = [8193, 12288]          # a whole tile between two tiles: 8 193 (the third tile is one item) and three full ones
SEL_KS = [(25, 63), (31, 32)]              # every planned case at a one-word and at a two-word key width, in turn
WINDOW = (5, 9)
KEPT_COUNTS, DROPPED_COUNTS = (5, 7, 9), (4, 10, 1, U32)

PATTERNS = {
    "none": lambda i, n: False,
    "all": lambda i, n: True,
    "first": lambda i, n: i == 0,
    "last": lambda i, n: i == n - 1,
    "lane63": lambda i, n: i % WAVE == WAVE - 1,          # only the last lane of every wave
    "lane0": lambda i, n: i % WAVE == 0,
    "row255": lambda i, n: i % ROW == ROW - 1,            # the last item of every row (the last lane of its last wave)
    "row0": lambda i, n: i % ROW == 0,
    "tile4095": lambda i, n: i % TILE == TILE - 1,
    "tile0": lambda i, n: i % TILE == 0,
    "tile1-empty": lambda i, n: i // TILE != 1,           # a whole tile keeps nothing between two that keep everything
    "tile1-only": lambda i, n: i // TILE == 1,
    "period65": lambda i, n: i % 65 == 0,                 # a wrong stride shows in every row
    "period257": lambda i, n: i % 257 == 0,
}


def kept_of(pattern, n):
    """the planned index set, or None where the pattern says nothing at this n (it keeps nothing or everything, or has no
    third tile)"""
    if pattern in ("tile1-empty", "tile1-only") and n <= 2 * TILE:
        return None
    f = PATTERNS[pattern]
    kept = tuple(i for i in range(n) if f(i, n))
    if pattern not in ("none", "all") and len(kept) in (0, n):
        return None
    return kept


def planned_counts(n, kept):
    ks = set(kept)
    counts, a, b = [], 0, 0
    for i in range(n):
        if i in ks:
            counts.append(KEPT_COUNTS[a % 3])
            a += 1
        else:
            counts.append(DROPPED_COUNTS[b % 4])
            b += 1
    return counts


def _bound_tags(nkept, ndropped):
    t = []
    if nkept >= 1:
        t.append("S.count=lo-kept")
    if nkept >= 3:
        t.append("S.count=hi-kept")
    if ndropped >= 1:
        t.append("S.count=lo-1-dropped")
    if ndropped >= 2:
        t.append("S.count=hi+1-dropped")
    return t


def _select_cases():
    idx = 0
    for n in sorted(set(SEL_N) | set(SEL_N_THREE_TILES)):
        groups = {}
        for p in PATTERNS:
            if n not in SEL_N and p not in ("tile1-empty", "tile1-only"):
                continue
            kept = kept_of(p, n)
            if kept is not None:
                groups.setdefault(kept, []).append(p)
        for kept, ps in groups.items():
            for K in SEL_KS[idx % 2]:
                name = "sel_n%d_%s_k%d" % (n, ps[0], K)
                tags = ["S.n=%d" % n, "S.K=%d" % K] + ["S.keep=%s" % p for p in ps] + _bound_tags(len(kept), n - len(kept))

                def make(name=name, n=n, K=K, kept=kept, tags=tags):
                    keys = list(drawn_keys(2 * K, n, 11))
                    return Case(name, "select", tags, K=K, runs=[(keys, planned_counts(n, kept))], windows=[WINDOW])
                yield name, make
            idx += 1


# ---- selection: count windows over merged runs ------------------------------------------------------------------------------

def _window_cases():
    def subtract():
        ks = drawn_keys(50, 6000, 21)
        a = [k for j, k in enumerate(ks) if j % 3 != 1]          # j % 3: 0 both (3), 1 rhs only (2), 2 lhs only (1)
        b = [k for j, k in enumerate(ks) if j % 3 != 2]
        return Case("win_1_1", "select", ["W.1..1", "W.1..1.at-lo", "W.1..1.at-hi", "W.1..1.hi+1", "W.counts-1-2-3", "W.runs=2", "S.K=25"],
                    K=25, runs=[(a, 1), (b, 2)], windows=[(1, 1)])
    yield "win_1_1", subtract

    for s in (2, 3, 6):
        def sets(s=s):
            # s distinct sets and the first given twice: a key of all has s + 1, one that misses a set given once s,
            # one that misses the set given twice s - 1, one of the second set alone 1
            ks = drawn_keys(50, 4000, 30 + s)
            A = []
            for i in range(s):
                A.append([k for j, k in enumerate(ks) if j % 4 == 0 or (j % 4 == 1 and i != 1) or (j % 4 == 2 and i != 0)
                          or (j % 4 == 3 and i == 1)])
            w = "W.%d..%d" % (s, s)
            return Case("win_%d_sets" % s, "select", [w, w + ".lo-1", w + ".at-lo", w + ".at-hi", w + ".hi+1", "W.runs=%d" % (s + 1), "S.K=31"],
                        K=31, runs=[(x, 1) for x in A] + [(A[0], 1)], windows=[(s, s)])
        yield "win_%d_sets" % s, sets

    def top():
        ks = list(drawn_keys(64, 3000, 41))
        # a run of literal counts and a run of weight 1 over every third key: 1, 2, 3, 2^32 - 2, 2^32 - 1 (twice: as a
        # literal count and as 2^32 - 2 + 1; 2^32 - 1 + 1 saturates)
        c = [(1, 2, U32 - 2, U32 - 1, U32)[j % 5] for j in range(len(ks))]
        return [(ks, c), (ks[::3], 1)]

    def top_2():
        w = "W.2..%d" % U32
        return Case("win_2_max", "select", [w, w + ".lo-1", w + ".at-lo", w + ".at-hi", "W.runs=2", "S.K=32"], K=32, runs=top(),
                    windows=[(2, U32)])
    yield "win_2_max", top_2

    def top_max():
        w = "W.%d..%d" % (U32, U32)
        return Case("win_max_max", "select", [w, w + ".lo-1", w + ".at-lo", w + ".at-hi", "W.runs=2", "S.K=32"], K=32, runs=top(),
                    windows=[(U32, U32)])
    yield "win_max_max", top_max

    def zero(merged):
        ks = list(drawn_keys(126, 5000, 43))
        c = [(0, 1, 0, 2)[j % 4] for j in range(len(ks))]
        runs = [(ks, c)] + ([(ks[::2], [0] * len(ks[::2])), (ks[1::5], 0)] if merged else [])
        name = "win_0_0_merged" if merged else "win_0_0"
        return Case(name, "select", ["W.0..0", "W.0..0.at-lo", "W.0..0.at-hi", "W.0..0.hi+1", "W.zero-count", "W.runs=%d" % len(runs), "S.K=63"],
                    K=63, runs=runs, windows=[(0, 0)])
    yield "win_0_0", lambda: zero(False)
    yield "win_0_0_merged", lambda: zero(True)

    def twice():
        w = "W.2..%d" % U32
        return Case("win_twice", "select", [w, w + ".lo-1", w + ".at-lo", w + ".at-hi", "W.runs=2", "W.twice", "S.K=32"], K=32, runs=top(),
                    windows=[(2, U32), (3, 3)])
    yield "win_twice", twice


# ---- the set algebra as the commands compose it -----------------------------------------------------------------------------

def _scenarios():
    """(name, K, [sets], tags of the relation)"""
    K = 25
    top = (1 << (2 * K)) - 1
    ks = [k for k in drawn_keys(2 * K, 3002, 51) if k not in (0, top)][:3000]
    ev, od = ks[0::2], ks[1::2]
    yield "disjoint", K, [ev, od], ["A.disjoint", "A.interleaved"]
    yield "identical", K, [ks, ks], ["A.identical"]
    yield "b_empty", K, [ks, []], ["A.b-empty"]
    yield "a_empty", K, [[], ks], ["A.a-empty"]
    yield "nested", K, [ks, ks[100:2000:3]], ["A.nested"]
    yield "first_key", K, [ks[:1] + ks[2:], ks[1:]], ["A.differ-first"]
    yield "last_key", K, [ks[:-1], ks[:-2] + ks[-1:]], ["A.differ-last"]
    yield "key0", K, [[0] + ks, ks], ["A.differ-key0", "A.nested"]
    yield "top_key", K, [ks + [top], ks], ["A.differ-max", "A.nested"]
    # K = 32 and 63 take two-word keys; a 32-mer has 64 bits, so its high word is always zero: there the key that differs "at
    # the top" differs in bit 63, the sign bit of the low word
    for K2 in (32, 63):
        base = [k for k in drawn_keys(2 * K2, 2000, 52)]
        x = base[1000]
        hi = x ^ (1 << (64 if K2 == 63 else 63))          # the same low word, another high word
        lo = x ^ 1                                        # the same high word, another low word
        rest = [k for k in base if k not in (x, hi, lo)]
        yield "high_word_k%d" % K2, K2, [sorted(rest + [x]), sorted(rest + [hi])], ["A.differ-high-word" if K2 == 63 else "A.differ-bit63"]
        yield "low_word_k%d" % K2, K2, [sorted(rest + [x]), sorted(rest + [lo])], ["A.differ-low-word"]


def _algebra_cases():
    for sname, K, sets, rel in _scenarios():
        for op in ("intersect", "subtract", "annotate"):
            name = "%s_%s" % (op, sname)
            tags = ["A.op=%s" % op, "A.K=%d" % K] + rel

            def make(name=name, K=K, sets=sets, op=op, tags=tags):
                tags = list(tags)
                try:
                    r = _algebra_result(op, sets)
                    if not r:
                        tags.append("A.result-empty")
                except sm.Refused:
                    tags.append("A.refused")
                return Case(name, "algebra", tags, K=K, sets=[list(s) for s in sets], op=op)
            yield name, make
    K = 25
    ks = list(drawn_keys(2 * K, 3000, 53))
    for name, sets, extra in (("intersect_three_times", [ks, ks, ks], ["A.same-set-3x"]),
                              ("intersect_one_empty_among_full", [ks, [], ks[::2]], ["A.one-empty-among-full"]),
                              ("intersect_all_empty", [[], []], ["A.all-empty", "A.undefined"])):
        yield name, (lambda name=name, sets=sets, extra=extra:
                     Case(name, "algebra", ["A.op=intersect", "A.K=25"] + extra, K=25, sets=sets, op="intersect"))


def _algebra_result(op, sets):
    if op == "intersect":
        return sm.intersect(sets)
    if op == "subtract":
        return sm.subtract(*sets)
    return sm.annotate(*sets)[0]


# ---- annotation: count_bits_kernel ---------------------------------------------------------------------------------------------

BITS_M = [1, 63, 64, 65, 4031, 4032, 4033, 4095, 4096, 4097, 16383, 16384, 16385]          # (m = 0: through the ABI only)
BITS_K = 25
# count of item i of m: 1 lhs only, 2 rhs only, 3 both, 4 neither (a third run of weight 4: at the ABI a count is a number)
BITS_PATTERNS = {
    "all-lhs": lambda i, m: 1,
    "all-rhs": lambda i, m: 2,
    "all-common": lambda i, m: 3,
    "lhs=last-item": lambda i, m: 1 if i == m - 1 else 2,
    "lhs=item63-of-last-full-word": lambda i, m: 1 if i == m // 64 * 64 - 1 else 2,
    "lhs=mod65,rhs=mod63": lambda i, m: (1 if i % 65 == 0 else 0) + (2 if i % 63 == 0 else 0) or 4,
    "lhs=even-words": lambda i, m: (1 if (i // 64) % 2 == 0 else 0) + (2 if i % 3 == 0 else 0) or 4,
}


def bits_counts(pattern, m):
    if pattern == "lhs=item63-of-last-full-word" and m < 64:
        return None
    if pattern == "lhs=last-item" and m < 2:
        return None
    f = BITS_PATTERNS[pattern]
    return tuple(f(i, m) for i in range(m))


def _bits_cases():
    for m in BITS_M:
        groups = {}
        for p in BITS_PATTERNS:
            c = bits_counts(p, m)
            if c is not None:
                groups.setdefault(c, []).append(p)
        for counts, ps in groups.items():
            name = "bits_m%d_%s" % (m, ps[0])
            yield name, (lambda name=name, m=m, counts=counts, ps=ps:
                         Case(name, "bits", ["B.m=%d" % m] + ["B.%s" % p for p in ps], K=BITS_K,
                              keys=list(drawn_keys(2 * BITS_K, m, 61)), counts=list(counts)))


# ---- graph-to-kmer-set: mark_normal_kernel ---------------------------------------------------------------------------------------

def _g2k_long(K):
    """a few hundred edges of K + 1 bases with their reverse complements: A..A / T..T, where K + 1 is even an edge that is
    its own reverse complement, where the key has two words a pair that differs in the high word only and one that differs
    in the low word only"""
    length = K + 1
    rng = random.Random(700 + K)
    e = {0}                                                            # A..A; its reverse complement T..T joins below
    if length % 2 == 0:
        half = rng.getrandbits(length)
        e.add((half << length) | sm.revcomp(half, length // 2))         # u + rc(u)
    while len(e) < 150:
        e.add(rng.getrandbits(2 * length))
    if 2 * length > 64:
        x = rng.getrandbits(2 * length)
        e |= {x, x ^ (1 << 64), x ^ (1 << (2 * length - 1)), x ^ 1, x ^ (1 << 63)}
    e |= {sm.revcomp(x, length) for x in e}
    return sorted(e)


def _g2k_cases():
    for K in range(1, 6):
        n = 1 << (2 * (K + 1))
        yield "g2k_all_k%d" % K, (lambda K=K, n=n: Case("g2k_all_k%d" % K, "g2k", ["G.all-edges.K=%d" % K] + (["G.self-complementary"] if K % 2 else []),
                                                       K=K, edges=list(range(n))))
    import dense_graphs as dg
    for gname, K, edges, counts in dg.corpus():
        if len(edges) == 1 << (2 * K + 2):
            continue                                         # (a complete graph: g2k_all_k<K> above)
        name = "g2k_dense_" + gname
        yield name, (lambda name=name, K=K, edges=edges: Case(name, "g2k", _g2k_tags(edges, K, ["G.dense-corpus"]), K=K, edges=list(edges)))
    for K in (30, 31, 62):
        def long_(K=K):
            e = _g2k_long(K)
            return Case("g2k_long_k%d" % K, "g2k", _g2k_tags(e, K, ["G.len=%d" % (K + 1)]), K=K, edges=e)
        yield "g2k_long_k%d" % K, long_

    def asym():
        e = _g2k_long(31)
        lone = [x for x in e if sm.revcomp(x, 32) != x and x != 0][::7]          # these lose their reverse complements
        gone = {sm.revcomp(x, 32) for x in lone}
        e = [x for x in e if x not in gone]
        return Case("g2k_asymmetric_k31", "g2k", _g2k_tags(e, 31, ["G.len=32"]), K=31, edges=e)
    yield "g2k_asymmetric_k31", asym


def _g2k_tags(edges, K, tags):
    """the data-derived tags of a graph-to-kmer-set case that the builders above cannot know by plan (a dense graph's self-
    complementary edges): stated by realised() again, from the data"""
    return list(tags) + sorted(_g2k_data_tags(edges, K))


def _g2k_data_tags(edges, K):
    length = K + 1
    s = set(edges)
    t = set()
    if any(sm.revcomp(e, length) == e for e in edges):
        t.add("G.self-complementary")
    if any(sm.revcomp(e, length) not in s for e in edges):
        t.add("G.asymmetric")
    if length > 6:
        if 0 in s and (1 << (2 * length)) - 1 in s:
            t.add("G.homopolymers")
        if 2 * length > 64:
            lows, highs = {}, {}
            for e in edges:
                lows.setdefault(e & M64, set()).add(e >> 64)
                highs.setdefault(e >> 64, set()).add(e & M64)
            if any(len(v) > 1 for v in lows.values()):
                t.add("G.pair-differs-in-high-word-only")
            if any(len(v) > 1 for v in highs.values()):
                t.add("G.pair-differs-in-low-word-only")
    return t


# ---- emit_estimate -------------------------------------------------------------------------------------------------------------

def estimates(m, other):
    """[(label, M)]: every estimate a case is emitted with, none above 64 m; `other` = the count of a second input whose
    sum with m is what a merge passes"""
    out = [("m", m), ("m+1", m + 1), ("2m-1", 2 * m - 1), ("2m", 2 * m), ("2m+1", 2 * m + 1), ("4m", 4 * m), ("sum", m + other)]
    j = 1
    while 1 << j <= 64 * m:
        if m < 1 << j:
            out += [("2^%d-1" % j, (1 << j) - 1), ("2^%d" % j, 1 << j), ("2^%d+1" % j, (1 << j) + 1)]
        j += 1
    assert all(M <= 64 * m + 1 for _, M in out)
    return [(l, M) for l, M in out if M <= 64 * m]


def _estimate_cases():
    for K in (25, 40):
        yield "estimate_k%d" % K, (lambda K=K: Case("estimate_k%d" % K, "estimate", ["E.K=%d" % K, "E.two-words" if K > 31 else "E.one-word"],
                                                   K=K, keys=list(drawn_keys(2 * K, 5000, 71)), other=3500))


# ---- text ----------------------------------------------------------------------------------------------------------------------

DIGIT_COUNTS = [1, 9]
for _d in range(1, 10):
    DIGIT_COUNTS += [10 ** _d - 1, 10 ** _d] if _d > 1 else [10]
DIGIT_COUNTS = sorted(set(DIGIT_COUNTS)) + [U32 - 1, U32]          # 1, 9, 10, 99, 100, ..., 999 999 999, 10^9, 2^32 - 2, 2^32 - 1
LONG_COUNTS = [10 ** 9, U32 - 1, U32]                                # the ten-digit ones
LONG_AT = [0, 255, 256, 4095, 4096, -1]
SWEEP = 256 * 64 * 256                                               # bytes one sweep of dump_kmers_kernel's capped grid writes


def _text_cases():
    for length, m in ((1, 4), (2, 16), (31, 300), (32, 300), (33, 300), (63, 300), (63, 65535), (63, 65536), (63, 65537)):
        name = "dumpk_len%d_m%d" % (length, m)
        tags = ["T.kmers.len=%d" % length]
        body = m * (length + 1)
        if m > 300:
            tags.append("T.kmers.body%ssweep" % ("<" if body < SWEEP else "=" if body == SWEEP else ">"))
        yield name, (lambda name=name, length=length, m=m, tags=tags:
                     Case(name, "dumpk", tags, K=length, keys=list(drawn_keys(2 * length, m, 81))))

    def small(part):
        # K = 1: 16 edges, so the 21 counts take two cases
        counts = (DIGIT_COUNTS + DIGIT_COUNTS)[part * 8: part * 8 + 16]
        return Case("dumpe_len2_%d" % part, "dumpe", _dumpe_tags(counts, 1), K=1, edges=list(range(16)), counts=counts)
    yield "dumpe_len2_0", lambda: small(0)
    yield "dumpe_len2_1", lambda: small(1)
    for K in (31, 32, 62):
        def big(K=K):
            edges = list(drawn_keys(2 * K + 2, 5000, 82))
            counts = [DIGIT_COUNTS[i % (len(DIGIT_COUNTS) - 1)] for i in range(len(edges))]          # (2^32 - 1 only where planted: 256 keys hold it at the most)
            for j, at in enumerate(LONG_AT):
                counts[at] = LONG_COUNTS[(j + K) % 3]
            counts[100] = U32
            return Case("dumpe_len%d" % (K + 1), "dumpe", _dumpe_tags(counts, K), K=K, edges=edges, counts=counts)
        yield "dumpe_len%d" % (K + 1), big


def _dumpe_tags(counts, K):
    t = {"T.edges.len=%d" % (K + 1)}
    t |= {"T.count=%d" % c for c in set(counts) if c in DIGIT_COUNTS}
    for at in LONG_AT:
        if len(counts) > max(at, 0) + 1 and counts[at] >= 10 ** 9:
            t.add("T.long@%s" % ("last" if at < 0 else at))
    return sorted(t)


RANGED = ["dumpk_len31_m300", "dumpk_len63_m300", "dumpe_len2_0", "dumpe_len32", "dumpe_len63"]


def range_cuts(m):
    """the ascending cut points of a dump cut into pieces [c_j, c_j+1): 0, 1, m - 1, m, on and beside 256 and 4 096, a cut
    twice in the middle and m twice at the end (pieces of count 0, the last at first == m)"""
    mid = m // 2
    cuts = [0, 1] + [c for c in (255, 256, 257, 4095, 4096, 4097) if 1 < c < m - 1] + [mid, mid, m - 1, m, m]
    return sorted(cuts)


def cut_tags(m):
    cuts = range_cuts(m)
    pieces = list(zip(cuts, cuts[1:]))
    t = {"R.cut=%s" % c for c in cuts if c in (0, 1, 255, 256, 257, 4095, 4096, 4097)}
    t |= {"R.cut=m-1"} if m - 1 in cuts else set()
    t |= {"R.cut=m"} if m in cuts else set()
    if any(a == b and 0 < a < m for a, b in pieces):
        t.add("R.count=0-in-the-middle")
    if any(a == b == m for a, b in pieces):
        t.add("R.count=0-at-m")
    return t


# ---- lint ------------------------------------------------------------------------------------------------------------------------

LINT_KS = (3, 27, 31, 40)


def _lint_base(K, pairs, seed=0):
    """a symmetric graph of `pairs` strand pairs, no edge its own reverse complement, counts 1 .. 9 equal on both strands"""
    length = K + 1
    rng = random.Random(900 + K + seed)
    g = {}
    while len(g) < 2 * pairs:
        e = rng.getrandbits(2 * length)
        r = sm.revcomp(e, length)
        if e != r and e not in g:
            g[e] = g[r] = rng.randint(1, 9)
    edges = sorted(g)
    return edges, [g[e] for e in edges]


def _drop(edges, counts, victims, length):
    """the list without the reverse complements of edges[v]: each edges[v] becomes an edge without its partner"""
    gone = {sm.revcomp(edges[v], length) for v in victims}
    keep = [i for i, e in enumerate(edges) if e not in gone]
    return [edges[i] for i in keep], [counts[i] for i in keep]


def _lint_cases():
    for K in LINT_KS:
        length = K + 1
        pairs = 40 if K == 3 else 1200

        def base(K=K, pairs=pairs):
            return _lint_base(K, pairs)

        def mk(name, tags, build, K=K):
            full = "lint_k%d_%s" % (K, name)

            def make():
                e, c = build()
                return Case(full, "lint", ["L.K=%d" % K] + tags, K=K, edges=e, counts=c)
            return full, make

        yield mk("clean", ["L.clean"], base)

        def missing(where, base=base, length=length):
            e, c = base()
            n = len(e)
            # the victim keeps its place when its partner goes: the first edge's partner lies behind it, the last one's
            # in front of it; a middle one with its partner behind it
            v = {"0": 0, "end": n - 1}.get(where)
            if v is None:
                v = next(i for i in range(n // 2, n) if sm.revcomp(e[i], length) > e[i])
            return _drop(e, c, [v], length)
        yield mk("missing_at_0", ["L.missing@0"], lambda m=missing: m("0"))
        yield mk("missing_in_the_middle", ["L.missing@middle"], lambda m=missing: m("middle"))
        yield mk("missing_at_the_end", ["L.missing@end"], lambda m=missing: m("end"))

        def bump(base=base):
            e, c = base()
            c[len(e) // 3] += 1
            return e, c
        yield mk("count_mismatch", ["L.mismatch-pair"], bump)

        def zero(both, base=base, length=length):
            e, c = base()
            i = len(e) // 4
            c[i] = 0
            if both:
                c[e.index(sm.revcomp(e[i], length))] = 0
            return e, c
        yield mk("zero_on_both_strands", ["L.zero-both"], lambda z=zero: z(True))
        yield mk("zero_on_one_strand", ["L.zero-one"], lambda z=zero: z(False))

        if length % 2 == 0:
            def selfc(base=base, length=length):
                e, c = base()
                half = 0x1B1B1B1B1B1B1B1B & ((1 << length) - 1)
                s = (half << length) | sm.revcomp(half, length // 2)
                assert sm.revcomp(s, length) == s and s not in e
                g = dict(zip(e, c))
                g[s] = 7
                e = sorted(g)
                return e, [g[x] for x in e]
            yield mk("self_complementary", ["L.self-complementary", "L.clean"], selfc)

        def dup(how, base=base, length=length):
            # an edge twice (an equal neighbour): the second copy does not exceed its predecessor
            e, c = base()
            i = len(e) // 2
            e, c = e[:i + 1] + e[i:], c[:i + 1] + c[i:]
            if how == "mismatch":
                c[i + 1] += 1                                # ... and differs from its partner: kind 4 overwritten by 2
            if how == "zero":
                j = e.index(sm.revcomp(e[i], length))
                c[i] = c[i + 1] = c[j] = 0                   # ... and is zero like its partner: it stays kind 4, the others are kind 3
            return e, c
        yield mk("duplicate", ["L.duplicate"], lambda d=dup: d("plain"))
        yield mk("duplicate_mismatch", ["L.duplicate", "L.kind4-overwritten"], lambda d=dup: d("mismatch"))
        yield mk("duplicate_zero", ["L.duplicate", "L.zero-both", "L.kind4-kept-over-3"], lambda d=dup: d("zero"))

        if K == 3:
            continue
        for count in (33, 64, 1000):
            def many(count=count, base=base, length=length):
                e, c = base()
                fwd = [i for i in range(len(e)) if sm.revcomp(e[i], length) > e[i]]
                return _drop(e, c, fwd[:count], length)
            yield mk("missing_%d" % count, ["L.offenders=%d" % count, "L.one-kind"], many)

            def mixed(count=count, base=base, length=length):
                # a third of the offenders without a partner, the others in pairs: the counts differ, or both are zero
                e, c = base()
                fwd = [i for i in range(len(e)) if sm.revcomp(e[i], length) > e[i]]
                lone = count - count // 3 * 2
                e2, c2 = _drop(e, c, fwd[:lone], length)
                at = {x: i for i, x in enumerate(e2)}
                for n, i in enumerate(fwd[lone:lone + count // 3]):
                    a, b = at[e[i]], at[sm.revcomp(e[i], length)]
                    if n % 2:
                        c2[a] = c2[b] = 0
                    else:
                        c2[a] += 1
                return e2, c2
            yield mk("mixed_%d" % count, ["L.offenders=%d" % count, "L.mixed"] + (["L.zero-both"] if count // 3 >= 2 else []), mixed)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

_BUILDERS = dict(list(_select_cases()) + list(_window_cases()) + list(_algebra_cases()) + list(_bits_cases()) + list(_g2k_cases())
                 + list(_estimate_cases()) + list(_text_cases()) + list(_lint_cases()))
NAMES = list(_BUILDERS)


def names(kind):
    prefix = {"select": ("sel_", "win_"), "algebra": ("intersect_", "subtract_", "annotate_"), "bits": ("bits_",), "g2k": ("g2k_",),
              "estimate": ("estimate_",), "dumpk": ("dumpk_",), "dumpe": ("dumpe_",), "lint": ("lint_",)}[kind]
    return [n for n in NAMES if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c


def _window_vocab(lo, hi):
    """the window and the sides of its bounds that hold a count ((1, 1): the counts are 1, 2 and 3, none below)"""
    w = "W.%d..%d" % (lo, hi)
    return [w] + [w + s for s, ok in ((".lo-1", lo > 1), (".at-lo", True), (".at-hi", True), (".hi+1", hi < U32)) if ok]


CONDITIONS = (
    ["S.n=%d" % n for n in sorted(set(SEL_N) | set(SEL_N_THREE_TILES))] + ["S.K=%d" % k for k in (25, 31, 32, 63)]
    + ["S.keep=%s" % p for p in PATTERNS] + ["S.count=lo-kept", "S.count=hi-kept", "S.count=lo-1-dropped", "S.count=hi+1-dropped"]
    + _window_vocab(1, 1) + _window_vocab(2, 2) + _window_vocab(3, 3) + _window_vocab(6, 6) + _window_vocab(2, U32)
    + _window_vocab(U32, U32) + _window_vocab(0, 0)
    + ["W.counts-1-2-3", "W.zero-count", "W.twice", "W.runs=1", "W.runs=2", "W.runs=3", "W.runs=4", "W.runs=7"]
    + ["A.op=intersect", "A.op=subtract", "A.op=annotate", "A.K=25", "A.K=32", "A.K=63", "A.disjoint", "A.interleaved", "A.identical",
       "A.a-empty", "A.b-empty", "A.nested", "A.differ-first", "A.differ-last", "A.differ-key0", "A.differ-max", "A.differ-high-word", "A.differ-bit63",
       "A.differ-low-word", "A.same-set-3x", "A.one-empty-among-full", "A.all-empty", "A.undefined", "A.refused", "A.result-empty"]
    + ["B.m=%d" % m for m in BITS_M] + ["B.%s" % p for p in BITS_PATTERNS]
    + ["G.all-edges.K=%d" % K for K in range(1, 6)] + ["G.dense-corpus", "G.len=31", "G.len=32", "G.len=63", "G.homopolymers",
                                                       "G.self-complementary", "G.pair-differs-in-high-word-only",
                                                       "G.pair-differs-in-low-word-only", "G.asymmetric"]
    + ["E.K=25", "E.K=40", "E.one-word", "E.two-words"]
    + ["T.kmers.len=%d" % n for n in (1, 2, 31, 32, 33, 63)] + ["T.kmers.body<sweep", "T.kmers.body=sweep", "T.kmers.body>sweep"]
    + ["T.edges.len=%d" % n for n in (2, 32, 33, 63)] + ["T.count=%d" % c for c in DIGIT_COUNTS]
    + ["T.long@%s" % a for a in (0, 255, 256, 4095, 4096, "last")]
    + ["L.K=%d" % K for K in LINT_KS]
    + ["L.clean", "L.missing@0", "L.missing@middle", "L.missing@end", "L.mismatch-pair", "L.zero-both", "L.zero-one", "L.self-complementary",
       "L.duplicate", "L.kind4-overwritten", "L.kind4-kept-over-3", "L.offenders=33", "L.offenders=64", "L.offenders=1000", "L.one-kind",
       "L.mixed"])
RANGE_CONDITIONS = (["R.cut=%s" % c for c in (0, 1, 255, 256, 257, 4095, 4096, 4097, "m-1", "m")]
                    + ["R.count=0-in-the-middle", "R.count=0-at-m"])


# ---- the tags a case has, by its data --------------------------------------------------------------------------------------------

def realised(c):
    t = set()
    if c.kind == "select":
        keys, counts = sm.merged(c.runs)
        n = len(keys)
        t.add("S.K=%d" % c.K)
        lo, hi = c.windows[0]
        literal = len(c.runs) == 1 and isinstance(c.runs[0][1], list) and (lo, hi) == WINDOW
        if literal:                                      # a planned kept set
            t.add("S.n=%d" % n)
            kept = tuple(i for i, v in enumerate(counts) if lo <= v <= hi)
            for p in PATTERNS:
                if kept_of(p, n) == kept:
                    t.add("S.keep=%s" % p)
            vs = set(counts)
            t |= {tag for tag, v in (("S.count=lo-kept", lo), ("S.count=hi-kept", hi), ("S.count=lo-1-dropped", lo - 1),
                                     ("S.count=hi+1-dropped", hi + 1)) if v in vs}
        else:
            w = "W.%d..%d" % (lo, hi)
            vs = set(counts)
            t.add(w)
            t |= {w + s for s, v in ((".lo-1", lo - 1), (".at-lo", lo), (".at-hi", hi), (".hi+1", hi + 1)) if v in vs and 0 <= v <= U32}
            t.add("W.runs=%d" % len(c.runs))
            if {1, 2, 3} <= vs and (lo, hi) == (1, 1):
                t.add("W.counts-1-2-3")
            if (lo, hi) == (0, 0) and 0 in vs:
                t.add("W.zero-count")
            if len(c.windows) > 1:
                t.add("W.twice")
    elif c.kind == "algebra":
        t |= {"A.op=%s" % c.op, "A.K=%d" % c.K}
        sets = [list(s) for s in c.sets]
        top = (1 << (2 * c.K)) - 1
        if all(not s for s in sets):
            t.add("A.all-empty")
        elif len(sets) == 3 and sets[0] == sets[1] == sets[2]:
            t.add("A.same-set-3x")
        elif len(sets) > 2 and any(not s for s in sets) and sum(1 for s in sets if s) >= 2:
            t.add("A.one-empty-among-full")
        elif len(sets) == 2:
            a, b = sets
            sa, sb = set(a), set(b)
            diff = sa ^ sb
            if not b:
                t.add("A.b-empty")
            elif not a:
                t.add("A.a-empty")
            elif a == b:
                t.add("A.identical")
            else:
                if not sa & sb:
                    t.add("A.disjoint")
                    u = sorted(sa | sb)
                    if all((x in sa) != (y in sa) for x, y in zip(u, u[1:])):
                        t.add("A.interleaved")
                if sb < sa:
                    t.add("A.nested")
                if len(a) == len(b) and a[1:] == b[1:]:
                    t.add("A.differ-first")
                if len(a) == len(b) and a[:-1] == b[:-1]:
                    t.add("A.differ-last")
                if diff == {0}:
                    t.add("A.differ-key0")
                if diff == {top}:
                    t.add("A.differ-max")
                if len(diff) == 2 and c.K >= 32:
                    x, y = sorted(diff)
                    if x & M64 == y & M64:
                        t.add("A.differ-high-word")
                    elif x ^ y == 1 << 63:
                        t.add("A.differ-bit63")
                    elif x >> 64 == y >> 64:
                        t.add("A.differ-low-word")
        try:
            if not _algebra_result(c.op, sets):
                t.add("A.result-empty")
        except sm.Refused:
            t.add("A.refused")
        except sm.Undefined:
            t.add("A.undefined")
    elif c.kind == "bits":
        m = len(c.keys)
        t.add("B.m=%d" % m)
        for p in BITS_PATTERNS:
            if bits_counts(p, m) == tuple(c.counts):
                t.add("B.%s" % p)
    elif c.kind == "g2k":
        n = len(c.edges)
        if c.K <= 5:
            if c.edges == list(range(1 << (2 * c.K + 2))):
                t.add("G.all-edges.K=%d" % c.K)
            else:
                t.add("G.dense-corpus")
        else:
            t.add("G.len=%d" % (c.K + 1))
        assert n
        t |= _g2k_data_tags(c.edges, c.K)
    elif c.kind == "estimate":
        t |= {"E.K=%d" % c.K, "E.two-words" if words_of(c.K) == 2 else "E.one-word"}
    elif c.kind == "dumpk":
        t.add("T.kmers.len=%d" % c.K)
        body = len(c.keys) * (c.K + 1)
        if abs(body - SWEEP) <= c.K + 1:
            t.add("T.kmers.body%ssweep" % ("<" if body < SWEEP else "=" if body == SWEEP else ">"))
    elif c.kind == "dumpe":
        t |= set(_dumpe_tags(c.counts, c.K))
    elif c.kind == "lint":
        t.add("L.K=%d" % c.K)
        length = c.K + 1
        n = len(c.edges)
        tot, off = sm.lint(c.edges, c.counts, c.K, False)
        atot, aoff = sm.lint(c.edges, c.counts, c.K, True)
        if not off and not aoff:
            t.add("L.clean")
        miss = sorted(i for i, k, o in off if k == sm.MISSING)
        if len(off) >= 33:
            t.add("L.offenders=%d" % len(off))
            t.add("L.one-kind" if len({k for _, k, _ in off}) == 1 else "L.mixed")
        elif len(miss) == 1:
            t.add("L.missing@%s" % ("0" if miss[0] == 0 else "end" if miss[0] == n - 1 else "middle"))
        if tot["count_mismatch"] == 2 and not tot["zero_count"] and not tot["order_violation"] and len(off) == 2:
            t.add("L.mismatch-pair")
        at = {}
        for i, e in enumerate(c.edges):
            at.setdefault(e, i)
        for i, e in enumerate(c.edges):
            j = at.get(sm.revcomp(e, length))
            if c.counts[i] == 0 and j is not None:
                t.add("L.zero-both" if c.counts[j] == 0 else "L.zero-one")
            if j == i:
                t.add("L.self-complementary")
        if tot["order_violation"]:
            t.add("L.duplicate")
            fours = sum(1 for _, k, _ in off if k == sm.ORDER)
            if fours < tot["order_violation"]:
                t.add("L.kind4-overwritten")
            if any(k == sm.ORDER and c.counts[i] == 0 for i, k, _ in off):
                t.add("L.kind4-kept-over-3")
    return t


# ---- what the tests share ------------------------------------------------------------------------------------------------------

def strip(files, base):
    return {n[len(base):]: b for n, b in files.items()}


def first_difference(got, exp):
    """None, or which file differs first and where"""
    if sorted(got) != sorted(exp):
        return "file names differ: %s vs %s" % (sorted(got), sorted(exp))
    for name in sorted(exp):
        a, b = got[name], exp[name]
        if a != b:
            n = min(len(a), len(b))
            off = next((i for i in range(n) if a[i] != b[i]), n)
            return "%s: %d vs %d bytes, first difference at offset %d: %s vs %s" % (name, len(a), len(b), off, a[off:off + 8].hex(),
                                                                                   b[off:off + 8].hex())
    return None


def kmer_set_files(oracle, keys, K, M=None):
    return strip(oracle.write_kmer_set(keys, K, M=M, out="ks"), "ks")


@functools.lru_cache(maxsize=None)
def algebra_expected(oracle, name):
    """what the oracle's command writes for an algebra case: ({suffix: bytes}, stats or None) -- or the exception it refuses
    with, returned, not raised"""
    c = case(name)
    files = {}
    names = []
    for i, s in enumerate(c.sets):
        files.update(oracle.write_kmer_set(s, c.K, out="in%d" % i))
        names.append("in%d" % i)
    try:
        if c.op == "intersect":
            return strip(oracle.intersect_kmer_sets(files, names, "out"), "out"), None
        if c.op == "subtract":
            return strip(oracle.subtract_kmer_set(files, names[0], names[1], "out"), "out"), None
        f, stats = oracle.merge_and_annotate(files, names[0], names[1], "out")
        return strip(f, "out"), stats
    except oracle.OracleError as e:
        return e, None


@functools.lru_cache(maxsize=None)
def g2k_expected(oracle, name):
    c = case(name)
    files = oracle.write_graph(c.edges, [1] * len(c.edges), c.K, out="gr")
    return strip(oracle.graph_to_kmer_set(files, "gr", "out"), "out")


def host_keys(keys, words):
    """the keys as goss_gpu_push_run_host takes them: a numpy array of `words` u64 per key"""
    import numpy as np
    if words == 1:
        return np.array(keys, dtype=np.uint64)
    return np.array([[k & M64, k >> 64] for k in keys], dtype=np.uint64).reshape(-1)


def host_counts(w, n):
    import numpy as np
    return np.array(w if isinstance(w, (list, tuple)) else [w] * n, dtype=np.uint32)
