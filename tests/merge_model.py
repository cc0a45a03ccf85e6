"""What merge_runs must compute, stated without a device: sorted (key, count) runs in, one run out.

`merge` is the model: a dict of big integers.  The rest of the module builds the inputs the merge tests
push -- runs laid out for one path of the merge and one of its limits -- and asserts the property a test
asks for on its own output, in Python, before anything reaches a device.

A segment is the top `segbits` bits of a key of `bits` = 2 * length bits (merge_runs starts at 8 bits for
totals of at most 2^18 entries and retries at 10 and 12); an entry is one (key, count) of one run, so a key
held by 64 runs is 64 entries of its segment.
"""
import collections
import random

U32 = 0xFFFFFFFF          # the largest stored count -- as an input count it is the number 4 294 967 295
GRAPH, KMER = "graph", "kmer"

MERGE_CAP = 2048          # kMergeCap: entries of one segment the segment merge takes
MERGE_RUNS = 64           # kMergeRuns
SEG_MERGE_MIN = 1024      # smallest total the segment merge takes
MAX_BIG = 256             # kMaxBig: keys at or above 2^32 - 1 a graph result may hold
TABLE_LOCK = 1 << 31      # the table merge's slot word: a count that reaches it sends the merge elsewhere

Merged = collections.namedtuple("Merged", "keys exact u32 big")


def merge(runs, mode):
    """runs: lists of (key, count), keys strictly increasing inside a run, 1 <= count <= 2^32 - 1."""
    assert mode in (GRAPH, KMER)
    total = {}
    for run in runs:
        last = -1
        for key, count in run:
            assert key > last, "a run's keys must be strictly increasing"
            assert 1 <= count <= U32, "not a multiplicity: %r" % (count,)
            last = key
            total[key] = total.get(key, 0) + count
    keys = sorted(total)
    exact = [total[k] for k in keys]
    if mode == GRAPH:
        u32 = [e & U32 for e in exact]
        big = {k: e for k, e in zip(keys, exact) if e >= U32}
    else:
        u32 = [min(e, U32) for e in exact]
        big = {}
    return Merged(keys, exact, u32, big)


# ---- geometry -------------------------------------------------------------------------------------------------------
def key_bits(k, mode):
    """bits of a key: a k-mer set holds k-mers, a graph holds edges of k + 1 bases"""
    return 2 * (k + (1 if mode == GRAPH else 0))


def key_words(bits):
    return 1 if bits <= 62 else 2


def segment(key, bits, segbits=8):
    return key >> (bits - segbits)


def segment_totals(runs, bits, segbits=8):
    """entries per segment over all runs"""
    tot = collections.Counter()
    for run in runs:
        for key, _ in run:
            tot[segment(key, bits, segbits)] += 1
    return tot


def total_entries(runs):
    return sum(len(r) for r in runs)


# ---- case builder ---------------------------------------------------------------------------------------------------
EMPTY_SEG = 0x55          # no key of any run
QUIET_SEG = 0x33          # populated, but run 0 holds nothing of it
DENSE_SEG = 0xA7          # where a `dense` layout puts its entries (nothing else goes there then)

Case = collections.namedtuple("Case", "runs bits placed pairs tie_key")


def build_case(bits, nruns, total, seed, dense=None, sums=(), disjoint=False, fill_count=None):
    """`nruns` runs with `total` entries in all, keys of `bits` bits.

    Every case holds key 0 and key 2^bits - 1; for two-word keys, pairs that differ only in the high word, only in
    the low word, and the adjacent pair (hi, 2^64 - 1) / (hi + 1, 0) -- both members in one segment where the
    length allows (at exactly 64 bits the high word is 0 and only the low-word pairs exist); a key present in every
    run; an empty segment; a populated segment run 0 holds nothing of.  The rest is random.

    dense  = ("cluster", n): n entries in DENSE_SEG whose keys share every bit above their low 12 -- one segment at
             8, 10 and 12 bits alike;  ("spread", n): n entries in DENSE_SEG spread evenly over its four 10-bit
             sub-prefixes.  Spread over the runs evenly; nothing else enters that segment.
    sums   = [(label, [part, part, ..])]: a fresh key per label whose counts in len(parts) distinct runs are the
             parts; `placed[label]` is the key.
    disjoint: no key in more than one run (and so no key in every run).
    fill_count: count of an ordinary entry (default: small, now and then up to 2^20).
    """
    rng = random.Random(seed)
    assert bits >= 8 and nruns >= 1
    top = (1 << bits) - 1
    reserved = {EMPTY_SEG} | ({DENSE_SEG} if dense else set())
    runs = [dict() for _ in range(nruns)]

    def ordinary():
        if fill_count is not None:
            return fill_count(rng)
        return rng.randint(1, 1 << 20) if rng.random() < 0.1 else rng.randint(1, 60)

    def allowed(key, special=True):
        s = segment(key, bits)
        return s not in reserved and not (special and s == QUIET_SEG)

    def holders(n):
        return rng.sample(range(nruns), max(1, min(n, nruns)))

    def put(key, where):
        if disjoint:
            if any(key in r for r in runs):
                return
            where = where[:1]
        for r in where:
            runs[r].setdefault(key, ordinary())

    # the ends of the key space
    put(0, holders(3))
    put(top, holders(3))
    # a key in every run: ties in every sub-run of its segment
    tie_key = None
    if not disjoint:
        while tie_key is None or not allowed(tie_key):
            tie_key = rng.getrandbits(bits)
        put(tie_key, list(range(nruns)))
    # comparisons across the word boundary
    pairs = []
    if bits >= 64:
        hb = bits - 64          # (0 at 64 bits: the high word is always 0, only the low word can differ)
        lo_free = 64 - max(0, 8 - hb)          # low-word bits below the segment prefix

        def pair(make):
            for _ in range(10000):
                a, b = make()
                if a != b and a <= top and b <= top and allowed(a) and allowed(b):
                    return a, b
            raise AssertionError("no such pair at %d bits" % bits)

        def high_only():
            h, lo = rng.getrandbits(hb), rng.getrandbits(64)
            h2 = h ^ (1 << rng.randrange(max(1, hb - 8)))
            return (h << 64) | lo, (h2 << 64) | lo

        def low_only(bit):
            def make():
                h, lo = rng.getrandbits(hb), rng.getrandbits(64)
                return (h << 64) | lo, (h << 64) | (lo ^ (1 << bit))
            return make

        def adjacent():
            h = rng.getrandbits(hb) & ~1
            return (h << 64) | ((1 << 64) - 1), (h + 1) << 64

        for make in (high_only, low_only(0), low_only(lo_free - 1), adjacent) if hb else (low_only(0), low_only(lo_free - 1)):
            a, b = pair(make)
            pairs.append((a, b))
            common = holders(1)
            put(a, common + holders(2))
            put(b, common + holders(2))
    # counts placed on purpose
    placed = {}
    for label, parts in sums:
        assert 1 <= len(parts) <= nruns and not (disjoint and len(parts) > 1), label
        key = None
        while key is None or not allowed(key) or any(key in r for r in runs):
            key = rng.getrandbits(bits)
        for r, part in zip(rng.sample(range(nruns), len(parts)), parts):
            runs[r][key] = part
        placed[label] = key
    # the dense segment
    if dense:
        kind, n = dense
        assert bits >= 26, "a dense layout needs room below a 14-bit prefix"
        prefix = DENSE_SEG << (bits - 8)
        if kind == "cluster":
            prefix |= (rng.getrandbits(bits - 8 - 12) << 12) if bits > 20 else 0
        per = [n // nruns + (1 if r < n % nruns else 0) for r in range(nruns)]
        for r in range(nruns):
            if kind == "cluster":
                assert per[r] <= 4096
                lows = rng.sample(range(4096), per[r])
                keys = [prefix | lo for lo in lows]
            else:
                keys = set()
                i = r          # (the runs start at different sub-prefixes: a remainder entry does not pile up on one)
                while len(keys) < per[r]:
                    key = prefix | ((i % 4) << (bits - 10)) | rng.getrandbits(bits - 10)
                    if key not in keys:
                        keys.add(key)
                        i += 1
            for key in keys:
                runs[r][key] = ordinary()
    # a segment that run 0 stays out of
    quiet = (QUIET_SEG << (bits - 8)) | rng.getrandbits(bits - 8)
    if not any(quiet in r for r in runs):
        runs[nruns - 1 if nruns > 1 else 0][quiet] = ordinary()
    # the rest at random, up to the total asked for
    have = sum(len(r) for r in runs)
    assert have <= total, "the fixed part alone is %d entries, %d asked for" % (have, total)
    tries = 0
    while have < total:
        tries += 1
        assert tries < 200 * total + 100000, "key space too small for %d entries in %d runs" % (total, nruns)
        key = rng.getrandbits(bits)
        r = rng.randrange(nruns)
        if not allowed(key, special=False) or key in runs[r]:
            continue
        if segment(key, bits) == QUIET_SEG and r == 0 and nruns > 1:
            continue
        if disjoint and any(key in q for q in runs):
            continue
        runs[r][key] = ordinary()
        have += 1
    out = [sorted(r.items()) for r in runs]

    # what was promised
    assert total_entries(out) == total
    seen = set().union(*[set(r) for r in runs])
    assert 0 in seen and top in seen
    assert max(seen) <= top
    segs = segment_totals(out, bits)
    assert EMPTY_SEG not in segs
    if nruns > 1:
        assert segs[QUIET_SEG] >= 1 and all(segment(k, bits) != QUIET_SEG for k, _ in out[0])
    if disjoint:
        assert sum(len(r) for r in runs) == len(seen)
    else:
        assert all(tie_key in r for r in runs)
    if dense:
        assert segs[DENSE_SEG] == dense[1]
        assert max(v for s, v in segs.items() if s != DENSE_SEG) <= MERGE_CAP
    else:
        assert max(segs.values()) <= MERGE_CAP
    for label, parts in sums:
        assert sum(r[placed[label]] for r in runs if placed[label] in r) == sum(parts)
    return Case(out, bits, placed, pairs, tie_key)


# ---- the sums the count tests place -----------------------------------------------------------------------------------
def split(total, n):
    """`total` as n nearly equal positive parts"""
    assert total >= n
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def count_sums(nruns):
    """(label, parts) of every placed sum of the count cases that fits `nruns` runs; the expected `exact` is
    sum(parts), and the model says what the device must store for it."""
    n = min(nruns, MERGE_RUNS)
    sums = [
        ("2^32-2", [U32 - 2, 1]),                       # the largest count that is not kept beside the run
        ("2^32-2 in %d parts" % n, split(U32 - 1, n)),
        ("2^32-1 as 2 + (2^32-3)", [2, U32 - 2]),
        ("2^32-1 in %d parts" % n, split(U32, n)),
        ("2^32", [U32 - 6, 7]),
        ("2^32 as halves", [1 << 31, 1 << 31]),
        ("2^32+1", [U32 - 1, 3]),
        ("2^33-2", [U32, U32]),                         # two stored counts of 2^32 - 1
        ("literal 2^32-1 alone", [U32]),                # a stored count that IS 2^32 - 1, its key in no other run
        ("literal 2^32-1 plus 1", [U32, 1]),
    ]
    if nruns >= MERGE_RUNS:
        sums.append(("64 x (2^32-2)", [U32 - 1] * MERGE_RUNS))
    return sums
