"""What the commands on either side of a build must compute, stated over Python integers: the set algebra of
intersect-kmer-sets / subtract-kmer-set / merge-and-annotate-kmer-sets (the count windows of goss_gpu_select_counts over
weighted runs), the membership bitmaps (goss_gpu_emit_count_bits), graph-to-kmer-set (goss_gpu_select_normal), the text
forms (goss_gpu_emit_dump / _range) and lint-graph's first pass (goss_gpu_lint).  No device, no oracle: plain `set` /
`dict` arithmetic and format strings.  tests/setops_edges.py builds the corpus these are run over.

Every rule stands beside the line of the reference it comes from, as gossamer_amd/host/GossMerge.cpp cites them.
"""
import bisect

U32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
NONE = M64                       # `other` of an edge whose reverse complement is not in the list (~0)

KMER_SET_VERSION = 2011101701    # GossCmdDumpKmerSet.cc:44, the version line of goss_gpu_emit_dump_range
GRAPH_VERSION = 2011101014       # GossCmdDumpGraph.cc:50
KMERS, EDGES = 0, 1


class Undefined(Exception):
    """the reference has no answer (it dereferences an empty vector)"""


class Refused(Exception):
    """the reference throws"""


# ---- weighted runs and count windows ---------------------------------------------------------------------------------

def merged(runs):
    """runs: [(keys, weight or list of counts)] -> (sorted keys, their summed counts as a k-mer-set context holds them:
    32 bits, saturating at 2^32 - 1).  A count of 0 is a number like any other."""
    total = {}
    for keys, w in runs:
        ws = w if isinstance(w, (list, tuple)) else [w] * len(keys)
        for k, c in zip(keys, ws):
            total[k] = total.get(k, 0) + c
    keys = sorted(total)
    return keys, [min(total[k], U32) for k in keys]


def select(keys, counts, lo, hi):
    """goss_gpu_select_counts: the items with lo <= count <= hi, order kept, counts kept"""
    kept = [(k, c) for k, c in zip(keys, counts) if lo <= c <= hi]
    return [k for k, _ in kept], [c for _, c in kept]


# ---- the set algebra --------------------------------------------------------------------------------------------------

def intersect(sets):
    """intersect-kmer-sets: the k-mers of every non-empty input, sorted."""
    live = [set(s) for s in sets if len(s)]          # an invalid (empty) iterator is not kept among the sets: GossCmdIntersectKmerSets.cc:38-41
    if not live:                                     # every input empty: the visiting loop reads element 0 of an empty vector (:47-50)
        raise Undefined("every input k-mer set is empty")
    return sorted(set.intersection(*live))


def subtract(a, b):
    """subtract-kmer-set: the k-mers of a that b does not hold (GossCmdSubtractKmerSet.cc:47-66); either may be empty."""
    return sorted(set(a) - set(b))


def annotate(a, b):
    """merge-and-annotate-kmer-sets -> (sorted union, lhs words, rhs words, (|a|, |b|, common))"""
    if not len(a) or not len(b):                     # "nonsense": GossCmdMergeAndAnnotateKmerSets.cc:40-43
        raise Refused("nonsense")
    sa, sb = set(a), set(b)
    union = sorted(sa | sb)
    return (union, wordy_bits([k in sa for k in union]), wordy_bits([k in sb for k in union]),
            (len(sa), len(sb), len(sa & sb)))         # the line on stdout, :204


def as_windows(op, sets):
    """How the commands compose an operation from weighted runs and one count window:
    -> ([(keys, weight)] of the runs pushed, (lo, hi) or None).  An empty set pushes no run."""
    if op == "intersect":
        live = [s for s in sets if len(s)]
        s = len(live) or 1
        return [(x, 1) for x in live], (s, s)        # weight 1 each, kept where the count is the number of sets
    a, b = sets
    runs = [(x, w) for x, w in ((a, 1), (b, 2)) if len(x)]
    return runs, ((1, 1) if op == "subtract" else None)          # lhs 1, rhs 2: count 1 = lhs only; annotate keeps all


def wordy_bits(flags):
    """The words of a WordyBitVector after one push_backX per flag and end(): (m - 1) // 64 + 1 of them, one zero word
    when nothing was pushed (WordyBitVector.hh:90-116), bit b of word w = item 64 w + b, nothing set behind item m - 1."""
    m = len(flags)
    words = [0] * ((m - 1) // 64 + 1 if m else 1)
    for i, f in enumerate(flags):
        if f:
            words[i >> 6] |= 1 << (i & 63)
    return words


def words_bytes(words):
    return b"".join(w.to_bytes(8, "little") for w in words)


def count_bits(counts, mask):
    """goss_gpu_emit_count_bits: bit i = (counts[i] & mask) != 0"""
    return wordy_bits([(c & mask) != 0 for c in counts])


# ---- graph-to-kmer-set ------------------------------------------------------------------------------------------------

def revcomp(x, length):
    r = 0
    for _ in range(length):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def fnv(x):
    """FNV-1a over the 16 bytes of the key, least significant first (BigInteger.hh:528-536, 572-582)"""
    h = 14695981039346656037
    for i in range(16):
        h = ((h ^ ((x >> (8 * i)) & 0xFF)) * 1099511628211) & M64
    return h


def normal_edges(edges, K, normalize=None):
    """the edges that are their own canonical form; normalize: oracle_lib.normalize (edge_type::isNormal,
    RankSelect.hh:117-124, is position_type::normalize(e) == e)"""
    if normalize is None:
        from oracle_lib import normalize
    return [e for e in edges if normalize(e, K + 1) == e]


def normal_edges_by_pairs(edges, K):
    """The same rule without normalize: an edge and its reverse complement form a pair.  A pair of two distinct edges
    keeps exactly one, the one with the smaller hash (the smaller value where the hashes tie); an edge that is its own
    reverse complement is kept.  Whether the partner is in the list does not matter."""
    out = []
    for e in edges:
        r = revcomp(e, K + 1)
        if r == e:
            out.append(e)
            continue
        keep = min((e, r), key=lambda x: (fnv(x), x))
        assert keep in (e, r)
        if keep == e:
            out.append(e)
    return out


# ---- text -------------------------------------------------------------------------------------------------------------

def text_of(x, length):
    return "".join("ACGT"[(x >> (2 * (length - 1 - i))) & 3] for i in range(length))


def dump_piece(keys, counts, K, kind, flags, first, count):
    """The text goss_gpu_emit_dump_range gives for elements [first, first + count): the two header lines in front of the
    piece that starts at 0 and of no other, then one line per element."""
    m = len(keys)
    assert first <= m and count <= m - first
    out = []
    if first == 0:
        if kind == KMERS:
            out.append("#%d\n%d\t%d\n" % (KMER_SET_VERSION, K, m))                       # GossCmdDumpKmerSet.cc:44-45
        else:
            out.append("#%d\n%d\t%d\t%d\n" % (GRAPH_VERSION, K, m, flags))               # GossCmdDumpGraph.cc:50-51
    for i in range(first, first + count):
        if kind == KMERS:
            out.append("%s\n" % text_of(keys[i], K))                                     # GossCmdDumpKmerSet.cc:47-53
        else:
            out.append("%s\t%d\n" % (text_of(keys[i], K + 1), counts[i]))                # GossCmdDumpGraph.cc:53-61
    return "".join(out).encode()


def dump_text(keys, counts, K, kind, flags=0):
    return dump_piece(keys, counts, K, kind, flags, 0, len(keys))


# ---- lint-graph, pass 1 -------------------------------------------------------------------------------------------------

MISSING, MISMATCH, ZERO, ORDER = 1, 2, 3, 4


def lint(edges, counts, K, asymmetric):
    """-> ({"missing_rc", "count_mismatch", "zero_count", "order_violation"}, {(index, kind, other)})
    over a list that is at least non-decreasing (an equal neighbour is the order violation; in a list that goes down the
    search for the reverse complement has no defined answer).  `other`: the first index that holds the reverse complement,
    NONE where there is none.  An edge is an offender once, under the kind the kernel documents: 4 where it does not
    exceed its predecessor, overwritten by 1 (no reverse complement) or 2 (the multiplicities differ; asymmetric: both
    are zero); 3 (a zero multiplicity, symmetric graphs only, and only where the reverse complement exists) only where
    no other kind applies.  GossCmdLintGraph.cc:131-199."""
    tot = {"missing_rc": 0, "count_mismatch": 0, "zero_count": 0, "order_violation": 0}
    off = set()
    for i, (e, c) in enumerate(zip(edges, counts)):
        kind, other = 0, NONE
        if i > 0 and not edges[i - 1] < e:
            tot["order_violation"] += 1
            kind = ORDER
        r = revcomp(e, K + 1)
        j = bisect.bisect_left(edges, r)
        if j >= len(edges) or edges[j] != r:
            tot["missing_rc"] += 1
            kind = MISSING
        else:
            other = j
            cp = counts[j]
            if asymmetric:
                if c == 0 and cp == 0:
                    tot["count_mismatch"] += 1
                    kind = MISMATCH
            else:
                if c != cp:
                    tot["count_mismatch"] += 1
                    kind = MISMATCH
                if c == 0:
                    tot["zero_count"] += 1
                    if not kind:
                        kind = ZERO
        if kind:
            off.add((i, kind, other))
    return tot, off
