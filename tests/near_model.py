"""compute-near-kmers over Python integers: the loop of GossCmdComputeNearKmers.cc:58-121 as it stands, plus the two
flags the library offers for what that loop was probably meant to do.

keys: the set's k-mers, sorted (rank = index); lhs, rhs: one bit (0 / 1) per rank.  Per rank i with lhs[i] != rhs[i],
x = keys[i]; for j = 0 .. K-1 and b = 0 .. 3, y = x ^ (b << j) (whole_bases: b << 2j), y == x skipped; i is gray when
some y is in the set at a rank r with lhs[r] != rhs[r] and lhs[r] != lhs[i].  y is looked up as it is, the reference
discards what its normalize returns (GraphEssentials.hh:152-157); normalize=True looks its canonical form up instead.
A gray rank gets both new bits 0; only old bits are read."""
import oracle_lib as o


def reference_masks(K, whole_bases=False):
    """the 3K masks in the order the reference's two loops produce them (duplicates included)"""
    return [b << ((2 * j) if whole_bases else j) for j in range(K) for b in range(1, 4)]


def distinct_masks(K, whole_bases=False):
    """what the kernel walks: for the reference's shift by bits the K + 1 single bits 0 .. K and the K pairs 3 << j"""
    if whole_bases:
        return reference_masks(K, True)
    return [1 << t for t in range(K + 1)] + [3 << j for j in range(K)]


def near_kmers(keys, lhs, rhs, K, whole_bases=False, normalize=False, masks=None):
    """-> (new lhs bits, new rhs bits, gray count)"""
    if masks is None:
        masks = reference_masks(K, whole_bases)
    rank = {x: i for i, x in enumerate(keys)}
    assert len(rank) == len(keys) == len(lhs) == len(rhs)
    new_l, new_r, gray = list(lhs), list(rhs), 0
    for i, x in enumerate(keys):
        if lhs[i] == rhs[i]:
            continue
        for m in masks:
            y = x ^ m
            if y == x:
                continue
            if normalize:
                y = o.normalize(y, K)
            r = rank.get(y)
            if r is not None and lhs[r] != rhs[r] and lhs[r] != lhs[i]:
                new_l[i] = new_r[i] = 0
                gray += 1
                break
    return new_l, new_r, gray


def pack_bits(bits):
    """WordyBitVector words after len(bits) push_backX calls and end(): (n - 1) // 64 + 1 little-endian u64 words, one
    zero word for no bits (WordyBitVector.hh:90-116) -- the .lhs-bits / .rhs-bits files"""
    n = len(bits)
    words = [0] * ((n - 1) // 64 + 1 if n else 1)
    for i, b in enumerate(bits):
        if b:
            words[i >> 6] |= 1 << (i & 63)
    return words


def unpack_bits(words, n):
    return [(words[i >> 6] >> (i & 63)) & 1 for i in range(n)]


def words_to_bytes(words):
    return b"".join(int(w).to_bytes(8, "little") for w in words)


def bytes_to_words(data):
    assert len(data) % 8 == 0
    return [int.from_bytes(data[i:i + 8], "little") for i in range(0, len(data), 8)]
