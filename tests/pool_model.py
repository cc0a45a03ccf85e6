"""pool-samples over Python integers and sets (GossCmdPoolSamples.cc): the union's order, the samples' sizes, the common
k-mers of every pair, the positions i * z + r of the <out>-index SparseArray and the <out>.sim text.  Nothing here calls
the library; the text goes through gossamer_amd.format_double, the restatement of a C++ ostream's default formatting.

A *planned* case is z sorted keys and one S-bit mask per key (bit i: the key is in sample i): the rows, sizes and common
counts are then known by construction -- planned_* computes them from the masks alone, the set functions from the
samples as sets of keys -- and the two must agree (test_pool_cpu.py)."""
from gossamer_amd.binding import format_double


# ---- from samples as collections of keys --------------------------------------------------------------------------------

def union_order(samples):
    """the keys of the union in rank order"""
    u = set()
    for s in samples:
        u.update(s)
    return sorted(u)


def sizes(samples):
    return [len(set(s)) for s in samples]


def intersections(samples):
    """inter[i][j] = common k-mers of samples i and j: symmetric, the diagonal the sizes"""
    sets = [set(s) for s in samples]
    n = len(sets)
    out = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            out[i][j] = out[j][i] = len(sets[i] & sets[j])
    return out


def positions(samples):
    """for sample i in order, i * z + r for every k-mer of the sample at rank r of the union: strictly increasing"""
    order = union_order(samples)
    rank = {k: r for r, k in enumerate(order)}
    z = len(order)
    out = []
    for i, s in enumerate(samples):
        out.extend(i * z + r for r in sorted(rank[k] for k in set(s)))
    return out


def index_shape(samples):
    """(N, M, N_end) of SparseArray::Builder(name, fac, N = z * S, M = m) ... end(N)"""
    z, m = len(union_order(samples)), sum(sizes(samples))
    return z * len(samples), m, z * len(samples)


def sim_text(inter, size):
    """one line i '\\t' j '\\t' sim '\\n' per pair i < j, sim = double(inter) / double(|i| + |j| - inter)"""
    out = []
    n = len(size)
    for i in range(n):
        for j in range(i + 1, n):
            out.append("%d\t%d\t%s\n" % (i, j, format_double(float(inter[i][j]) / float(size[i] + size[j] - inter[i][j]))))
    return "".join(out)


# ---- planned cases: from the masks alone ------------------------------------------------------------------------------

def planned_samples(keys, masks, nsets):
    """the samples of a planned case as lists of keys"""
    return [[k for k, m in zip(keys, masks) if (m >> i) & 1] for i in range(nsets)]


def planned_sizes(masks, nsets):
    return [sum((m >> i) & 1 for m in masks) for i in range(nsets)]


def planned_rows(masks, nsets):
    """row i as one Python integer: bit r set when k-mer r is in sample i"""
    rows = [0] * nsets
    for r, m in enumerate(masks):
        i = 0
        while m:
            if m & 1:
                rows[i] |= 1 << r
            m >>= 1
            i += 1
    return rows


def planned_intersections(masks, nsets):
    rows = planned_rows(masks, nsets)
    return [[bin(rows[i] & rows[j]).count("1") for j in range(nsets)] for i in range(nsets)]


def planned_positions(masks, nsets):
    """the positions when every one of the z keys counts as a union k-mer (the library is told z; a key in no sample
    still takes a rank)"""
    z = len(masks)
    return [i * z + r for i in range(nsets) for r, m in enumerate(masks) if (m >> i) & 1]


def slab_masks(masks, first, nbits, junk=0):
    """what goss_gpu_pool_add_masks is handed for samples first ... first + nbits - 1: their bits at 0 ... nbits - 1,
    and `junk` ORed in above them (the union's weight of the command's slabs: to be ignored)"""
    keep = (1 << nbits) - 1
    top = (junk << nbits) & 0xFFFFFFFF
    return [((m >> first) & keep) | top for m in masks]
