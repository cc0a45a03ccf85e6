"""The batched queries (kernels_query.hpp) at the limits of the key widths: graphs at K = 30 (nodes and edges in one
word), 31 (nodes in one word, edges in two: query_node_ranks_kernel<Key1, Key2>) and 62 (both in two, the top of the
high word live); k-mer sets at K = 31, 32 and 63 (62, 64 and 126 bits) with and without normalize; and K = 1 .. 5
exhaustively, every key and every node.  Objects are written with the oracle and opened with Object.open; expected
answers come from test_gpu_query's numpy helpers and, beside them, from Python ints and bisect."""
import bisect
import random

import numpy as np
import pytest

import dense_graphs as dg
import gossamer_amd as g
import tips_cases
from test_gpu_query import _check_node_ranks, _check_normalize, check_rank_select, to_keys

pytestmark = pytest.mark.gpu


def u64(a):
    return np.asarray(a).astype(np.uint64).tolist()


def all_t(n):
    return 4 ** n - 1


# ---- graphs at K = 30, 31, 62 --------------------------------------------------------------------------------------

def wide_graph(oracle, K):
    """tips_cases.combined_graph(K) and three planted edge pairs, so that the nodes at the limits have edges:
    T..T -> T with its reverse complement, which is A..A -> A; T..T -> G with its reverse complement C -> A..A; and the
    node whose low 62 bits are all set (for K = 31 that is T..T again) -> T: there (node << 2) + 4 carries out of the
    low word."""
    edges, counts, _ = tips_cases.combined_graph(K)
    got = dict(zip(edges, counts))
    low62 = min(all_t(K), (1 << 62) - 1)
    for e, c in (((all_t(K) << 2) | 3, 7), ((all_t(K) << 2) | 2, 9), ((low62 << 2) | 3, 11)):
        got.setdefault(e, c)
        got.setdefault(oracle.revcomp(e, K + 1), got[e])
    edges = sorted(got)
    return edges, [got[e] for e in edges]


def limit_nodes(K, edges, rng):
    node_mask = all_t(K)
    own = {e >> 2 for e in edges} | {e & node_mask for e in edges}
    nodes = [0, all_t(K)]
    for v in sorted(own):
        nodes += [v, max(0, v - 1), min(all_t(K), v + 1)]
    bits = {30: (58, 59), 31: (60, 61), 62: (62, 63, 64, 123)}[K]
    for b in bits:
        nodes += [1 << b, (1 << b) - 1, (1 << b) | 1, all_t(K) ^ (1 << b)]
        nodes += [rng.randrange(4 ** K) | (1 << b) for _ in range(50)]
    # the low word of node << 2 is all ones but the last two bits: + 4 carries
    if K == 62:
        nodes += [(rng.randrange(1 << 62) << 62) | ((1 << 62) - 1) for _ in range(50)] + [(1 << 62) - 1]
    return nodes


def expect_node_ranks(edges, K, nodes, incoming, oracle):
    ns = [oracle.revcomp(v, K) for v in nodes] if incoming else nodes
    return [bisect.bisect_left(edges, v << 2) for v in ns], [bisect.bisect_left(edges, (v << 2) + 4) for v in ns]


@pytest.mark.parametrize("K", [30, 31, 62])
def test_graph_queries_at_the_width_limits(oracle, K):
    L = K + 1
    rng = random.Random(600 + K)
    edges, counts = wide_graph(oracle, K)
    assert sum(1 for e in edges if e >> 2 == all_t(K)) >= 2 and edges[0] == 0 and edges[-1] == all_t(L)
    files = oracle.write_graph(edges, counts, K, out="gq")
    rd = oracle.SparseReader(files, "gq-edges")
    with g.Object.open(files, "gq", g.OBJECT_GRAPH) as obj:
        assert (obj.key_words, obj.node_words) == {30: (1, 1), 31: (2, 1), 62: (2, 2)}[K]
        check_rank_select(obj, edges, 4 ** L, rng, 2000, rd, 200)
        want = np.asarray(counts, dtype=np.uint32)
        assert np.array_equal(obj.multiplicity(np.arange(len(edges), dtype=np.uint64)), want)
        assert np.array_equal(obj.lookup(to_keys(edges, obj.key_words)), want)
        _check_node_ranks(obj, edges, K, rng)
        nodes = limit_nodes(K, edges, rng)
        for incoming in (False, True):
            b, e = obj.node_ranks(to_keys(nodes, obj.node_words), incoming=incoming)
            eb, ee = expect_node_ranks(edges, K, nodes, incoming, oracle)
            assert u64(b) == eb and u64(e) == ee, incoming
        # the all-T node: two edges leave it, and its end is the edge count
        b, e = obj.node_ranks(to_keys([all_t(K)], obj.node_words))
        assert (int(b[0]), int(e[0])) == (len(edges) - 2, len(edges))
        if K == 62:
            b, e = obj.node_ranks(to_keys([(1 << 62) - 1], 2))
            assert int(e[0]) - int(b[0]) == 1 and edges[int(b[0])] == (1 << 64) - 1


# ---- k-mer sets at K = 31, 32, 63 ----------------------------------------------------------------------------------

def wide_kmers(oracle, K, rng):
    text = {"A": "A" * K, "T but one": "T" * (K - 1) + "G", "ACAC": ("AC" * K)[:K]}
    if K % 2 == 0:
        u = "".join(rng.choice("ACGT") for _ in range(K // 2))
        text["palindrome"] = u + dg.rc_text(u)
        assert oracle.revcomp(oracle.kmer_value(text["palindrome"]), K) == oracle.kmer_value(text["palindrome"])
    special = {oracle.normalize(oracle.kmer_value(s), K) for s in text.values()}
    return sorted(special | {oracle.normalize(rng.randrange(4 ** K), K) for _ in range(2000)})


@pytest.mark.parametrize("K", [31, 32, 63])
def test_kmer_set_queries_at_the_width_limits(oracle, K):
    rng = random.Random(700 + K)
    elems = wide_kmers(oracle, K, rng)
    stored = set(elems)
    files = oracle.write_kmer_set(elems, K, out="ks")
    rd = oracle.SparseReader(files, "ks.kmers")
    with g.Object.open(files, "ks", g.OBJECT_KMER_SET) as obj:
        assert obj.key_words == (1 if K == 31 else 2)
        check_rank_select(obj, elems, 4 ** K, rng, 2000, rd, 200)
        _check_normalize(obj, elems, K)
        # keys whose top two bits are set, and their reverse complements: either strand of stored k-mers, and strangers
        top = [v for x in elems for v in (x, oracle.revcomp(x, K)) if v >> (2 * K - 2) == 3]
        top += [(3 << (2 * K - 2)) | rng.randrange(4 ** (K - 1)) for _ in range(500)] + [all_t(K)]
        assert len(top) > 1000 and any(v in stored for v in top) and any(oracle.revcomp(v, K) in stored for v in top)
        q = top + [oracle.revcomp(v, K) for v in top]
        canon = [oracle.normalize(v, K) for v in q]
        assert any(c != v for c, v in zip(canon, q)) and any(c not in stored for c in canon)
        r, p = obj.rank(to_keys(q, obj.key_words), normalize=True)
        assert u64(r) == [bisect.bisect_left(elems, c) for c in canon]
        assert p.tolist() == [c in stored for c in canon]
        assert obj.lookup(to_keys(q, obj.key_words), normalize=True).tolist() == [int(c in stored) for c in canon]
        # without the flag the key is looked up as it stands
        r, p = obj.rank(to_keys(q, obj.key_words))
        assert u64(r) == [bisect.bisect_left(elems, v) for v in q] and p.tolist() == [v in stored for v in q]


# ---- K = 1 .. 5, every key and every node ----------------------------------------------------------------------------

def check_every_key(oracle, obj, elems, counts, L):
    """rank, presence and lookup of all 4^L keys with and without normalize; select of every rank; the rank one past
    the last is refused and named"""
    n = len(elems)
    count_of = dict(zip(elems, counts))
    every = list(range(4 ** L))
    for nz in (False, True):
        looked = [oracle.normalize(v, L) for v in every] if nz else every
        r, p = obj.rank(to_keys(every, 1), normalize=nz)
        assert u64(r) == [bisect.bisect_left(elems, v) for v in looked], nz
        assert p.tolist() == [v in count_of for v in looked], nz
        assert obj.lookup(to_keys(every, 1), normalize=nz).tolist() == [count_of.get(v, 0) for v in looked], nz
    assert obj.count == n and u64(obj.select(np.arange(n, dtype=np.uint64))) == elems
    with pytest.raises(g.GossGpuError) as e:
        obj.select(np.arange(n + 1, dtype=np.uint64))
    assert e.value.status == -1 and "query %d" % n in str(e.value)
    with pytest.raises(g.GossGpuError) as e:
        obj.rank(to_keys(every + [4 ** L], 1))
    assert e.value.status == -1 and "query %d" % 4 ** L in str(e.value)


@pytest.mark.parametrize("K", [1, 2, 3, 5])
@pytest.mark.parametrize("step", [1, 2])
def test_small_kmer_sets_exhaustively(oracle, K, step):
    canon = sorted({oracle.normalize(v, K) for v in range(4 ** K)})[::step]
    with g.Object.open(oracle.write_kmer_set(canon, K, out="ks"), "ks", g.OBJECT_KMER_SET) as obj:
        assert obj.key_words == 1
        check_every_key(oracle, obj, canon, [1] * len(canon), K)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_small_graphs_exhaustively(oracle, K):
    """the two largest graphs of the dense corpus at this K: the complete one, and the largest that is not"""
    graphs = sorted((gr for gr in dg.corpus() if gr[1] == K), key=lambda gr: -len(gr[2]))[:2]
    assert len(graphs[0][2]) == 4 ** (K + 1) > len(graphs[1][2])
    for name, _, edges, counts in graphs:
        with g.Object.open(oracle.write_graph(edges, counts, K, out="gq"), "gq", g.OBJECT_GRAPH) as obj:
            assert (obj.key_words, obj.node_words) == (1, 1)
            check_every_key(oracle, obj, edges, counts, K + 1)
            assert obj.multiplicity(np.arange(len(edges), dtype=np.uint64)).tolist() == counts
            nodes = list(range(4 ** K))
            degrees = {}
            for nz in (False, True):
                for incoming in (False, True):
                    ns = [oracle.normalize(v, K) for v in nodes] if nz else nodes
                    eb, ee = expect_node_ranks(edges, K, ns, incoming, oracle)
                    b, e = obj.node_ranks(to_keys(nodes, 1), incoming=incoming, normalize=nz)
                    assert u64(b) == eb and u64(e) == ee, (name, nz, incoming)
                    degrees[nz, incoming] = sum(ee) - sum(eb)
            # every edge leaves one node and enters one
            assert degrees[False, False] == degrees[False, True] == len(edges), name
