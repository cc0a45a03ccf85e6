"""Queries against objects resident in HBM (goss_gpu_object_*, gossamer_amd.Object): rank / presence, select,
multiplicity, lookup and node ranks of committed, product-built and oracle-written KmerSets, Graphs and bare
SparseArrays.  Expected answers come from numpy (searchsorted over the decoded element list) and from the
oracle's restatement of the reference's readers (SparseReader, vba_get)."""
import json
import os
import random
import struct

import numpy as np
import pytest

import gossamer_amd as g

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KMER_SET_CMDS = ("build-kmer-set", "merge-kmer-sets", "intersect-kmer-sets", "subtract-kmer-set", "merge-and-annotate-kmer-sets")


def _golden():
    import base64
    import zlib
    with open(os.path.join(HERE, "golden", "small_objects.json")) as f:
        gd = json.load(f)
    for c in gd["cases"]:
        c["bytes"] = {n: zlib.decompress(base64.b64decode(h)) for n, h in c["files"].items()}
    return gd


# ---- keys as python ints <-> the ABI's layout ------------------------------------------------------------------

def to_keys(vals, words):
    vals = [int(v) for v in vals]
    if words == 1:
        return np.array(vals, dtype=np.uint64)
    return np.array([[v & 0xFFFFFFFFFFFFFFFF, v >> 64] for v in vals], dtype=np.uint64).reshape(-1, 2)


def from_keys(a, words):
    a = np.asarray(a)
    if words == 1:
        return [int(x) for x in a.reshape(-1)]
    a = a.reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[:, 0], a[:, 1])]


def sorted_array(vals, words):
    """what np.searchsorted can search: uint64 for one-word keys, python ints (object) for two-word keys"""
    return np.array([int(v) for v in vals], dtype=np.uint64 if words == 1 else object)


def expect_rank(elems, queries, words):
    e = sorted_array(elems, words)
    q = sorted_array(queries, words)
    r = np.searchsorted(e, q, side="left")
    present = np.zeros(len(q), dtype=bool)
    inside = r < len(e)
    present[inside] = e[r[inside]] == q[inside]
    return r.astype(np.uint64), present


def decode(files, sa):
    import oracle_lib
    rd = oracle_lib.SparseReader(files, sa)
    return [rd.select(i) for i in range(rd.count())], rd


def boundary_queries(elems, universe, rng, nrandom, D):
    q = [0, universe - 1]
    q += [rng.randrange(universe) for _ in range(nrandom)]
    for x in elems:
        q += [x, max(0, x - 1), min(universe - 1, x + 1)]
    # the first and last element of every high-bits group (the posD boundaries) and the group's own ends
    groups = {}
    for x in elems:
        groups.setdefault(x >> D, []).append(x)
    for h, xs in groups.items():
        q += [xs[0], xs[-1], h << D, min(universe - 1, ((h + 1) << D) - 1)]
    return q


def check_rank_select(obj, elems, universe, rng, nrandom, oracle_reader=None, n_oracle=0):
    words = obj.key_words
    n = len(elems)
    assert obj.count == n
    if n:
        got = obj.select(np.arange(n, dtype=np.uint64))
        assert from_keys(got, words) == elems
        r, p = obj.rank(to_keys(elems, words))
        assert np.array_equal(r, np.arange(n, dtype=np.uint64)) and p.all()
    q = boundary_queries(elems, universe, rng, nrandom, obj.D)
    r, p = obj.rank(to_keys(q, words))
    er, ep = expect_rank(elems, q, words)
    assert np.array_equal(r, er)
    assert np.array_equal(p, ep)
    if oracle_reader is not None:
        for i in rng.sample(range(len(q)), min(n_oracle, len(q))):
            assert oracle_reader.rank(q[i]) == int(r[i]), q[i]
            assert oracle_reader.access(q[i]) == bool(p[i]), q[i]
    return q, r, p


# ---- 1 + 2: the committed objects ----------------------------------------------------------------------------------

def test_golden_objects():
    import oracle_lib
    gd = _golden()
    rng = random.Random(41)
    for c in gd["cases"]:
        name, K = c["name"], c["k"]
        graph = c["cmd"] not in KMER_SET_CMDS
        kind = g.OBJECT_GRAPH if graph else g.OBJECT_KMER_SET
        sa = name + ("-edges" if graph else ".kmers")
        elems, rd = decode(c["bytes"], sa)
        length = K + 1 if graph else K
        with g.Object.open(c["bytes"], name, kind) as obj:
            assert obj.K == K and obj.count == len(elems)
            assert obj.key_words == (1 if 2 * length <= 62 else 2)
            check_rank_select(obj, elems, 4 ** length, rng, 2000 if obj.key_words == 1 else 500, rd, 300)
            if graph:
                m = obj.multiplicity(np.arange(len(elems), dtype=np.uint64))
                for i in rng.sample(range(len(elems)), 40):
                    assert int(m[i]) == oracle_lib.vba_get(c["bytes"], name + "-counts", i)
                assert np.array_equal(obj.lookup(to_keys(elems, obj.key_words)), m)
            else:
                assert (obj.lookup(to_keys(elems, obj.key_words)) == 1).all()


def test_golden_dumps_known_answers():
    """each line of the committed dump-kmer-set / dump-graph text, encoded and looked up: the dump's multiplicity
    (1 for a k-mer set)"""
    gd = _golden()
    cases = {c["name"]: c for c in gd["cases"]}
    for name, kind in (("ks25a", g.OBJECT_KMER_SET), ("gr27a", g.OBJECT_GRAPH)):
        lines = gd["dumps"][name].splitlines()
        K = int(lines[1].split("\t")[0])
        rows = [ln.split("\t") for ln in lines[2:] if ln]
        seqs = [r[0] for r in rows]
        want = np.array([int(r[1]) if kind == g.OBJECT_GRAPH else 1 for r in rows], dtype=np.uint32)
        assert len(seqs[0]) == (K + 1 if kind == g.OBJECT_GRAPH else K)
        with g.Object.open(cases[name]["bytes"], name, kind) as obj:
            got = obj.lookup(g.encode_kmers(seqs, len(seqs[0])))
            assert np.array_equal(got, want)


# ---- 3 + 6 + 7 + 9: the product's own objects ------------------------------------------------------------------

def _genome_reads(seed, genome_len=12000, nreads=1500, read_len=100):
    rng = random.Random(seed)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    gen = [rng.choice("ACGT") for _ in range(genome_len)]
    for i in range(30):                                 # homopolymers, palindromes, T..TA..A (as fuzz_parity.py plants them)
        n = rng.randint(20, 90)
        if i % 3 == 0:
            piece = rng.choice("ACGT") * n
        elif i % 3 == 1:
            half = "".join(rng.choice("ACGT") for _ in range(n // 2))
            piece = half + "".join(comp[x] for x in reversed(half))
        else:
            piece = "T" * (n // 2) + "A" * (n - n // 2)
        at = rng.randrange(genome_len - n)
        gen[at:at + n] = piece
    gen = "".join(gen)
    reads = []
    for _ in range(nreads):
        p = rng.randrange(genome_len - read_len)
        r = gen[p:p + read_len]
        reads.append(r if rng.random() < 0.5 else "".join(comp[x] for x in reversed(r)))
    return "\n".join(reads) + "\n"


def _revcomp(v, n):
    import oracle_lib
    return oracle_lib.revcomp(v, n)


@pytest.mark.parametrize("k,mode", [(25, g.MODE_KMER_SET), (45, g.MODE_KMER_SET), (27, g.MODE_GRAPH), (55, g.MODE_GRAPH)])
def test_product_objects_emitted_and_from_files(k, mode):
    import oracle_lib
    import torch
    reads = _genome_reads(k)
    graph = mode == g.MODE_GRAPH
    rng = random.Random(k)
    with g.Context(k, mode, hbm_budget=256 << 20) as ctx:
        ctx.push_host(reads)
        ctx.finish()
        elems, counts = ctx.result()
        files = {"x" + s: b for s, b in ctx.emit().items()}
        a = g.Object.from_context(ctx)
    # (the emitted object outlives its context)
    kind = g.OBJECT_GRAPH if graph else g.OBJECT_KMER_SET
    length = k + 1 if graph else k
    with a, g.Object.open(files, "x", kind) as b:
        assert a.info() == b.info()
        rd = oracle_lib.SparseReader(files, "x-edges" if graph else "x.kmers")
        nrand = 20000 if a.key_words == 1 else 4000
        qa = check_rank_select(a, elems, 4 ** length, rng, nrand, rd, 400)
        qb = check_rank_select(b, elems, 4 ** length, random.Random(k), nrand)
        assert all(np.array_equal(x, y) for x, y in zip(qa[1:], qb[1:]))
        keys = to_keys(elems, a.key_words)
        if graph:
            want = np.asarray(counts, dtype=np.uint32)
            for obj in (a, b):
                assert np.array_equal(obj.multiplicity(np.arange(len(elems), dtype=np.uint64)), want)
                assert np.array_equal(obj.lookup(keys), want)
            _check_node_ranks(a, elems, k, rng)
        else:
            _check_normalize(a, elems, k)
        # the torch path gives the numpy path's answers
        q = to_keys(qa[0], a.key_words)
        tq = torch.from_numpy(q.view(np.int64)).cuda()
        tr, tp = a.rank(tq)
        assert isinstance(tr, torch.Tensor) and tr.is_cuda
        assert np.array_equal(tr.cpu().numpy().view(np.uint64), qa[1]) and np.array_equal(tp.cpu().numpy(), qa[2])
        assert np.array_equal(a.lookup(tq).cpu().numpy().view(np.uint32), a.lookup(q))
        ranks = torch.arange(len(elems), dtype=torch.int64, device="cuda")
        assert np.array_equal(a.select(ranks).cpu().numpy().view(np.uint64), keys)


def _check_normalize(obj, elems, k):
    """both strands of every element are present with the flag; without it only the stored (canonical) one"""
    rcs = [_revcomp(x, k) for x in elems]
    both = to_keys(elems + rcs, obj.key_words)
    assert (obj.lookup(both, normalize=True) == 1).all()
    _, p = obj.rank(both, normalize=True)
    assert p.all()
    stored = set(elems)
    want = np.array([1] * len(elems) + [1 if r in stored else 0 for r in rcs], dtype=np.uint32)
    assert np.array_equal(obj.lookup(both), want)
    assert any(r != x for r, x in zip(rcs, elems)) and not all(r in stored for r in rcs)


def _check_node_ranks(obj, edges, K, rng):
    """out- and in-degree of every node and of random nodes against counts over the edge list; the all-T node's end
    is the edge count"""
    nodes = sorted({e >> 2 for e in edges} | {_revcomp(e >> 2, K) for e in edges})
    nodes += [0, 4 ** K - 1] + [rng.randrange(4 ** K) for _ in range(2000)]
    words = obj.node_words
    e = sorted_array(edges, obj.key_words)

    def expect(ns):
        lo = np.searchsorted(e, sorted_array([n << 2 for n in ns], obj.key_words))
        hi = np.searchsorted(e, sorted_array([(n << 2) + 4 for n in ns], obj.key_words))
        return lo.astype(np.uint64), hi.astype(np.uint64)

    b, en = obj.node_ranks(to_keys(nodes, words))
    eb, ee = expect(nodes)
    assert np.array_equal(b, eb) and np.array_equal(en, ee)
    assert int(en[nodes.index(4 ** K - 1)]) == len(edges)
    bi, ei = obj.node_ranks(to_keys(nodes, words), incoming=True)
    eb, ee = expect([_revcomp(n, K) for n in nodes])
    assert np.array_equal(bi, eb) and np.array_equal(ei, ee)
    outdeg = np.asarray(en, dtype=np.int64) - np.asarray(b, dtype=np.int64)
    assert ((outdeg >= 0) & (outdeg <= 4)).all() and outdeg.sum() >= len(edges)


# ---- 4: bare SparseArrays, every DenseSelect block kind, wide universes --------------------------------------------

def _block_kinds(img):
    h = struct.unpack("<16Q", img[:128])
    idx, nb = h[2], h[8]
    kinds = set()
    for blk in range(nb):
        w = struct.unpack("<Q", img[idx + 8 * blk: idx + 8 * blk + 8])[0] & 7
        kinds.add("scan" if w == 0 else "two-level" if w == 5 else "explicit")
    return kinds


def _bare_cases():
    rng = random.Random(22)
    cases = []
    for bits in (72, 100):
        dense = sorted({rng.getrandbits(bits) for _ in range(20000)})
        cases.append(("dense%d" % bits, dense, 1 << bits, len(dense)))
        # an estimate far above the count: small D, a sparse bitmap of 2^22 zeros
        sparse = sorted({rng.getrandbits(bits) for _ in range(30000)})
        cases.append(("sparse%d" % bits, sparse, 1 << bits, int(2 ** 22 / 1.4426950408889634)))
    return cases


def test_bare_sparse_arrays_all_block_kinds():
    import oracle_lib
    rng = random.Random(23)
    kinds = set()
    big_d = False
    for name, pos, N, M in _bare_cases():
        files = oracle_lib.write_sparse_array(pos, N, M, base="sa")
        kinds |= _block_kinds(files["sa-d0"]) | _block_kinds(files["sa-d1"])
        rd = oracle_lib.SparseReader(files, "sa")
        with g.Object.open(files, "sa", g.OBJECT_SPARSE_ARRAY) as obj:
            assert obj.key_words == 2 and obj.N == N and obj.count == len(pos), name
            big_d |= obj.D >= 64
            check_rank_select(obj, pos, N, rng, 3000, rd, 300)
            assert (obj.lookup(to_keys(pos, 2)) == 1).all()
    assert kinds == {"scan", "explicit", "two-level"}, kinds
    assert big_d


# ---- 5: VariableByteArray widths --------------------------------------------------------------------------------

def test_multiplicity_widths():
    import oracle_lib
    rng = random.Random(24)
    K = 27
    special = [1, 255, 256, 65535, 65536, 2 ** 24, 2 ** 32 - 1]
    edges = sorted({rng.getrandbits(2 * K + 2) for _ in range(5000)})
    counts = [special[i % len(special)] if i % 3 == 0 else rng.choice([1, 2, 3, rng.randrange(1, 2 ** 32)]) for i in range(len(edges))]
    files = oracle_lib.write_graph(edges, counts, K, out="gw")
    with g.Object.open(files, "gw", g.OBJECT_GRAPH) as obj:
        want = np.array(counts, dtype=np.uint32)
        assert np.array_equal(obj.multiplicity(np.arange(len(edges), dtype=np.uint64)), want)
        assert np.array_equal(obj.lookup(to_keys(edges, 1)), want)
        present = set(edges)
        absent = [x + 1 for x in edges if x + 1 not in present][:500]
        assert (obj.lookup(to_keys(absent, 1)) == 0).all()
        for i in rng.sample(range(len(edges)), 30):
            assert oracle_lib.vba_get(files, "gw-counts", i) == counts[i]


# ---- 8: refusals -----------------------------------------------------------------------------------------------

def _status(f):
    with pytest.raises(g.GossGpuError) as e:
        f()
    return e.value.status, str(e.value)


def test_refusals_and_empty_object():
    import oracle_lib
    K = 25
    rng = random.Random(25)
    elems = sorted({rng.getrandbits(2 * K) for _ in range(3000)})
    ks = oracle_lib.write_kmer_set(elems, K, out="ks")
    with g.Object.open(ks, "ks", g.OBJECT_KMER_SET) as obj:
        st, msg = _status(lambda: obj.rank(np.array([5, 4 ** K, 7], dtype=np.uint64)))
        assert st == -1 and "query 1" in msg
        st, msg = _status(lambda: obj.select(np.array([0, 1, len(elems)], dtype=np.uint64)))
        assert st == -1 and "query 2" in msg
        assert _status(lambda: obj.multiplicity(np.array([0], dtype=np.uint64)))[0] in (-1, -5)
        assert _status(lambda: obj.node_ranks(np.array([0], dtype=np.uint64)))[0] in (-1, -5)
        assert obj.lookup(np.array([elems[0]], dtype=np.uint64))[0] == 1      # (the object still answers)
    low = sorted(n for n in ks if n.startswith("ks.kmers.low-bits"))[0]
    for damage, name in ((lambda f: f.pop("ks.kmers-d1"), "ks.kmers-d1"),
                         (lambda f: f.__setitem__(low, f[low][:-1]), low),
                         (lambda f: f.__setitem__("ks.kmers-d1", f["ks.kmers-d1"][:-24]), "ks.kmers-d1"),
                         (lambda f: f.__setitem__("ks.kmers.high-bits", f["ks.kmers.high-bits"][:8]), "ks.kmers.high-bits")):
        files = dict(ks)
        damage(files)
        st, msg = _status(lambda: g.Object.open(files, "ks", g.OBJECT_KMER_SET))
        assert st == -1 and name in msg, msg
    gr = oracle_lib.write_graph([1, 2, 3], [1, 2, 3], 27, out="gq")
    gr.pop("gq-counts.ord2")
    st, msg = _status(lambda: g.Object.open(gr, "gq", g.OBJECT_GRAPH))
    assert st == -1 and "gq-counts.ord2" in msg
    empty = oracle_lib.write_kmer_set([], K, out="e")
    with g.Object.open(empty, "e", g.OBJECT_KMER_SET) as obj:
        r, p = obj.rank(np.array([0, 12345, 4 ** K - 1], dtype=np.uint64))
        assert (r == 0).all() and not p.any()
        assert (obj.lookup(np.array([0, 99], dtype=np.uint64)) == 0).all()
        assert _status(lambda: obj.select(np.array([0], dtype=np.uint64)))[0] == -1
