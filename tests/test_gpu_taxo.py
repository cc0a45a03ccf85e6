"""annotate-kmers and classify-reads on the device (goss_gpu_object_taxo_*, Object.taxo_*) against the model
(tests/taxo_model.py) over the corpus of tests/taxo_cases.py, which test_taxo_cpu.py holds to its claims.  Sets are
written with the oracle and opened with Object.open."""
import random

import numpy as np
import pytest

import gossamer_amd as g
import match_model as mm
import oracle_lib as o
import taxo_cases as tc
import taxo_model as tm

pytestmark = pytest.mark.gpu

NONE, MANY = g.TAXO_NONE, g.TAXO_MANY


def open_set(keys, K):
    return g.Object.open(o.write_kmer_set(keys, K, out="ks"), "ks", g.OBJECT_KMER_SET)


def open_case(name, K):
    c = tc.fixture(name, K)
    obj = open_set(c["keys"], K)
    obj.taxo_tree(c["tree"].ids, c["tree"].parent)
    obj.taxo_annotation(None)
    return c, obj


def annotate_all(obj, name, K, order=None, one_batch=False):
    bs = tc.batches(name, K)
    bs = [bs[i] for i in order] if order else bs
    if one_batch:
        bs = [(b"".join(d for d, _ in bs), [x for _, ids in bs for x in ids])]
    wins, hits = [], 0
    for data, ids in bs:
        w, info = obj.taxo_annotate(data, np.array(ids, dtype=np.uint32))
        assert info["reads"] == len(ids) and info["windows"] == int(w.sum())
        wins += w.tolist()
        hits += info["hits"]
    return wins, hits


def lists(t, dtype=np.uint32):
    import torch
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy().view(dtype)
    assert t.dtype == dtype
    return t.tolist()


@pytest.mark.parametrize("name,K", tc.NAMES)
def test_corpus(name, K):
    import torch
    exp = tc.expected(name, K)
    c, obj = open_case(name, K)
    t, data = c["tree"], c["data"]
    with obj:
        assert obj.count == len(c["keys"])
        # untouched: every rank NONE, every count 0, every read without a class
        ann, counts = obj.taxo_read_annotation()
        assert set(ann.tolist()) == {NONE} and not counts.any()
        res, _, info = obj.taxo_classify_reads(data)
        assert set(res.tolist()) == {NONE} and info["none"] == info["reads"] and info["unannotated"] > 0

        wins, hits = annotate_all(obj, name, K)
        items = tc.per_read_items(name, K)
        assert wins == [len(mm.windows(d, K)) for d, _ in items]
        assert hits == len(tm.touches(c["keys"], K, items))
        ann, counts = obj.taxo_read_annotation()
        assert ann.dtype == np.uint32 and counts.dtype == np.uint64
        assert ann.tolist() == exp["ann"]
        assert counts.tolist() == exp["counts"]
        first = ann.tobytes()

        # bytes in, numpy out
        res, nwin, starts, info = obj.taxo_classify_reads(data, starts=True)
        assert (lists(res), lists(nwin), lists(starts, np.uint64)) == (exp["result"], exp["windows"], mm.read_starts(data))
        assert {k: info[k] for k in exp["info"]} == exp["info"] and info["ms"] >= 0
        # a device tensor that begins at 1 mod 8; tensors come back; the same arrays a second time
        t1 = torch.from_numpy(np.frombuffer(b"\n" + data, dtype=np.uint8).copy()).cuda()[1:]
        assert t1.data_ptr() % 8 == 1
        res2, nwin2, info2 = obj.taxo_classify_reads(t1)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (res2, nwin2))
        assert (lists(res2), lists(nwin2)) == (exp["result"], exp["windows"])
        assert {k: info2[k] for k in exp["info"]} == exp["info"]
        # what match_reads says of the same bytes
        mw, mh, _ = obj.match_reads(data, normalize=True)
        assert mw.tolist() == exp["windows"]
        assert all(h > 0 for h, r in zip(mh.tolist(), exp["result"]) if r != NONE)

        # the figures per node, and the mates of the pairs
        assert obj.taxo_tally(res).tolist() == tm.tally(t, exp["result"])
        assert obj.taxo_tally(res2).tolist() == tm.tally(t, exp["result"])
        a = obj.taxo_classify_reads(tc.lines(*c["pairs"][0]))[0]
        b = obj.taxo_classify_reads(tc.lines(*c["pairs"][1]))[0]
        assert (a.tolist(), b.tolist()) == exp["mates"]
        assert obj.taxo_pair(a, b).tolist() == exp["pair"]
        assert lists(obj.taxo_pair(torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda())) == exp["pair"]

        # annotating again changes nothing (idempotent); the file written and loaded back classifies alike
        annotate_all(obj, name, K)
        assert obj.taxo_read_annotation()[0].tobytes() == first
        obj.taxo_annotation(first)
        assert obj.taxo_read_annotation()[0].tobytes() == first
        assert obj.taxo_classify_reads(data)[0].tolist() == exp["result"]

    # other orders, one batch, another order of the nodes: identical bytes
    n = len(tc.batches(name, K))
    order = list(range(n))
    random.Random(n).shuffle(order)
    for kw in ({"order": order[::-1]}, {"order": order, "one_batch": True}):
        _, obj = open_case(name, K)
        with obj:
            annotate_all(obj, name, K, **kw)
            assert obj.taxo_read_annotation()[0].tobytes() == first


def test_pair_and_tally_against_the_model():
    name, K = "bin127", 15
    c, obj = open_case(name, K)
    t = c["tree"]
    rng = random.Random(11)
    vals = t.ids + [NONE, MANY]
    a = [rng.choice(vals) for _ in range(5000)] + [x for x in vals for _ in vals]
    b = [rng.choice(vals) for _ in range(5000)] + [y for _ in vals for y in vals]
    # a tally whose lanes mostly agree, one whose lanes all differ, and a short one
    skew = [t.ids[t.root]] * 3000 + [rng.choice(vals) for _ in range(77)] + [NONE] * 500 + [MANY] * 129
    with obj:
        assert obj.taxo_pair(np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)).tolist() == tm.pair(t, a, b)
        for v in (skew, a, vals, vals[:3], []):
            assert obj.taxo_tally(np.array(v, dtype=np.uint32)).tolist() == tm.tally(t, v)
        assert obj.taxo_pair(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)).tolist() == []


def test_special_inputs():
    name, K = "star70", 31
    exp = tc.expected(name, K)
    c, obj = open_case(name, K)
    with obj:
        annotate_all(obj, name, K)
        res, nwin, starts, info = obj.taxo_classify_reads(b"", starts=True)
        assert (res.tolist(), nwin.tolist(), starts.tolist()) == ([], [], [0]) and info["reads"] == 0
        w, info = obj.taxo_annotate(b"", np.zeros(0, dtype=np.uint32))
        assert w.tolist() == [] and info["reads"] == 0
        res, nwin, starts, info = obj.taxo_classify_reads(b"\n\n\n", starts=True)
        assert (res.tolist(), nwin.tolist(), starts.tolist()) == ([NONE] * 3, [0] * 3, [0, 1, 2, 2]) and info["none"] == 3
        # a last read without its newline
        data = c["data"][:-1]
        res, nwin, starts, _ = obj.taxo_classify_reads(data, starts=True)
        assert (res.tolist(), nwin.tolist(), starts.tolist()) == (exp["result"], exp["windows"], mm.read_starts(data))
        # one node id for all the reads
        leaf = c["nodes"]["leaf"]
        obj.taxo_annotation(None)
        w, _ = obj.taxo_annotate(c["data"], leaf)
        assert w.tolist() == exp["windows"]
        ann = obj.taxo_read_annotation()[0]
        assert set(ann.tolist()) == {leaf, NONE}
    # an empty set accepts everything and touches nothing: no tree, no annotation, any node ids
    with open_set([], K) as obj:
        assert obj.count == 0
        nreads = len(exp["result"])
        for step in range(2):
            w, info = obj.taxo_annotate(c["data"], 12345)
            assert w.tolist() == exp["windows"] and info["hits"] == 0 and info["reads"] == nreads
            res, nwin, info = obj.taxo_classify_reads(c["data"])
            assert res.tolist() == [NONE] * nreads and nwin.tolist() == exp["windows"]
            assert (info["none"], info["many"], info["unannotated"]) == (nreads, 0, 0)
            ann, counts = obj.taxo_read_annotation()
            assert ann.tolist() == [] and not counts.any()
            obj.taxo_tree(c["tree"].ids, c["tree"].parent)
            obj.taxo_annotation(None)
            obj.taxo_annotation(b"")


def test_annotate_host_form_with_room_to_spare():
    """goss_gpu_object_taxo_annotate_host where nothing in the staged batch ends on a 256-byte boundary and max_reads
    exceeds the reads: 70 bytes, three reads, five node ids.  The ids must reach the kernel from their own slot."""
    import ctypes as C
    K = 15
    rng = random.Random(5)
    first, second = (bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (22, 23))
    reads, nodes = [first, second, first], [20, 30, 30]      # (the first read's k-mers: lca(20, 30) = 10)
    data = b"\n".join(reads) + b"\n"
    assert len(data) == 70
    t = tm.Tree([10, 20, 30], [0, 0, 0])
    keys = sorted(set(tm.canonical_windows(first, K) + tm.canonical_windows(second, K)[2:]))
    items = list(zip(reads, nodes))
    exp_ann, _ = tm.annotate(t, keys, K, items)
    assert set(exp_ann) == {10, 30}
    with open_set(keys, K) as obj:
        obj.taxo_tree(t.ids, t.parent)
        obj.taxo_annotation(None)
        rn = np.array(nodes + [20, 20], dtype=np.uint32)
        w = np.full(5, 0xDEAD, dtype=np.uint32)
        info = g.binding.TaxoInfo()
        rc = obj._L.goss_gpu_object_taxo_annotate_host(obj._h, data, len(data), rn.ctypes.data, g.TAXO_NORMALIZE, 5, w.ctypes.data, C.byref(info))
        assert rc == 0, obj._L.goss_gpu_object_last_error(obj._h)
        assert info.reads == 3 and w.tolist() == [len(mm.windows(r, K)) for r in reads] + [0xDEAD] * 2
        assert info.windows == int(w[:3].sum()) and info.hits == len(tm.touches(keys, K, items))
        assert obj.taxo_read_annotation()[0].tolist() == exp_ann


def refused(call, status, *words):
    with pytest.raises(g.GossGpuError) as e:
        call()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert str(w) in str(e.value), str(e.value)


def test_refusals():
    name, K = "bin127", 15
    exp = tc.expected(name, K)
    c = tc.fixture(name, K)
    t, data = c["tree"], c["data"]
    ids, parent = list(t.ids), list(t.parent)
    nreads = len(exp["result"])
    INVALID, STATE = -1, -5
    # a graph object
    edges = sorted({v for x in c["keys"][:200] for v in (x, o.revcomp(x, K))})
    with g.Object.open(o.write_graph(edges, [1] * len(edges), K - 1, out="gr"), "gr", g.OBJECT_GRAPH) as gr:
        refused(lambda: gr.taxo_tree(ids, parent), INVALID, "KmerSet")
        refused(lambda: gr.taxo_annotation(None), INVALID, "KmerSet")
        refused(lambda: gr.taxo_classify_reads(data), INVALID, "KmerSet")
        refused(lambda: gr.taxo_annotate(data, 1), INVALID, "KmerSet")
    with open_set(c["keys"], K) as obj:
        # nothing before a tree, nothing before an annotation
        refused(lambda: obj.taxo_annotation(None), STATE, "no tree")
        refused(lambda: obj.taxo_classify_reads(data), STATE, "no tree")
        refused(lambda: obj.taxo_pair(np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)), STATE, "no tree")
        # trees that are none
        root = t.root
        other = (root + 1) % t.n
        refused(lambda: obj.taxo_tree([], []), INVALID)
        refused(lambda: obj.taxo_tree(ids, parent[:other] + [other] + parent[other + 1:]), INVALID, "both their own parent")
        refused(lambda: obj.taxo_tree(ids, parent[:root] + [other] + parent[root + 1:]), INVALID)        # no root (a cycle through it)
        refused(lambda: obj.taxo_tree(ids, parent[:other] + [t.n] + parent[other + 1:]), INVALID, "names parent")
        refused(lambda: obj.taxo_tree(ids[:other] + [ids[root]] + ids[other + 1:], parent), INVALID, ids[root], "twice")
        for bad in (NONE, MANY):
            refused(lambda: obj.taxo_tree(ids[:other] + [bad] + ids[other + 1:], parent), INVALID, bad, "reserved")
        leafi = next(i for i in range(t.n) if not t.kids[i])
        cyc = list(parent)
        cyc[parent[leafi]] = leafi               # the leaf's parent hangs under the leaf: a cycle off the root
        refused(lambda: obj.taxo_tree(ids, cyc), INVALID, "does not hang under the root")
        refused(lambda: obj.taxo_annotation(None), STATE, "no tree")

        obj.taxo_tree(ids, parent)
        refused(lambda: obj.taxo_classify_reads(data), STATE, "no annotation")
        refused(lambda: obj.taxo_annotate(data, ids[0]), STATE, "no annotation")
        refused(lambda: obj.taxo_read_annotation(), STATE, "no annotation")
        obj.taxo_annotation(None)
        annotate_all(obj, name, K)
        kept = obj.taxo_read_annotation()[0].tobytes()
        assert kept == np.array(exp["ann"], dtype=np.uint32).tobytes()

        # an id the tree lacks: in the reads' nodes, in a loaded annotation, in pair and tally -- nothing is touched
        missing = next(x for x in range(1, 1 << 20) if x not in t.index)
        nodes = np.full(nreads, ids[3], dtype=np.uint32)
        nodes[5] = missing
        refused(lambda: obj.taxo_annotate(data, nodes), INVALID, "read 5", missing)
        nodes[5] = NONE
        refused(lambda: obj.taxo_annotate(data, nodes), INVALID, "read 5", NONE)
        nodes[5] = ids[3]
        loaded = np.array(exp["ann"], dtype=np.uint32)
        loaded[[77, 400]] = missing
        refused(lambda: obj.taxo_annotation(loaded), INVALID, "rank 77", missing)
        loaded[[77, 400]] = MANY
        refused(lambda: obj.taxo_annotation(loaded), INVALID, "rank 77", MANY)
        refused(lambda: obj.taxo_pair(np.array([ids[0], missing], dtype=np.uint32), np.array([ids[0]] * 2, dtype=np.uint32)), INVALID, "pair 1")
        refused(lambda: obj.taxo_tally(np.array([ids[0], ids[1], missing], dtype=np.uint32)), INVALID, "value 2", missing)
        # too many reads for the arrays; flags that do not exist
        refused(lambda: obj.taxo_classify_reads(data, max_reads=nreads - 1), g.binding.ERR_BUFFER, "max_reads = %d" % nreads)
        refused(lambda: obj.taxo_annotate(data, nodes[:nreads - 1], max_reads=nreads - 1), g.binding.ERR_BUFFER, "max_reads = %d" % nreads)
        refused(lambda: obj.taxo_classify_reads(data, flags=2), INVALID, "flag")
        refused(lambda: obj.taxo_annotate(data, ids[0], flags=4), INVALID, "flag")
        assert obj.taxo_read_annotation()[0].tobytes() == kept
        assert obj.taxo_classify_reads(data)[0].tolist() == exp["result"]

        # a second tree replaces the first and drops the annotation, whose classes were the first's numbers
        obj.taxo_tree(ids[::-1], [t.n - 1 - p for p in parent[::-1]])
        refused(lambda: obj.taxo_classify_reads(data), STATE, "no annotation")
        obj.taxo_annotation(kept)
        assert obj.taxo_classify_reads(data)[0].tolist() == exp["result"]
        assert obj.taxo_read_annotation()[1].tolist() == exp["counts"][::-1]


def test_without_normalize_the_windows_are_looked_up_as_they_stand():
    name, K = "path40", 15
    c, obj = open_case(name, K)
    t, keys = c["tree"], c["keys"]
    rank_of = {x: i for i, x in enumerate(keys)}
    items = tc.per_read_items(name, K)
    touched = [set() for _ in keys]
    for d, node in items:
        for _, x, _ in mm.windows(d, K):
            if x in rank_of:
                touched[rank_of[x]].add(node)
    exp = tm.annotate_sets(t, touched)
    assert exp != tc.expected(name, K)["ann"]
    with obj:
        for data, ids in tc.batches(name, K):
            obj.taxo_annotate(data, np.array(ids, dtype=np.uint32), normalize=False)
        assert obj.taxo_read_annotation()[0].tolist() == exp
        res = []
        for b, e in mm.read_spans(c["data"]):
            res.append(tm.classify_set(t, [exp[rank_of[x]] for _, x, _ in mm.windows(c["data"][b:e], K) if x in rank_of and exp[rank_of[x]] != NONE]))
        assert obj.taxo_classify_reads(c["data"], normalize=False)[0].tolist() == res
