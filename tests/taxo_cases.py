"""The corpus of the taxonomy tests: trees, k-mer sets, the genomes that annotate them and the reads classified against
the result.  Plain Python over taxo_model.py and match_model.py; nothing here knows the library.  test_taxo_cpu.py holds
every case to the claims made here, so that test_gpu_taxo.py cannot pass on an empty case.

Trees (TREES): a lone root; a path of 40; a star of 1 + 70 leaves (more classes than a wave has lanes); a complete
binary tree of 127; a random tree of 1 000.  Node ids are sparse and in no order, 0 and 0xFFFFFFFD among them, and the
nodes are given in a shuffled order, so an index, a pre-order number and an id are three different things.

Every tree names the nodes the planted inputs are about, where it has them: root; leaf, its deepest node; mid, halfway
up from it; leaf2, under mid and incomparable with leaf; sib, incomparable with mid (with leaf where there is no mid).

A case (fixture(tree, K), K = 15, 31, 32 -- both sides of the one-word / two-word key) holds
  keys    the canonical K-mers of a handful of 600-base genomes, one of which (`un`) no item annotates
  items   [(reads, node id)] in the order of the annotation list: a genome for each named node; a segment shared by
          leaf and leaf2 (lifted to their lca), one by leaf and then mid (lifted to mid), one by leaf and sib (lifted to the root), one first touched by the root
          and then by leaf and sib (no write after the first); the head of the root's genome once more; and `wave`, one K-mer on 128 consecutive one-window
          lines, each line another node of W (the star's 70 leaves; elsewhere the leaves under mid), so that the lanes
          of one wave join many classes into one word
  data    the reads: first a read of 5 000 bases whose first tile holds a chain and whose third holds sib, then its
          mirror (two incomparable classes first, a chain two tiles on); pieces of root, mid and leaf in each of the six
          orders; leaf with sib; a read with only unannotated hits; reads without a hit; empty and short reads; and (on
          the binary tree) a read boundary on every offset from -(K + 1) to K + 1 around a 2 048-byte tile edge, a piece
          ending right on it and another beginning right behind
  pairs   (file 1, file 2): mates that are each a chain and together are not, and the milder combinations."""
import functools
import itertools
import random

import match_model as mm
import taxo_model as tm

TILE = 2048
KS = (15, 31, 32)
TREES = ("root1", "path40", "star70", "bin127", "rand1000")
NAMES = [(t, K) for t in TREES for K in KS]


def _structure(name):
    """parent[] with node 0 the root and every parent before its children"""
    if name == "root1":
        return [0]
    if name == "path40":
        return [0] + list(range(39))
    if name == "star70":
        return [0] * 71
    if name == "bin127":
        return [0] + [(i - 1) // 2 for i in range(1, 127)]
    rng = random.Random(7)
    return [0] + [rng.randrange(max(0, i - 30), i) if i % 3 else rng.randrange(i) for i in range(1, 1000)]


@functools.lru_cache(maxsize=None)
def tree(name):
    parent = _structure(name)
    n = len(parent)
    rng = random.Random("tree " + name)
    order = list(range(n))
    rng.shuffle(order)                           # order[j] = the structural node given j-th
    at = {v: j for j, v in enumerate(order)}
    ids = rng.sample(range(1, 0xFFFFFFFD), n)
    ids[rng.randrange(n)] = 0
    if n > 1:
        ids[(ids.index(0) + 1) % n] = 0xFFFFFFFD
    return tm.Tree(ids, [at[parent[v]] for v in order])


@functools.lru_cache(maxsize=None)
def named(name):
    """{root, leaf, mid, leaf2, sib: node id or None} and W, the nodes of the wave lines"""
    t = tree(name)
    root = t.ids[t.root]
    depth = {x: t.depth(x) for x in t.ids}
    leaf = max(t.ids, key=lambda x: (depth[x], -t.index[x]))
    anc = t.ancestors(leaf)
    mid = anc[len(anc) // 2] if len(anc) >= 3 else None

    def incomparable(a, b):
        return not tm.is_ancestor_or_equal(t, a, b) and not tm.is_ancestor_or_equal(t, b, a)
    leaf2 = next((x for x in sorted(t.subtree_ids(mid)) if incomparable(x, leaf)), None) if mid is not None else None
    ref = mid if mid is not None else leaf
    sib = next((x for x in sorted(t.ids) if incomparable(x, ref)), None) if leaf != root else None
    under = t.subtree_ids(mid) if mid is not None else t.ids
    W = [x for x in sorted(under) if not t.kids[t.index[x]] and x != root][:70]
    out = {"root": root, "leaf": leaf if leaf != root else None, "mid": mid, "leaf2": leaf2, "sib": sib}
    return out, (W if len(W) >= 2 else [])


def lines(*reads):
    return ("\n".join(reads) + "\n").encode()


def _plant(body, at, seg):
    return body[:at] + seg + body[at + len(seg):]


@functools.lru_cache(maxsize=None)
def fixture(name, K):
    t = tree(name)
    nodes, W = named(name)
    rng = random.Random("case %s %d" % (name, K))
    have = [k for k in ("root", "leaf", "mid", "leaf2", "sib") if nodes[k] is not None]       # (the order of the items)
    gen = {k: mm.genome(rng, 600) for k in have + ["un"]}
    seg = {k: mm.genome(rng, 3 * K) for k in ("lift", "lift_root", "settled", "rise", "wave")}
    if "leaf2" in have:
        gen["leaf"], gen["leaf2"] = _plant(gen["leaf"], 50, seg["lift"]), _plant(gen["leaf2"], 200, seg["lift"])
    if "sib" in have:
        gen["leaf"], gen["sib"] = _plant(gen["leaf"], 250, seg["lift_root"]), _plant(gen["sib"], 30, seg["lift_root"])
    if "leaf" in have:
        gen["root"] = _plant(gen["root"], 300, seg["settled"])
        gen["leaf"] = _plant(gen["leaf"], 150, seg["settled"])
        if "sib" in have:
            gen["sib"] = _plant(gen["sib"], 150, seg["settled"])
    if "mid" in have:
        gen["leaf"], gen["mid"] = _plant(gen["leaf"], 480, seg["rise"]), _plant(gen["mid"], 200, seg["rise"])
    items = [(lines(gen[k][:170], gen[k][170 - K + 1:]), nodes[k]) for k in have]       # (two reads that overlap: every window once)
    items.append((lines(gen["root"][:100]), nodes["root"]))          # (a second time: nothing changes)
    wave_kmer = seg["wave"][:K]
    if W:
        items.append((b"".join(lines(wave_kmer) for _ in range(128)), None))       # (node ids per line: wave_nodes)
    texts = list(gen.values()) + ([wave_kmer] if W else [])
    keys = sorted(set().union(*(set(tm.canonical_windows(x.encode(), K)) for x in texts)))

    # pieces: 2K bases of a stretch of a genome that nothing else was planted into
    clean = {"root": 20, "mid": 20, "leaf": 400, "leaf2": 20, "sib": 400, "un": 100}

    def piece(k, flip=False):
        s = gen[k][clean[k]:clean[k] + 2 * K]
        return mm.rc_text(s) if flip else s

    def foreign(n):
        return mm.genome(rng, n)
    chain = [k for k in ("root", "mid", "leaf") if k in have]
    reads = []
    if "sib" in have:
        a = foreign(5000)
        a = _plant(_plant(_plant(a, 100, piece("root")), 300, piece("leaf")), 2 * TILE + 200, piece("sib"))
        b = foreign(5000)
        b = _plant(_plant(_plant(b, 100, piece("leaf")), 100 + 2 * K + 7, piece("sib")), 4000, piece("root"))
        reads += [a, b]
    for j, perm in enumerate(itertools.permutations(chain)):
        reads.append(foreign(j) + "N".join(piece(k, flip=(j + i) % 2 == 1) for i, k in enumerate(perm)) + foreign(3))
    if "sib" in have:
        reads += [piece("leaf") + "N" + piece("sib"), piece("sib") + piece("leaf")]
    if "leaf2" in have:
        reads += [seg["lift"], seg["lift"] + "N" + piece("leaf2"), seg["lift"][:K + 2] + "n" + piece("mid")]
    reads += [piece("un"), piece("un") + "N" + piece("root"), foreign(80), "", foreign(K - 1), gen["root"][20:20 + K].lower(), seg["settled"]]
    if W:
        reads.append(wave_kmer)
    data = lines(*reads)
    if name == "bin127":
        out = [data]
        at = len(data)
        for d in range(-(K + 1), K + 2):
            edge = (at + 4 * K + TILE - 1) // TILE * TILE + d      # where this read's '\n' goes
            first = foreign(edge - at - 2 * K) + piece("leaf")
            second = piece("mid" if d % 2 else "sib")
            out.append(lines(first, second))
            at += len(out[-1])
        data = b"".join(out)

    def mate(*ks):
        return "N".join(piece(k) for k in ks) if ks else foreign(60)
    pairs = [(("root",), ("root",)), ((), ("root",)), (("root",), ()), ((), ())]
    if "leaf" in have:
        pairs += [(("root", "leaf"), ("root",)), (("leaf",), ("root",))]
    if "mid" in have:
        pairs += [(("root",), ("mid", "leaf")), (("mid",), ("root",))]
    if "sib" in have:
        pairs += [(("root", "leaf"), ("sib",)), (("root", "sib"), ("root", "leaf")), (("leaf", "sib"), ("root",)), ((), ("sib", "leaf"))]
    return {"K": K, "tree": t, "nodes": nodes, "W": W, "keys": keys, "items": items, "data": data, "gen": gen, "seg": seg,
            "pairs": ([mate(*a) for a, _ in pairs], [mate(*b) for _, b in pairs])}


def wave_nodes(name):
    """the node id of each of the 128 wave lines: the nodes of W in turn"""
    W = named(name)[1]
    return [W[i % len(W)] for i in range(128)]


@functools.lru_cache(maxsize=None)
def batches(name, K):
    """[(reads, [node id per read])], one per item"""
    out = []
    for data, node in fixture(name, K)["items"]:
        n = len(mm.read_spans(data))
        out.append((data, wave_nodes(name) if node is None else [node] * n))
    return out


def per_read_items(name, K):
    """the items with one node id each, a wave line an item of its own: what the model takes"""
    out = []
    for data, ids in batches(name, K):
        spans = mm.read_spans(data)
        out += [(data[b:e], x) for (b, e), x in zip(spans, ids)]
    return out


@functools.lru_cache(maxsize=None)
def expected(name, K):
    """{ann, counts, result, windows, info, pair} of the model, computed once"""
    c = fixture(name, K)
    t = c["tree"]
    ann, counts = tm.annotate(t, c["keys"], K, per_read_items(name, K))
    res, nwin, info = tm.classify(t, ann, c["keys"], K, c["data"])
    a = tm.classify(t, ann, c["keys"], K, lines(*c["pairs"][0]))[0]
    b = tm.classify(t, ann, c["keys"], K, lines(*c["pairs"][1]))[0]
    return {"ann": ann, "counts": counts, "result": res, "windows": nwin, "info": info, "mates": (a, b), "pair": tm.pair(t, a, b)}
