"""The model of annotate-kmers and classify-reads (taxo_model.py): the algebra its order-free statement rests on, that
statement against the reference's loops restated, hand-worked cases, the phylogeny's text, the corpus of the GPU tests
(taxo_cases.py) against vacuity, the declarations of include/goss_gpu_taxo.h, and what the two commands refuse before
they ask for a device.  No GPU."""
import collections
import ctypes as C
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import match_model as mm
import oracle_lib as o
import taxo_cases as tc
import taxo_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
GOLDEN = os.path.join(ROOT, "tests", "golden", "taxo")
NONE, MANY = tm.NONE, tm.MANY


def small_tree():
    """15 nodes: ids 100 + i, node i's parent (i - 1) // 2"""
    return tm.Tree([100 + i for i in range(15)], [0] + [(i - 1) // 2 for i in range(1, 15)])


# ---- the algebra -------------------------------------------------------------------------------------------------------

def test_lca_and_combine_are_semilattice_joins_over_every_triple():
    """associative, commutative, idempotent over every triple of the 127-node tree -- combine also with NONE (the
    identity) and MANY (absorbing) among the values -- by tables of the model's own answers"""
    t = tc.tree("bin127")
    ids = t.ids
    n = len(ids)
    L = np.array([[t.index[tm.lca(t, a, b)] for b in ids] for a in ids])
    vals = ids + [NONE, MANY]
    at = {v: i for i, v in enumerate(vals)}
    Cm = np.array([[at[tm.combine(t, a, b)] for b in vals] for a in vals])
    for T, m in ((L, n), (Cm, n + 2)):
        i = np.arange(m)
        assert (T == T.T).all()
        assert (T[i, i] == i).all()
        a, b, c = np.meshgrid(i, i, i, indexing="ij")
        assert (T[T[a, b], c] == T[a, T[b, c]]).all()
    assert (Cm[n, :] == np.arange(n + 2)).all() and (Cm[n + 1, :] == n + 1).all()
    # the three-node argument behind associativity: a <= b and c comparable with b  =>  c comparable with a
    anc = np.array([[tm.is_ancestor_or_equal(t, a, b) for b in ids] for a in ids])
    comp = anc | anc.T
    assert not (anc[:, :, None] & comp[None, :, :] & ~comp[:, None, :]).any()


def test_the_order_free_statement_is_the_reference_loops():
    t = small_tree()
    ids = t.ids
    # classify: every sequence of up to 4 classes, so every subset in every order and with repeats
    for k in range(0, 5):
        for seq in itertools.product(ids, repeat=k):
            want = tm.classify_set(t, seq)
            assert tm.classify_ref_loop(t, list(seq)) == want
            got = NONE
            for c in seq:
                got = tm.combine(t, got, c)
            assert got == want
    # annotate: every sequence of up to 4 touches of one rank
    for k in range(0, 5):
        for seq in itertools.product(ids, repeat=k):
            assert tm.annotate_ref_loop(t, 1, [(0, v) for v in seq]) == tm.annotate_sets(t, [set(seq)])
    # 200 random inputs over a big tree, in shuffled orders
    t = tc.tree("rand1000")
    rng = random.Random(5)
    for _ in range(200):
        leaf = rng.choice(t.ids)
        pool = t.ancestors(leaf) if rng.random() < 0.6 else rng.sample(t.ids, 6)
        seq = [rng.choice(pool) for _ in range(rng.randrange(1, 9))]
        want_c, want_a = tm.classify_set(t, seq), tm.annotate_sets(t, [set(seq)])
        for _ in range(3):
            rng.shuffle(seq)
            assert tm.classify_ref_loop(t, list(seq)) == want_c
            assert tm.annotate_ref_loop(t, 1, [(0, v) for v in seq]) == want_a
            assert functools_reduce_combine(t, seq) == want_c


def functools_reduce_combine(t, seq):
    got = NONE
    for c in seq:
        got = tm.combine(t, got, c)
    return got


# ---- by hand -----------------------------------------------------------------------------------------------------------

def test_hand_worked_tree():
    t = small_tree()                             # 100; 101 102; 103 104 | 105 106; 107 108 | 109 110 | 111 112 | 113 114
    assert t.ancestors(110) == [110, 104, 101, 100] and t.depth(100) == 0 and t.depth(114) == 3
    assert [t.ids[i] for i in t.preorder()] == [100, 101, 103, 107, 108, 104, 109, 110, 102, 105, 111, 112, 106, 113, 114]
    assert tm.lca(t, 107, 108) == 103 and tm.lca(t, 107, 110) == 101 and tm.lca(t, 107, 114) == 100
    assert tm.lca(t, 103, 107) == 103 and tm.lca(t, 107, 107) == 107 and tm.lca(t, 100, 114) == 100
    assert tm.combine(t, 103, 107) == 107 and tm.combine(t, 107, 103) == 107 and tm.combine(t, 107, 108) == MANY
    assert tm.combine(t, NONE, 107) == 107 and tm.combine(t, 107, NONE) == 107 and tm.combine(t, NONE, NONE) == NONE
    assert tm.combine(t, MANY, 100) == MANY and tm.combine(t, NONE, MANY) == MANY and tm.combine(t, 100, 100) == 100
    assert tm.classify_set(t, []) == NONE and tm.classify_set(t, [101]) == 101
    assert tm.classify_set(t, [100, 110, 101, 104]) == 110 and tm.classify_set(t, [100, 110, 103]) == MANY
    assert tm.classify_ref_loop(t, [104, 100, 110, 110]) == 110 and tm.classify_ref_loop(t, [109, 110]) == MANY
    counts = [0] * 15
    for i, c in ((0, 2), (3, 1), (7, 5), (8, 1), (14, 4)):
        counts[i] = c
    assert tm.totals(t, counts) == [13, 7, 4, 7, 0, 0, 4, 5, 1, 0, 0, 0, 0, 0, 4]
    vals = [100, 107, 107, NONE, MANY, 114, MANY]
    assert tm.node_counts(t, vals) == [1, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 1]
    assert tm.tally(t, vals)[-2:] == [1, 2]
    assert tm.pair(t, [103, 107, NONE, 107], [107, 108, 105, MANY]) == [107, MANY, 105, MANY]


def test_hand_worked_annotate_and_classify():
    """K = 3 over eight k-mers; the canonical form of a 3-mer is whatever match_model says, so the reads are spelt from
    the keys themselves"""
    K = 3
    t = small_tree()
    texts = ["AAC", "ACG", "CAG", "GGA", "TTG", "CCA", "AGA", "GAT"]
    canon = [tm.canonical_windows(x.encode(), K)[0] for x in texts]
    assert len(set(canon)) == 8
    keys = sorted(canon)
    rank = {x: keys.index(c) for x, c in zip(texts, canon)}
    items = [(b"AACNACG\n", 107), (b"ACGNCAG\nGGA\n", 108), (b"CAG\n", 110), (b"GGA\n", 108), (b"TTG\n", 100), (b"TTGNCCA\n", 114)]
    ann, counts = tm.annotate(t, keys, K, items)
    want = {"AAC": 107, "ACG": 103, "CAG": 101, "GGA": 108, "TTG": 100, "CCA": 114, "AGA": NONE, "GAT": NONE}
    assert ann == [want[x] for x in sorted(texts, key=lambda x: rank[x])]
    assert tm.annotate_ref_loop(t, 8, tm.touches(keys, K, items)) == ann
    assert [counts[t.index[x]] for x in (100, 101, 103, 107, 108, 114)] == [1, 1, 1, 1, 1, 1] and sum(counts) == 6
    data = b"TTGNCAGNACGNAAC\nAACNGGA\nAGANGAT\nAGANTTG\nTTTTTTT\n\nCCANTTG\nCCANCAG\n"
    res, nwin, info = tm.classify(t, ann, keys, K, data)
    assert res == [107, MANY, NONE, 100, NONE, NONE, 114, MANY]
    assert nwin == [4, 2, 2, 2, 5, 0, 2, 2]
    assert info == {"reads": 8, "windows": 19, "none": 3, "many": 2, "unannotated": 3}


# ---- the phylogeny's text ----------------------------------------------------------------------------------------------

def test_phylogeny_text_byte_for_byte():
    import gossamer_amd as g
    src = open(os.path.join(GOLDEN, "phylogeny_in.txt")).read()
    want = open(os.path.join(GOLDEN, "phylogeny.txt")).read()
    for parse, fmt in ((tm.parse_phylogeny, tm.format_phylogeny), (g.parse_phylogeny, g.format_phylogeny)):
        root = parse(src)
        nodes, t = tm.flatten(root)
        assert t.ids == [1, 4000000000, 0, 77, 12] and t.parent == [0, 0, 1, 1, 0]
        assert [n["anns"]["name"] for n in nodes] == ["life", "Bacteria", "E.coli", "B.subtilis", "Archaea"]
        # counts given in another order of the nodes than the file's
        other = tm.Tree([12, 0, 1, 77, 4000000000], [2, 4, 2, 4, 2])
        tm.with_counts(root, other, [3, 4, 7, 5, 0])
        assert fmt(root) == want                 # key order (upper case first), one space per depth, tabs
        assert fmt(parse(want)) == want
        assert tm.table(root, other, [0, 2, 0, 0, 1]) == "2\tspecies\tE.coli\n3\tkingdom\tBacteria\n3\troot\tlife\n"
    nodes, ids, parent = g.phylogeny_nodes(g.parse_phylogeny(src), need=("node", "name", "kind"))
    assert (ids, parent) == ([1, 4000000000, 0, 77, 12], [0, 0, 1, 1, 0])
    for bad, word in (("( node 1 )", "name"), ("( name x )", "node"), ("( node x name y )", "id"), ("( node 1 name", "")):
        with pytest.raises(ValueError) as e:
            g.phylogeny_nodes(g.parse_phylogeny(bad))
        assert word in str(e.value)
    t = tc.tree("rand1000")
    assert tm.flatten(tm.parse_phylogeny(tm.format_phylogeny(tm.nested(t))))[1].ids == [t.ids[i] for i in t.preorder()]


# ---- the corpus --------------------------------------------------------------------------------------------------------

def test_trees_are_what_they_claim():
    sizes = {"root1": 1, "path40": 40, "star70": 71, "bin127": 127, "rand1000": 1000}
    for name, n in sizes.items():
        t = tc.tree(name)
        assert t.n == n and len(t.preorder()) == n
        if n > 1:
            assert 0 in t.ids and 0xFFFFFFFD in t.ids and t.ids != sorted(t.ids)
            assert [t.ids[i] for i in t.preorder()] != t.ids            # the order given is no pre-order
        assert all(x < 0xFFFFFFFE for x in t.ids)
    assert max(tc.tree("path40").depth(x) for x in tc.tree("path40").ids) == 39
    assert len(tc.tree("star70").kids[tc.tree("star70").root]) == 70 > 64
    assert collections.Counter(tc.tree("bin127").depth(x) for x in tc.tree("bin127").ids) == {d: 2 ** d for d in range(7)}
    assert len(tc.named("star70")[1]) == 70 and len(set(tc.wave_nodes("star70")[:64])) == 64
    nodes, W = tc.named("bin127")
    assert len(W) == 8 and all(tm.is_ancestor_or_equal(tc.tree("bin127"), nodes["mid"], x) for x in W)
    assert tc.NAMES == [(t, K) for t in ("root1", "path40", "star70", "bin127", "rand1000") for K in (15, 31, 32)]


def runs_with_two_classes(c, ann):
    """how many (run of 64 aligned positions, read) hold hit windows of more than one class"""
    K, keys, data = c["K"], c["keys"], c["data"]
    rank_of = {x: i for i, x in enumerate(keys)}
    seen = collections.defaultdict(set)
    for r, (b, e) in enumerate(mm.read_spans(data)):
        ws = mm.windows(data[b:e], K)
        for (pos, _, _), x in zip(ws, mm.canonical_many([(x, rc) for _, x, rc in ws])):
            if x in rank_of and ann[rank_of[x]] != NONE:
                seen[((b + pos) // 64, r)].add(ann[rank_of[x]])
    return sum(1 for s in seen.values() if len(s) > 1)


@pytest.mark.parametrize("name,K", tc.NAMES)
def test_every_case_meets_what_it_was_planted_for(name, K):
    c, exp = tc.fixture(name, K), tc.expected(name, K)
    t, nodes, keys, data = c["tree"], c["nodes"], c["keys"], c["data"]
    ann, res = exp["ann"], exp["result"]
    assert 1000 < len(keys) < 5000 and keys == sorted(set(keys)) and len(data) < 400000
    # annotate: first touch, lift and no-op all happen; some ranks stay untouched; the reference's loop agrees
    touches = tm.touches(keys, K, tc.per_read_items(name, K))
    assert tm.annotate_ref_loop(t, len(keys), touches) == ann
    cur, kinds = {}, collections.Counter()
    for r, v in touches:
        new = v if r not in cur else tm.lca(t, cur[r], v)
        kinds["first" if r not in cur else "noop" if new == cur[r] else "lift"] += 1
        cur[r] = new
    assert kinds["first"] and kinds["noop"] and ann.count(NONE) > 500
    assert exp["counts"][t.root] > 0 and sum(exp["counts"]) == len(keys) - ann.count(NONE)
    rank_of = {x: i for i, x in enumerate(keys)}

    def classes(text):
        return {ann[rank_of[x]] for x in tm.canonical_windows(text.encode(), K) if x in rank_of}
    if nodes["leaf"] is not None:
        assert kinds["lift"]
        assert classes(c["seg"]["settled"]) == {nodes["root"]}          # the root came first: nothing written after it
    if nodes["mid"] is not None:
        assert classes(c["seg"]["rise"]) == {nodes["mid"]}
    if nodes["leaf2"] is not None:
        assert classes(c["seg"]["lift"]) == {tm.lca(t, nodes["leaf"], nodes["leaf2"])} != {nodes["leaf"]}
    if nodes["sib"] is not None:
        assert classes(c["seg"]["lift_root"]) == {tm.lca(t, nodes["leaf"], nodes["sib"])}
    if c["W"]:
        # one k-mer, 128 one-window lines, and the lanes of a 64-position run bring more than one node to it
        wave = [d for d, _ in tc.batches(name, K) if len(mm.read_spans(d)) == 128][0]
        assert len(wave) == 128 * (K + 1) and len(set(tm.canonical_windows(wave[:K], K))) == 1
        assert len(set(tc.wave_nodes(name)[:64 // (K + 1) + 1])) > 1
        lca_w = c["W"][0]
        for x in c["W"]:
            lca_w = tm.lca(t, lca_w, x)
        assert classes(c["seg"]["wave"][:K]) == {lca_w} and lca_w not in c["W"]
    # classify: every outcome
    spans = mm.read_spans(data)
    per_read = [tm.read_classes(ann, keys, K, data[b:e]) for b, e in spans]
    assert any(r not in (NONE, MANY) for r in res)
    assert any(r == NONE and not cs and u == 0 and w > 0 for r, (cs, w, u) in zip(res, per_read))        # no hit
    assert any(r == NONE and not cs and u > 0 for r, (cs, w, u) in zip(res, per_read))                   # only unannotated hits
    assert any(r != NONE and u > 0 for r, (cs, w, u) in zip(res, per_read))                              # both kinds of hit
    assert any(w == 0 for _, w, _ in per_read) and exp["info"]["unannotated"] > 0
    assert all(tm.classify_ref_loop(t, cs) == r for r, (cs, _, _) in zip(res, per_read))
    chain = [nodes[k] for k in ("root", "mid", "leaf") if nodes[k] is not None]
    orders = {tuple(dict.fromkeys(cs)) for cs, _, _ in per_read if set(cs) == set(chain) and len(cs) > 0}
    assert orders == set(itertools.permutations(chain))
    if len(chain) > 1:
        assert runs_with_two_classes(c, ann) > 0
    if nodes["sib"] is not None:
        assert res.count(MANY) >= 4
        assert any(set(cs) == {nodes["leaf"], nodes["sib"]} for cs, _, _ in per_read)
        # the two long reads: MANY only across tiles, in both orders
        for r, first_is_chain in ((0, True), (1, False)):
            b, e = spans[r]
            assert e - b == 5000 and res[r] == MANY
            by_tile = collections.defaultdict(set)
            ws = mm.windows(data[b:e], K)
            for (pos, _, _), x in zip(ws, mm.canonical_many([(x, rc) for _, x, rc in ws])):
                if x in rank_of and ann[rank_of[x]] != NONE:
                    by_tile[(b + pos) // tc.TILE].add(ann[rank_of[x]])
            tiles = sorted(by_tile)
            assert len(tiles) == 2 and tiles[1] - tiles[0] == 2
            verdicts = [tm.classify_set(t, by_tile[x]) for x in tiles]
            assert (verdicts[0] != MANY, verdicts[1] == MANY) == (first_is_chain, False) and (verdicts[0] == MANY) != first_is_chain
    if name == "bin127":
        # a read boundary at every offset around a tile edge, hits right before it and right behind
        offs = set()
        for r in range(len(spans) - 1):
            e = spans[r][1]
            d = (e + tc.TILE // 2) % tc.TILE - tc.TILE // 2
            if abs(d) <= K + 1 and per_read[r][0] and per_read[r + 1][0] and spans[r + 1][1] - spans[r + 1][0] == 2 * K:
                last = mm.windows(data[spans[r][0]:e], K)[-1][0] + spans[r][0]
                assert last + K == e and res[r] == nodes["leaf"] and res[r + 1] in (nodes["mid"], nodes["sib"])
                offs.add(d)
        assert offs == set(range(-(K + 1), K + 2))
    # pairs: mates that are each a chain and together are not
    a, b = exp["mates"]
    if nodes["sib"] is not None:
        assert any(x not in (NONE, MANY) and y not in (NONE, MANY) and p == MANY for x, y, p in zip(a, b, exp["pair"]))
        assert any(x == MANY and p == MANY for x, p in zip(a, exp["pair"]))
    assert any(x == NONE and y != NONE and p == y for x, y, p in zip(a, b, exp["pair"]))
    assert any(x == NONE and y == NONE for x, y in zip(a, b))
    # pooling the mates' windows is the join of their results
    for m1, m2, p in zip(c["pairs"][0], c["pairs"][1], exp["pair"]):
        cs = tm.read_classes(ann, keys, K, m1.encode())[0] + tm.read_classes(ann, keys, K, m2.encode())[0]
        assert tm.classify_set(t, cs) == p == tm.classify_ref_loop(t, cs)


# ---- the library's declarations ----------------------------------------------------------------------------------------

def test_taxo_symbols_are_declared_and_exported():
    import gossamer_amd as g
    text = open(os.path.join(ROOT, "include", "goss_gpu_taxo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(goss_gpu_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(g.TAXO_SYMBOLS) and len(names) == 11
    top = open(os.path.join(ROOT, "include", "goss_gpu.h")).read()
    assert 0 < top.find('#include "goss_gpu_classify.h"') < top.find('#include "goss_gpu_taxo.h"')
    assert "#define GOSS_TAXO_NONE 0xFFFFFFFFu" in text and "#define GOSS_TAXO_MANY 0xFFFFFFFEu" in text
    assert (g.TAXO_NONE, g.TAXO_MANY, g.TAXO_NORMALIZE) == (0xFFFFFFFF, 0xFFFFFFFE, 1) == (tm.NONE, tm.MANY, 1)
    assert re.search(r"uint64_t reads;\s*uint64_t windows;\s*uint64_t hits;\s*uint64_t none;\s*uint64_t many;\s*uint64_t unannotated;\s*float ms;", text)
    assert C.sizeof(g.binding.TaxoInfo) == 8 * 6 + 8
    L = g.load()
    g.binding._declare_object(L)
    for n in names:
        assert hasattr(L, n), n
    assert L.goss_gpu_object_taxo_tree_host(None, 0, None, None) == -1
    assert L.goss_gpu_object_taxo_annotation_host(None, None) == -1
    assert L.goss_gpu_object_taxo_annotation_read(None, None, None) == -1
    assert L.goss_gpu_object_taxo_annotate(None, None, 0, None, 0, 0, None, None) == -1
    assert L.goss_gpu_object_taxo_annotate_host(None, None, 0, None, 0, 0, None, None) == -1
    assert L.goss_gpu_object_taxo_classify_reads(None, None, 0, 0, 0, None, None, None, None) == -1
    assert L.goss_gpu_object_taxo_classify_reads_host(None, None, 0, 0, 0, None, None, None, None) == -1
    assert L.goss_gpu_object_taxo_pair(None, None, None, 0, None) == -1
    assert L.goss_gpu_object_taxo_pair_host(None, None, None, 0, None) == -1
    assert L.goss_gpu_object_taxo_tally(None, None, 0, None) == -1
    assert L.goss_gpu_object_taxo_tally_host(None, None, 0, None) == -1


# ---- the commands, before any device -----------------------------------------------------------------------------------

def run_goss(*args, cwd=None):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode()


def test_cli_usage_errors():
    for cmd, line in (("annotate-kmers", "annotate-kmers   Decorate a graph with an assignment of kmers to graphs."),
                      ("classify-reads", "classify-reads   thread the reads through the graph")):
        tail = "use\n\tgoss %s -h\nfor more usage information.\n" % cmd
        rc, _, err = run_goss(cmd, "-G", "a", "-G", "b", *(("--annotation-list", "x", "--phylogeny", "y") if cmd == "annotate-kmers" else ()))
        assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + tail
        rc, _, err = run_goss(cmd, "-G", "a", "--bogus")
        assert rc == 1 and err == "unknown option '--bogus'\n" + tail
        rc, _, err = run_goss(cmd, "-h")
        assert rc == 1 and "  " + line + "\n" in err
        for opt in (("--annotation-list", "--phylogeny") if cmd == "annotate-kmers" else ("--pairs", "--line-in", "--fasta-in", "--fastq-in", "--buffer-size")):
            assert opt in err, opt
        rc, _, err = run_goss("help")
        assert "  " + line + "\n" in err
    rc, _, err = run_goss("annotate-kmers", "-G", "a")
    assert rc == 1 and err.startswith("mandatory option annotation-list was not given.\nmandatory option phylogeny was not given.\n")


def test_cli_tree_and_list_errors_come_before_any_device(tmp_path):
    """every refusal of a phylogeny or an annotation list names what is wrong, and nothing has been written"""
    base = str(tmp_path / "nothing")             # no such set: a command that got as far as opening it would say so
    lst, phy = tmp_path / "list.txt", tmp_path / "phylo.txt"
    good = "( node 1 name root kind k ( node 2 name a kind k ) )\n"
    lst.write_text("g.fa 2\n")

    def annotate(tree, listing="g.fa 2\n"):
        phy.write_text(tree)
        lst.write_text(listing)
        rc, out, err = run_goss("annotate-kmers", "-G", base, "--annotation-list", str(lst), "--phylogeny", str(phy), "-T", "3")
        assert rc == 1 and out == b"" and err.startswith("error performing annotate-kmers:\n") and phy.read_text() == tree
        assert not os.path.exists(base + ".annotation")
        return err
    assert "has no 'node'" in annotate("( name root ( node 2 name a ) )")
    assert "node 1 (in file order) has no 'name'" in annotate("( node 1 name root ( node 2 ) )")
    assert "node id 7 occurs twice" in annotate("( node 7 name root ( node 7 name a ) )")
    assert "node id 4294967295 is reserved" in annotate("( node 1 name root ( node 4294967295 name a ) )")
    assert "node id 4294967294 is reserved" in annotate("( node 4294967294 name root )")
    assert "has the id '-3'" in annotate("( node -3 name root )")
    assert "has the id '4294967296'" in annotate("( node 4294967296 name root )")
    assert "it ends inside node 0 (in file order)" in annotate("( node 1 name root ( node 2 name a )")
    assert "tokens after the root's ')'" in annotate("( node 1 name root ) ( node 2 name a )")
    assert "has no value" in annotate("( node 1 name )")
    assert "does not begin with '('" in annotate("")
    assert "'g.fa' has node id 5, which the phylogeny" in annotate(good, "g.fa 2\nh.fa 3\ng.fa 5\n")
    assert "'h.fa' has no node id" in annotate(good, "g.fa 2 h.fa")
    assert "'g.fa' has the node id 'x'" in annotate(good, "g.fa x")
    assert "unable to open graph '%s'" % base in annotate(good, "g.fa 1\ng.fa 2\n")       # the last id of a repeated file holds

    reads = tmp_path / "r.txt"
    reads.write_bytes(b"ACGTACGTAC\n")

    def classify(tree, *more):
        open(base + ".taxo", "w").write(tree)
        rc, out, err = run_goss("classify-reads", "-G", base, "--line-in", str(reads), "-B", "1", "-T", "2", *more)
        assert rc == 1 and out == b"" and err.startswith("error performing classify-reads:\n")
        return err
    assert "node 1 (in file order) has no 'kind'" in classify("( node 1 name root kind k ( node 2 name a ) )")
    assert "node id 1 occurs twice" in classify("( node 1 name root kind k ( node 1 name a kind k ) )")
    assert "'%s.annotation'" % base in classify(good) and "No such file" in classify(good)
    open(base + ".annotation", "wb").write(bytes(7))
    assert "holds 7 bytes, no whole number of node ids" in classify(good)
    assert "an even number of input files is required (1 given)" in classify(good, "--pairs")
    # a set of 3 k-mers and an annotation of 2
    keys = sorted({o.normalize(v, 5) for v in (1, 77, 300)})
    base = str(tmp_path / "u")
    for name, data in o.write_kmer_set(keys, 5, out=base).items():
        open(name, "wb").write(data)
    open(base + ".annotation", "wb").write(bytes(8))
    open(base + ".taxo", "w").write(good)
    rc, out, err = run_goss("classify-reads", "-G", base, "--line-in", str(reads))
    assert rc == 1 and out == b""
