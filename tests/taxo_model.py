"""A model of annotate-kmers and classify-reads (goss_gpu_object_taxo_*, `goss annotate-kmers`, `goss classify-reads`)
over Python integers and dicts.  Nothing here knows the library.

Two statements of each computation stand side by side: the order-free one the device implements (a class per k-mer is
the lca of the nodes of the genomes that hold it; a read is counted for the deepest of its classes iff they are a chain
under the ancestor relation), and the reference's loops restated as they stand (GossCmdAnnotateKmers.cc:196-213: set or
lca in list order; GossCmdClassifyReads.cc:301-372: ancestor vectors, comparator sort, entailment scan, early return).
test_taxo_cpu.py holds the two to each other.

A tree is a Tree: nodes in the order given, ids[i], parent[i] (an index; the root's is its own), kids[i] in that order.
A phylogeny file is a nested token list: "(" key value ... child ... ")"; parse_phylogeny gives {"anns": {}, "kids": []}
nodes, format_phylogeny writes AnnotTree::write's form (keys in std::map order, one space per depth, key TAB value)."""
import functools

import match_model as mm

NONE, MANY = 0xFFFFFFFF, 0xFFFFFFFE


class Tree:
    def __init__(self, ids, parent):
        self.ids, self.parent = list(ids), list(parent)
        self.n = len(self.ids)
        self.index = {x: i for i, x in enumerate(self.ids)}
        assert len(self.index) == self.n
        roots = [i for i in range(self.n) if self.parent[i] == i]
        assert len(roots) == 1
        self.root = roots[0]
        self.kids = [[] for _ in range(self.n)]
        for i, p in enumerate(self.parent):
            if i != self.root:
                self.kids[p].append(i)
        self.up = {self.ids[i]: self.ids[p] for i, p in enumerate(self.parent)}      # id -> parent id

    def ancestors(self, x):
        """[x, its parent, ..., the root] (Phylogeny::ancestors)"""
        out = [x]
        while self.up[x] != x:
            x = self.up[x]
            out.append(x)
        return out

    def depth(self, x):
        return len(self.ancestors(x)) - 1

    def preorder(self):
        """node indices, a node before its children, children in the order given"""
        out, stack = [], [self.root]
        while stack:
            v = stack.pop()
            out.append(v)
            stack.extend(reversed(self.kids[v]))
        return out

    def subtree_ids(self, x):
        out, stack = [], [self.index[x]]
        while stack:
            v = stack.pop()
            out.append(self.ids[v])
            stack.extend(self.kids[v])
        return out


# ---- the order-free statement -------------------------------------------------------------------------------------------

def lca(t, a, b):
    """the deepest node that is an ancestor-or-equal of both (Phylogeny::lca: the last common element from the root)"""
    l, r = t.ancestors(a)[::-1], t.ancestors(b)[::-1]
    n = None
    for x, y in zip(l, r):
        if x != y:
            break
        n = x
    return n


def is_ancestor_or_equal(t, a, b):
    return a in t.ancestors(b)


def combine(t, a, b):
    """NONE the identity, MANY absorbing; the deeper of two comparable nodes, MANY for two that are not"""
    if a == NONE:
        return b
    if b == NONE:
        return a
    if a == MANY or b == MANY:
        return MANY
    if is_ancestor_or_equal(t, a, b):
        return b
    if is_ancestor_or_equal(t, b, a):
        return a
    return MANY


def classify_set(t, S):
    """the read's result from the set of classes of its hit windows: d iff S is a non-empty chain and d its deepest"""
    S = set(S)
    if not S:
        return NONE
    for a in S:
        for b in S:
            if not (is_ancestor_or_equal(t, a, b) or is_ancestor_or_equal(t, b, a)):
                return MANY
    return max(S, key=t.depth)


def annotate_sets(t, touched):
    """touched[r] = the set of node ids whose genomes hold k-mer r; the class is their lca, NONE for an empty set"""
    return [functools.reduce(lambda a, b: lca(t, a, b), sorted(s)) if s else NONE for s in touched]


# ---- the reference's loops as they stand -------------------------------------------------------------------------------

def annotate_ref_loop(t, n, touches):
    """KmerClasses::set over (rank, node id) in list order"""
    classes = [NONE] * n
    for r, v in touches:
        classes[r] = v if classes[r] == NONE else lca(t, classes[r], v)
    return classes


def _entail_less(l, r):
    """EntailmentComparitor over ancestor vectors, compared from the root end"""
    for x, y in zip(l[::-1], r[::-1]):
        if x != y:
            return x < y
    return len(l) <= len(r)


def _is_entailed_by(l, r):
    lr, rr = l[::-1], r[::-1]
    return len(lr) <= len(rr) and rr[:len(lr)] == lr


def classify_ref_loop(t, cn):
    """ReadAligner::push_back from the classes of the hit windows, in the order they were met: the node counted, or None
    where the reference returns without counting (no hit: NONE here; multiple spines: MANY here)"""
    if not cn:
        return NONE
    cn = sorted(set(cn))
    xs = [t.ancestors(c) for c in cn]
    rs = sorted(range(len(cn)), key=functools.cmp_to_key(lambda i, j: -1 if _entail_less(xs[i], xs[j]) else 1))
    ss = []
    for i in range(1, len(rs)):
        if not _is_entailed_by(xs[rs[i - 1]], xs[rs[i]]):
            ss.append(xs[rs[i - 1]][0])
    ss.append(xs[rs[-1]][0])
    n = ss[0]
    for _ in ss[1:]:
        return MANY
    return n


# ---- over k-mer sets and reads ------------------------------------------------------------------------------------------

def canonical_windows(read, K):
    return mm.canonical_many([(x, r) for _, x, r in mm.windows(read, K)])


def touched_sets(keys, K, items):
    """items: [(bytes of reads separated by '\\n', node id)] -> per rank the set of node ids"""
    rank_of = {x: i for i, x in enumerate(keys)}
    touched = [set() for _ in keys]
    for data, node in items:
        for b, e in mm.read_spans(data):
            for x in canonical_windows(data[b:e], K):
                if x in rank_of:
                    touched[rank_of[x]].add(node)
    return touched


def touches(keys, K, items):
    """the same as a list of (rank, node id) in the order the reference meets them"""
    rank_of = {x: i for i, x in enumerate(keys)}
    out = []
    for data, node in items:
        for b, e in mm.read_spans(data):
            out += [(rank_of[x], node) for x in canonical_windows(data[b:e], K) if x in rank_of]
    return out


def annotate(t, keys, K, items):
    """(annotation: a node id or NONE per rank, count per node in the order of the tree)"""
    ann = annotate_sets(t, touched_sets(keys, K, items))
    return ann, node_counts(t, ann)


def node_counts(t, values):
    """how often each node occurs, in the order of the tree; NONE and MANY are counted nowhere"""
    c = [0] * t.n
    for v in values:
        if v not in (NONE, MANY):
            c[t.index[v]] += 1
    return c


def tally(t, values):
    return node_counts(t, values) + [sum(1 for v in values if v == NONE), sum(1 for v in values if v == MANY)]


def totals(t, counts):
    """sum of counts over each node's subtree"""
    tot = list(counts)
    for v in reversed(t.preorder()):
        if v != t.root:
            tot[t.parent[v]] += tot[v]
    return tot


def read_classes(ann, keys, K, read):
    """(the classes of the read's hit windows in order, its valid windows, its hits at a rank without a class)"""
    rank_of = {x: i for i, x in enumerate(keys)}
    ws = canonical_windows(read, K)
    got = [ann[rank_of[x]] for x in ws if x in rank_of]
    return [c for c in got if c != NONE], len(ws), sum(1 for c in got if c == NONE)


def classify(t, ann, keys, K, data):
    """(result per read, windows per read, info) as goss_gpu_object_taxo_classify_reads answers"""
    res, nwin, unann = [], [], 0
    for b, e in mm.read_spans(data):
        cs, w, u = read_classes(ann, keys, K, data[b:e])
        res.append(classify_set(t, cs))
        nwin.append(w)
        unann += u
    info = {"reads": len(res), "windows": sum(nwin), "none": res.count(NONE), "many": res.count(MANY), "unannotated": unann}
    return res, nwin, info


def pair(t, a, b):
    return [combine(t, x, y) for x, y in zip(a, b)]


# ---- the phylogeny's text ----------------------------------------------------------------------------------------------

def parse_phylogeny(text):
    toks = text.split()
    at = 0

    def node():
        nonlocal at
        assert toks[at] == "("
        at += 1
        n = {"anns": {}, "kids": []}
        while toks[at] not in ("(", ")"):
            n["anns"][toks[at]] = toks[at + 1]
            at += 2
        while toks[at] != ")":
            n["kids"].append(node())
        at += 1
        return n
    return node()


def format_phylogeny(root):
    out = []

    def node(n, d):
        out.append(" " * d + "(\n")
        for k in sorted(n["anns"]):              # (std::map<string, string>: bytewise key order)
            out.append(" " * (d + 1) + k + "\t" + n["anns"][k] + "\n")
        for c in n["kids"]:
            node(c, d + 1)
        out.append(" " * d + ")\n")
    node(root, 0)
    return "".join(out)


def flatten(root):
    """(nodes in file order, Tree) of a parsed phylogeny"""
    nodes, parent = [], []

    def walk(n, p):
        i = len(nodes)
        nodes.append(n)
        parent.append(i if p is None else p)
        for c in n["kids"]:
            walk(c, i)
    walk(root, None)
    return nodes, Tree([int(n["anns"]["node"]) for n in nodes], parent)


def nested(t, names=None, kinds=None):
    """a Tree as a parsed phylogeny: node, name and, where given, kind"""
    def node(v):
        anns = {"node": str(t.ids[v]), "name": names[v] if names else "n%d" % t.ids[v]}
        if kinds:
            anns["kind"] = kinds[v]
        return {"anns": anns, "kids": [node(c) for c in t.kids[v]]}
    return node(t.root)


def with_counts(root, t, counts, second="total"):
    """the phylogeny annotate-kmers writes back: count and total on every node (file order = flatten's order)"""
    nodes, ft = flatten(root)
    by_id = {t.ids[i]: counts[i] for i in range(t.n)}
    c = [by_id[x] for x in ft.ids]
    tot = totals(ft, c)
    for n, a, b in zip(nodes, c, tot):
        n["anns"]["count"] = str(a)
        n["anns"][second] = str(b)
    return root


def table(root, t, counts):
    """classify-reads' stdout: post-order, children first in file order, nodes with a subtree sum > 0 (counts(), :397-418)"""
    nodes, ft = flatten(root)
    by_id = {t.ids[i]: counts[i] for i in range(t.n)}
    tot = totals(ft, [by_id[x] for x in ft.ids])
    out = []

    def walk(v):
        for c in ft.kids[v]:
            walk(c)
        if tot[v] > 0:
            out.append("%d\t%s\t%s\n" % (tot[v], nodes[v]["anns"]["kind"], nodes[v]["anns"]["name"]))
    walk(ft.root)
    return "".join(out)
