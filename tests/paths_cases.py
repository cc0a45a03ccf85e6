"""Hand-made graphs for the trim-paths / clip-links tests: pieces whose verdict follows by construction.

Every piece is a list of (text, multiplicity) strings over random bases (seeded by K and the piece's name);
tips_model.graph_of turns it into a sorted edge list that holds both strands.  `expect` holds the report fields of ONE
pass over the piece alone and "removed", the edges that really go; it is argued in the comment beside the piece and
never taken from the code under test.  A "long" stretch has more than 2K edges, so that a walk along it is too_long.

trim-paths: a start is an edge whose from-node has no incoming edge ("source").  clip-links: a start is an edge whose
from-node has two or more outgoing edges ("fork").  In a graph with equal multiplicities on both strands the mirror
image of a link that passes is a start that passes as well, so clip-links' `links` and `edges` come in twos -- except
where the link is its own mirror image.
"""
import random

from tips_model import graph_of

KS = (15, 31, 32)                     # one-word keys, the one-word limit (K + 1 = 32), two-word keys
BIG = (1 << 32) - 1                   # a multiplicity the device refuses (it keeps such counts elsewhere)
BIG_DEVICE = (1 << 32) - 2            # the largest it takes


def _rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class Pieces:
    def __init__(self, K, seed=0):
        self.K = K
        self.rng = random.Random(7919 * K + seed)

    def rnd(self, n):
        return "".join(self.rng.choice("ACGT") for _ in range(n))

    def other(self, *chs):
        return self.rng.choice([c for c in "ACGT" if c not in chs])

    def long(self):
        return self.rnd(2 * self.K + 5)

    # ---- trim-paths ------------------------------------------------------------------------------------------------

    # A long path (left + B + right, multiplicity 5) and a spur of `edges` edges that ENTERS it at node B from a source
    # of its own.  Starts: the path's left end and, on the other strand, its right end (both walk more than 2K edges
    # before B's second in-edge resp. rc(B)'s second out-edge stops them: too_long) and the spur's first edge, which
    # walks `edges` edges to B (in-degree 2).  On the other strand the spur leaves rc(B), whose in-degree is 1: no start.
    # `mults`: one multiplicity per spur edge, first to last.
    def spur_in(self, edges, mults=None, cutoff=None):
        K = self.K
        t = self.rnd(edges + K)                                  # the spur and, as its last K bases, B
        b = t[edges:]
        left, right = self.long() + self.other(t[edges - 1]), self.long()
        return self._spur(t, left + b + right, edges, mults, cutoff)

    # The same spur attached by its beginning: it LEAVES the path at B and ends nowhere.  On this strand its first
    # edge's from-node B has an incoming edge, so it is no start; it goes only because its free end is a source on the
    # other strand, from where the walk enters rc(B) (in-degree 2).
    def spur_out(self, edges, mults=None, cutoff=None):
        K = self.K
        t = self.rnd(edges + K)
        b = t[:K]
        left, right = self.long(), self.other(t[K]) + self.long()
        return self._spur(t, left + b + right, edges, mults, cutoff)

    def _spur(self, t, path, edges, mults, cutoff):
        K = self.K
        mults = mults or [2] * edges
        assert len(mults) == edges
        strings = [(path, 5)] + [(t[j:j + K + 1], mults[j]) for j in range(edges)]
        expect = {"candidates": 3, "too_long": 2}
        if edges > 2 * K:
            expect["too_long"] = 3
        elif cutoff is not None and max(mults) >= cutoff:
            expect["spared_by_cutoff"] = 1
        else:
            expect.update(paths=1, zapped=2 * edges, removed=2 * edges)
        return strings, expect

    # A lone path of l <= 2K edges.  Both strands are starts, each removes all 2 l edges: zapped = 4 l, really gone 2 l.
    # Alone in a graph this is the zapCount > z case (z = 2 l).
    def isolated(self, l, mult=4):
        return [(self.rnd(self.K + l), mult)], {"candidates": 2, "paths": 2, "zapped": 4 * l, "removed": 2 * l}

    # Two branches that leave a source N (out-degree 2) and meet again K + 1 edges later, then a long common tail.
    # Both first edges are starts (in(N) = 0) whose walks end at the meeting node (in-degree 2) after K + 1 <= 2K
    # edges: both go, whatever their out-degree at N -- prune-tips keeps them as joined at both ends.  The tail, walked
    # from its free end on the other strand, is too long.
    def source_bubble(self, mult=6):
        K = self.K
        n, z = self.rnd(K), self.rnd(3 * K + 5)
        return ([(n + "A" + z, mult), (n + "C" + z, mult)],
                {"candidates": 3, "paths": 2, "too_long": 1, "zapped": 2 * 2 * (K + 1), "removed": 2 * 2 * (K + 1)})

    # u + rc(u): the text is its own reverse complement, so the path's mirror image is the path itself, edge j being
    # the reverse complement of edge l - 1 - j (for even K + 1 the middle edge is its own).  One start, for both strands
    # are the same strand; zapped = 2 l where l edges go.  l = 7 or 8, whichever makes l + K even.
    def palindrome(self, mult=7):
        K = self.K
        l = 7 + (K % 2 == 0)
        u = self.rnd((l + K) // 2)
        return [(u + _rc_text(u), mult)], {"candidates": 1, "paths": 1, "zapped": 2 * l, "removed": l}

    # A cycle: no node without an incoming edge, no fork: no start for either command.
    def cycle(self, length=9, mult=3):
        t = self.rnd(length)
        return [(t + t[:self.K], mult)] if length >= self.K else [(t * (self.K // length + 2), mult)], {"candidates": 0}

    # ---- clip-links ------------------------------------------------------------------------------------------------

    # A link of l edges and multiplicity c from node A on one long path to node B on another.  `outs` are the
    # multiplicities of the other edges that leave A (the first is the path's own, the others long dead-end
    # branches), `ins` of the other edges that enter B.  Starts: every edge out of A and, on the other strand, every
    # edge out of rc(B): len(outs) + len(ins) + 2.  All but the link and its mirror image walk a long stretch.
    #   link:    too_long if l > 2K; else major_out unless 3 c < S_out; else major_in unless 3 c < S_in
    #   mirror:  the same with the two sums exchanged (its fork is rc(B), its join rc(A))
    # with S_out = (c + sum(outs)) mod 2^32 and S_in = (c + sum(ins)) mod 2^32, a sum of 0 being "not minor".
    def link(self, l, c, outs, ins):
        K = self.K
        t = self.rnd(l + K)
        a, b = t[:K], t[l:]
        used_out, used_in = [t[K]], [t[l - 1]]
        strings = [(t, c)]
        for j, m in enumerate(outs):
            ch = self.other(*used_out)
            used_out.append(ch)
            strings.append(((self.long() if j == 0 else "") + a + ch + self.long(), m))
        for j, m in enumerate(ins):
            ch = self.other(*used_in)
            used_in.append(ch)
            strings.append((self.long() + ch + b + (self.long() if j == 0 else ""), m))
        s_out, s_in = (c + sum(outs)) % (1 << 32), (c + sum(ins)) % (1 << 32)
        expect = {"candidates": len(outs) + len(ins) + 2, "too_long": len(outs) + len(ins)}
        for first, second in ((s_out, s_in), (s_in, s_out)):
            if l > 2 * K:
                expect["too_long"] += 1
            elif not (first != 0 and 3 * c < first):
                expect["major_out"] = expect.get("major_out", 0) + 1
            elif not (second != 0 and 3 * c < second):
                expect["major_in"] = expect.get("major_in", 0) + 1
            else:
                expect["links"] = expect.get("links", 0) + 1
                expect["edges"] = expect.get("edges", 0) + l
        expect["removed"] = 2 * l if expect.get("links") else 0
        return strings, expect

    # A branch of l edges and multiplicity c that leaves a long path (multiplicity p) at A and ends nowhere: the node
    # it ends in has ONE incoming edge, so S_in = c, c / c = 1 and the branch stays however weak it is at the fork.
    # Starts: the two edges out of A; the other strand has no fork (rc(A) has one outgoing edge).
    def dead_end(self, l, c, p):
        K = self.K
        t = self.rnd(l + K)
        strings = [(t, c), (self.long() + t[:K] + self.other(t[K]) + self.long(), p)]
        assert 3 * c < c + p
        return strings, {"candidates": 2, "too_long": 1, "major_in": 1, "removed": 0}

    # K + 1 even.  One edge w = h + rc(h) that is its own reverse complement leaves A, on a long path of multiplicity p,
    # and enters rc(A): a link of one edge that is its own mirror image.  The edges that enter rc(A) are w and the
    # reverse complement of the path's edge out of A, so S_in = S_out = c + p.  Starts: the two edges out of A, and
    # the other strand's fork is the same node.  links = 1, edges = 1, one edge gone.
    def self_link(self, c, p):
        K = self.K
        assert (K + 1) % 2 == 0
        h = self.rnd((K + 1) // 2)
        w = h + _rc_text(h)
        strings = [(w, c), (self.long() + w[:K] + self.other(w[K]) + self.long(), p)]
        assert 3 * c < c + p
        return strings, {"candidates": 2, "too_long": 1, "links": 1, "edges": 1, "removed": 1}

    # A source that forks into dead ends of 3 edges with the given multiplicities: len(mults) starts, none on the other
    # strand; every branch ends in a node with one incoming edge, so none goes: major_out where 3 c >= S, else major_in.
    def source_fork(self, mults):
        n = self.rnd(self.K)
        strings = [(n + "ACGT"[j] + self.rnd(2), m) for j, m in enumerate(mults)]
        s = sum(mults)
        out = sum(1 for m in mults if not 3 * m < s)
        return strings, {"candidates": len(mults), "major_out": out, "major_in": len(mults) - out, "removed": 0}

    # Two branches of multiplicities 1 and 5 from a source N to a meeting node M, K + 1 edges each, and a tail of 3
    # edges: S_out at N = S_in at M = 6.  The weak branch goes on both strands (3 < 6), the strong one stays (15 >= 6).
    def bubble(self):
        K = self.K
        n, m = self.rnd(K), self.rnd(K)
        strings = [(n + "A" + m, 1), (n + "C" + m, 5), (m + self.rnd(3), 6)]
        return strings, {"candidates": 4, "links": 2, "edges": 2 * (K + 1), "major_out": 2, "removed": 2 * (K + 1)}


TRIM_FIELDS = ("candidates", "paths", "zapped", "too_long", "spared_by_cutoff")
CLIP_FIELDS = ("candidates", "links", "edges", "too_long", "major_out", "major_in")


class Case:
    """One graph and what one pass of `cmd` ("trim" or "clip") finds in it.  expect is None where only the model's two
    forms and the device are held to each other (the dense graphs, prune-tips' combined graph)."""

    def __init__(self, name, cmd, K, edges, counts, expect=None, cutoff=None, tags=(), device=True):
        self.name, self.cmd, self.K, self.edges, self.counts = name, cmd, K, edges, counts
        self.expect, self.cutoff, self.tags, self.device = expect, cutoff, tuple(tags), device

    def __repr__(self):
        return self.name


def _case(name, cmd, K, piece, cutoff=None, tags=(), device=True):
    strings, expect = piece
    edges, counts = graph_of(strings, K)
    return Case("%s_k%d_%s" % (cmd, K, name), cmd, K, edges, counts, expect, cutoff, tags, device)


def trim_cases(K):
    out = []

    def add(name, make, cutoff=None, tags=()):
        out.append(_case(name, "trim", K, make(Pieces(K, len(out))), cutoff, (name,) + tuple(tags)))

    add("len_2K", lambda p: p.spur_in(2 * K))
    add("len_2K+1", lambda p: p.spur_in(2 * K + 1))
    add("len_1", lambda p: p.spur_in(1))
    add("isolated", lambda p: p.isolated(6), tags=("undefined_estimate",))
    add("source_into_path", lambda p: p.spur_in(K))
    add("attached_by_its_end", lambda p: p.spur_out(K))
    add("source_bubble", lambda p: p.source_bubble())
    add("palindrome", lambda p: p.palindrome(), tags=("undefined_estimate",))
    add("cycle", lambda p: p.cycle())
    # the cutoff flag: the one edge of multiplicity 9 among edges of 2 is the first, the last or a middle one; a cutoff of
    # 9 spares the path, a cutoff of 10 does not
    for where, at in (("first", 0), ("last", 4), ("middle", 2)):
        mults = [2] * 5
        mults[at] = 9
        for cutoff in (9, 10):
            add("cutoff_%s_%d" % (where, cutoff), lambda p, m=mults, c=cutoff: p.spur_in(5, m, c), cutoff,
                ("cutoff_spares" if cutoff == 9 else "cutoff_passes",))
        add("cutoff_%s_out" % where, lambda p, m=mults: p.spur_out(5, m, 9), 9, ("cutoff_spares",))
    return out


def clip_cases(K):
    out = []

    def add(name, make, tags=(), device=True):
        out.append(_case(name, "clip", K, make(Pieces(K, 100 + len(out))), None, (name,) + tuple(tags), device))

    # a third exactly on either side (c = 1, S = 3: stays), just under on both (S = 4: goes)
    add("third_at_fork", lambda p: p.link(K, 1, [2], [3]))
    add("third_at_join", lambda p: p.link(K, 1, [3], [2]))
    add("under_a_third", lambda p: p.link(K, 1, [3], [3]))
    add("major_at_fork", lambda p: p.link(K, 4, [5], [20]))
    add("major_at_join", lambda p: p.link(K, 4, [20], [5]))
    add("major_at_both", lambda p: p.link(K, 4, [5], [5]))
    for d in (2, 3, 4):
        add("out_degree_%d" % d, lambda p, d=d: p.link(3, 2, [3] * (d - 1), [9]))
        add("in_degree_%d" % d, lambda p, d=d: p.link(3, 2, [9], [3] * (d - 1)))
    add("out_degree_4_major", lambda p: p.link(3, 2, [1, 1, 1], [9]))
    add("in_degree_1", lambda p: p.dead_end(4, 1, 9))
    add("len_1", lambda p: p.link(1, 1, [5], [5]))
    add("len_2K", lambda p: p.link(2 * K, 1, [5], [5]), tags=("mirror_passes",))
    add("len_2K+1", lambda p: p.link(2 * K + 1, 1, [5], [5]))
    if (K + 1) % 2 == 0:                               # (no edge of odd length is its own reverse complement)
        add("self_link", lambda p: p.self_link(1, 5))
    # sums that wrap.  3 (2^32 - 1) + 1 = 3 * 2^32 - 2 -> 2^32 - 2, and 3 * 1 < 2^32 - 2: minor;
    # 3 (2^32 - 2) + 1 = 3 * 2^32 - 5 -> 2^32 - 5: minor.  Exactly 0: 2 + 2 (2^32 - 1) = 2^33 and 4 + 2 (2^32 - 2) = 2^33:
    # not minor, where the unwrapped sum would have made the link minor by far.
    add("wrap_out_big", lambda p: p.link(3, 1, [BIG] * 3, [3]), tags=("wrap",), device=False)
    add("wrap_in_big", lambda p: p.link(3, 1, [3], [BIG] * 3), tags=("wrap",), device=False)
    add("wrap_zero_big", lambda p: p.link(3, 2, [BIG] * 2, [5]), tags=("wrap_zero",), device=False)
    add("wrap_out", lambda p: p.link(3, 1, [BIG_DEVICE] * 3, [3]), tags=("wrap",))
    add("wrap_in", lambda p: p.link(3, 1, [3], [BIG_DEVICE] * 3), tags=("wrap",))
    add("wrap_zero_out", lambda p: p.link(3, 4, [BIG_DEVICE] * 2, [9]), tags=("wrap_zero",))
    add("wrap_zero_in", lambda p: p.link(3, 4, [9], [BIG_DEVICE] * 2), tags=("wrap_zero",))
    add("cycle", lambda p: p.cycle())
    return out


# Graphs with a given number of starts, at the wave (64) and workgroup (256) edges of the per-wave report adds and of
# the gather.  trim-paths: lone paths of 3 edges (2 starts each) and one palindrome (1).  clip-links: a fork has two or
# more outgoing edges, so a graph has no ONE start: bubbles (4 starts each), a source fork of two (2) and of three (3).
CANDIDATE_COUNTS = (0, 1, 63, 64, 65, 256, 257)


def _combine(parts):
    strings = [s for part, _ in parts for s in part]
    fields = set(f for _, e in parts for f in e)
    return strings, {f: sum(e.get(f, 0) for _, e in parts) for f in fields}


def count_case(cmd, K, want):
    p = Pieces(K, 5000 + want)
    if cmd == "trim":
        parts = [p.isolated(3) for _ in range(want // 2)] + ([p.palindrome()] if want % 2 else [])
        if not parts:
            parts = [p.cycle()]
    else:
        if want == 1:
            return None
        rest, parts = want, []
        if rest % 2:
            parts.append(p.source_fork([1, 1, 7]))
            rest -= 3
        if rest % 4:
            parts.append(p.source_fork([1, 7]))
            rest -= 2
        parts += [p.bubble() for _ in range(rest // 4)]
        if not parts:
            parts = [(p.isolated(3)[0], {"candidates": 0})]
    strings, expect = _combine(parts)
    assert expect["candidates"] == want
    edges, counts = graph_of(strings, K)
    return Case("%s_k%d_starts_%d" % (cmd, K, want), cmd, K, edges, counts, expect, None, ("starts_%d" % want,))


_corpus = []


def corpus():
    """Every case: the pieces and the start counts at K = 15, 31, 32, both commands over the dense graphs (K = 1 .. 5)
    and over prune-tips' combined graph."""
    if _corpus:
        return _corpus
    import dense_graphs
    import tips_cases
    for K in KS:
        _corpus.extend(trim_cases(K))
        _corpus.extend(clip_cases(K))
        for cmd in ("trim", "clip"):
            for want in CANDIDATE_COUNTS:
                c = count_case(cmd, K, want)
                if c:
                    _corpus.append(c)
            edges, counts, _ = tips_cases.combined_graph(K)
            _corpus.append(Case("%s_k%d_tips_combined" % (cmd, K), cmd, K, edges, counts, tags=("tips_combined",)))
    for name, K, edges, counts in dense_graphs.corpus():
        for cmd in ("trim", "clip"):
            _corpus.append(Case("%s_dense_%s" % (cmd, name), cmd, K, edges, counts, tags=("dense",)))
    return _corpus
