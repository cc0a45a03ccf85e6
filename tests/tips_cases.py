"""Hand-made graphs for the prune-tips tests: pieces whose classification follows by construction.

Every piece is a list of (text, multiplicity) strings over random bases (seeded by K); tips_model.graph_of turns a
list of pieces into a sorted edge list that holds both strands.  `expect` is what ONE iteration finds in the piece,
argued in the comment beside it.  The counts come from the construction, never from running the code under test.
"""
import random

from tips_model import graph_of


def _rc_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class Pieces:
    def __init__(self, K, seed=0):
        self.K = K
        self.rng = random.Random(1000 * K + seed)

    def rnd(self, n):
        return "".join(self.rng.choice("ACGT") for _ in range(n))

    def other(self, ch):
        return self.rng.choice([c for c in "ACGT" if c != ch])

    # A node without incoming edges that forks into two dead-end branches of K + 3 edges, multiplicities a and b.
    # Candidates: each branch's first edge (joined at the beginning: out(N) = 2) and, on the other strand, each
    # branch walked from its free end into rc(N) (joined at the end: in(rc N) = 2).  The attaching node is N in all
    # four cases and its edges carry a and b: a branch goes iff the other one is not weaker.
    def fork(self, a, b):
        K = self.K
        n = self.rnd(K)
        strings = [(n + "A" + self.rnd(K + 2), a), (n + "C" + self.rnd(K + 2), b)]
        cut = (a <= b) + (b <= a)                     # branches removed (both on a tie)
        expect = {"candidates": 4, "joined_at_begin": cut, "joined_at_end": cut, "tips": 2 * cut,
                  "outweighed": 4 - 2 * cut, "zapped": 2 * cut * 2 * (K + 3), "removed": cut * 2 * (K + 3)}
        return strings, expect

    # A path of multiplicity `path` with more than 2K edges on either side of a node B, and a spur of `edges` edges
    # and multiplicity `spur` that leaves B.  The path's two ends are candidates that walk more than 2K edges
    # (too_long) before B's second out-edge (resp. rc(B)'s second in-edge) stops them.  The spur's free end, seen
    # from the other strand, is a candidate that walks `edges` edges into rc(B) (in-degree 2: joined at the end);
    # the attaching node is B, whose out-edges carry `path` and `spur`.
    def spur(self, edges, spur, path):
        K = self.K
        left, b, right = self.rnd(2 * K + 5), self.rnd(K), self.rnd(2 * K + 6)
        s = b + self.other(right[0]) + self.rnd(edges - 1)
        expect = {"candidates": 3, "too_long": 2}
        if edges > 2 * K:
            expect["too_long"] = 3
        elif path < spur:
            expect["outweighed"] = 1
        else:
            expect.update(joined_at_end=1, tips=1, zapped=2 * edges, removed=2 * edges)
        return [(left + b + right, path), (s, spur)], expect

    # Two branches that leave a node without incoming edges and meet again K + 1 edges later (one differing base),
    # then a common tail of 2K + 5 edges.  Either branch's first edge is a candidate joined at both ends
    # (out(N) = 2, in(meeting node) = 2); the tail, walked from its free end on the other strand, is too long.
    def source_bubble(self, mult):
        K = self.K
        n, z = self.rnd(K), self.rnd(3 * K + 5)
        return [(n + "A" + z, mult), (n + "C" + z, mult)], {"candidates": 3, "both_joined": 2, "too_long": 1}

    # A lone path of 6 edges: its two ends (one per strand) are candidates joined nowhere.
    def isolated(self, mult):
        return [(self.rnd(self.K + 6), mult)], {"candidates": 2, "isolated": 2}

    # K + 1 even.  An edge w that is its own reverse complement joins the strand it lies on to the other strand:
    # to(w) = rc(from(w)).  A path through w is therefore its own mirror image, its two ends are joined alike, and
    # it can never be a tip -- but a walk can cross w, and the link arrays must hold rank(rc w) = rank(w).
    #  * lone_palindrome: u + rc(u), 7 edges, the middle one self-complementary: ONE candidate (both strands are the
    #    same strand), isolated.
    #  * hairpin: a spur that leaves a long path at B and ends in w comes back on the other strand into rc(B): it has
    #    no free end, hence no candidate of its own; the path's ends are too_long as in spur().
    def lone_palindrome(self, mult):
        assert (self.K + 1) % 2 == 0
        u = self.rnd((self.K + 1) // 2 + 3)
        return [(u + _rc_text(u), mult)], {"candidates": 1, "isolated": 1}

    def hairpin(self, spur, path):
        K = self.K
        assert (K + 1) % 2 == 0
        left, b, right = self.rnd(2 * K + 5), self.rnd(K), self.rnd(2 * K + 6)
        h = self.rnd((K + 1) // 2)
        s = b + self.other(right[0]) + self.rnd(3) + h + _rc_text(h)
        return [(left + b + right, path), (s, spur)], {"candidates": 2, "too_long": 2}


FIELDS = ("candidates", "tips", "zapped", "too_long", "both_joined", "isolated", "outweighed", "joined_at_begin",
          "joined_at_end")


def combined(K):
    """(strings, expected report fields of iteration 1, edges really removed by it) of all the pieces side by side."""
    p = Pieces(K)
    parts = [p.fork(3, 5), p.spur(2 * K, 2, 5), p.spur(2 * K + 1, 2, 5), p.spur(K, 9, 5), p.source_bubble(6), p.isolated(4)]
    if (K + 1) % 2 == 0:
        parts += [p.lone_palindrome(7), p.hairpin(2, 5)]
    strings = [s for part, _ in parts for s in part]
    expect = {f: sum(e.get(f, 0) for _, e in parts) for f in FIELDS + ("removed",)}
    return strings, expect


def combined_graph(K):
    strings, expect = combined(K)
    edges, counts = graph_of(strings, K)
    return edges, counts, expect


def error_reads(genome_len, coverage, error_rate, seed, read_len=100, repeat=300):
    """Reads of both strands with substituted bases off a random genome that holds one planted repeat: the text
    build-graph takes as line input (one read per line)."""
    rng = random.Random(seed)
    g = [rng.choice("ACGT") for _ in range(genome_len)]
    at = genome_len // 5
    g[3 * at:3 * at + repeat] = g[at:at + repeat]
    g = "".join(g)
    lines = []
    for _ in range(genome_len * coverage // read_len):
        p = rng.randrange(genome_len - read_len + 1)
        r = g[p:p + read_len]
        if rng.random() < 0.5:
            r = _rc_text(r)
        r = "".join(rng.choice([c for c in "ACGT" if c != ch]) if rng.random() < error_rate else ch for ch in r)
        lines.append(r)
    return "\n".join(lines) + "\n"
