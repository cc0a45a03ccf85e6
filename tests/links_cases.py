"""The corpus of the read link tests: graphs, reads over them, and per case the condition it exists for.

Graphs
  dense     the 40 graphs of dense_graphs.py (K = 1 .. 5, up to 4 096 edges).  Their reads hold every possible window:
            a de Bruijn sequence of order K + 1 as one read (4^(K+1) + K bases: at K = 5 it spans three tiles of the
            window kernel), the same sequence cut into overlapping reads of 37 bases, and 600 bases of it (repeated where it is shorter) with 'N's, lower
            case, an empty line and a '\\r'.
  planted   K = 30, 31 (one-word keys) and 62 (two-word keys), made of random strings (seeded; at these K two random
            strings share no K-mer by chance) so that the graph holds
              a join         X1 + J and X2 + J: the node where J begins has two edges in, one out
              a fork         J + Y1 and J + Y2
              a bubble       S + 'A' + T and S + 'C' + T
              a pure cycle   the windows of a circular string: every node one-in-one-out, no entry edge, no segment
              a homopolymer  A x (K + 3) + H: a self-loop that runs into a path
              a self-complementary edge   u + rc(u) in the middle of a string, where K + 1 is even (K = 31)
              a long contig  5 200 bases: reads around 2 048 bytes and one of 5 000 across the tiles
Every case is (name, batches, unique pattern (unique_of), condition): `condition(model, batches)` is what the case is there to show,
and test_links_cpu.py holds every case to it.  Everything here is plain Python and deterministic.
"""
import random

import dense_graphs as dg
import links_model as lm
import tips_model as tm

PLANTED_K = (30, 31, 62)
UNIQUE_PATTERNS = ("all", "none", "alternating", "last")
MANY = 70000


def rc_text(s):
    return s[::-1].translate(str.maketrans("ACGTacgtNn", "TGCAtgcaNn"))


def rand_text(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def de_bruijn(order):
    """a de Bruijn sequence over ACGT, as a string of 4^order + order - 1 bases that holds every window once"""
    a = [0] * (4 * order)
    seq = []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = "".join("ACGT"[c] for c in seq)
    return s + s[:order - 1]


def unique_of(pattern, entries, model=None):
    """the truth value per entry rank of a pattern, or None for "all"; ("without", text): every segment but that of
    the first window of `text`"""
    if isinstance(pattern, tuple):
        return [i != _seg(model, pattern[1]) for i in range(entries)]
    if pattern == "all":
        return None
    if pattern == "none":
        return [False] * entries
    if pattern == "alternating":
        return [i % 2 == 0 for i in range(entries)]
    return [i == entries - 1 for i in range(entries)]


# ---- dense ---------------------------------------------------------------------------------------------------------

def dense_reads(K):
    """the three batches of a dense graph"""
    s = de_bruijn(K + 1)
    cut = "\n".join(s[i:i + 37] for i in range(0, len(s) - K, 37 - K)) + "\n"
    odd = list((s * (600 // len(s) + 1))[:600])
    for i in range(11, len(odd), 53):
        odd[i] = "N" if i % 2 else "n"
    odd = "".join(odd)
    odd = odd[:200].lower() + "\n\n" + odd[200:400] + "\r\n" + "AC\n" + odd[400:]
    return [s + "\n", cut, odd]


def dense():
    """[(name, K, edges, counts, batches)]"""
    return [(name, K, edges, counts, dense_reads(K)) for name, K, edges, counts in dg.corpus()]


# ---- planted -------------------------------------------------------------------------------------------------------

_planted = {}


def planted(K):
    """dict(K, edges, counts, parts): parts maps a name to its string"""
    if K in _planted:
        return _planted[K]
    rng = random.Random(1000 + K)
    L = K + 1
    p = {}
    p["X1"], p["X2"], p["J"], p["Y1"], p["Y2"] = (rand_text(rng, K + 9) for _ in range(5))
    # (the join and the fork lie where the strings say: the bases next to them differ)
    p["X2"] = p["X2"][:-1] + "ACGT"[("ACGT".index(p["X1"][-1]) + 1) % 4]
    p["Y2"] = "ACGT"[("ACGT".index(p["Y1"][0]) + 1) % 4] + p["Y2"][1:]
    p["S"], p["T"] = rand_text(rng, K + 5), rand_text(rng, K + 5)
    p["R"] = rand_text(rng, 2 * K + 7)
    p["H"] = "C" + rand_text(rng, K + 6)
    p["contig"] = rand_text(rng, 5200)
    strings = [(p["X1"] + p["J"], 3), (p["X2"] + p["J"], 3), (p["J"] + p["Y1"], 3), (p["J"] + p["Y2"], 3),
               (p["S"] + "A" + p["T"], 2), (p["S"] + "C" + p["T"], 2),
               (p["R"] + p["R"][:K], 4), ("A" * (K + 3) + p["H"], 5), (p["contig"], 6)]
    if L % 2 == 0:
        u = rand_text(rng, L // 2)
        p["W"], p["V"] = rand_text(rng, K + 4), rand_text(rng, K + 4)
        p["self"] = p["W"] + u + rc_text(u) + p["V"]
        strings.append((p["self"], 7))
    # (a (K+1)-mer that two strings share comes with one multiplicity: X1 + J and J + Y1 share those of J)
    got = {}
    for text, mult in strings:
        for i in range(len(text) - K):
            e = tm.encode(text[i:i + L])
            got.setdefault(e, mult)
            got.setdefault(tm.revcomp(e, L), got[e])
    edges = sorted(got)
    _planted[K] = dict(K=K, edges=edges, counts=[got[e] for e in edges], parts=p)
    return _planted[K]


def _seg(model, text):
    """the segment of the first window of `text`"""
    return model.fresh(lm.windows_of(text, model.K)[0])


def _rows(model, batches, unique=None, carry=True):
    return lm.rows_of(model.read_links(batches, unique, carry)[0])


def _records(model, batches, unique=None, carry=True):
    return model.read_links(batches, unique, carry)[1]["records"]


def _unique_condition(m, b, pattern):
    """all: links; none: no hit; alternating: some windows hit and some that would do not; last: one unique segment
    alone makes no link"""
    info = m.read_links(b, unique_of(pattern, m.entries), False)[1]
    full = m.read_links(b, None, False)[1]
    return {"all": info["records"] > 0, "none": info["hits"] == 0, "alternating": 0 < info["hits"] < full["hits"],
            "last": info["records"] == 0}[pattern]


def planted_cases(K):
    """[(name, batches, unique pattern, condition)] over planted(K)"""
    g = planted(K)
    p = g["parts"]
    L = K + 1
    xj, jy1, jy2 = p["X1"] + p["J"], p["J"] + p["Y1"], p["J"] + p["Y2"]
    contig = p["contig"]
    a_piece, b_piece = p["X1"][:L + 3], p["Y1"][-(L + 3):]
    cross = jy1[len(p["J"]) - L:len(p["J"]) + 1]                  # two windows: the last edge of J, the first of Y1
    # the edge that enters the join from X1, an N, the edge that leaves the join: the only one out of its node
    join_n = xj[len(p["X1"]) - 1:len(p["X1"]) + K] + "N" + xj[len(p["X1"]):len(p["X1"]) + L]
    cases = []

    def add(name, batches, pattern, condition):
        cases.append((name, batches, pattern, condition))
        both = [("\n".join(rc_text(r) for r in b.split("\n"))) for b in batches]
        # the mirror reads walk the mirror segments backwards: in exact mode, every segment unique, as many records
        cases.append((name + "-rc", both, pattern, lambda m, b: _records(m, b, carry=False) == _records(m, batches, carry=False)))

    def differ(m, b):
        return _rows(m, b, carry=True) != _rows(m, b, carry=False)

    add("a-b", [jy1 + "\n"], "all", lambda m, b: _rows(m, b, carry=False) == [(_seg(m, p["J"]), _seg(m, p["Y1"][-L:]), 1, 0)])
    add("a-b-a", [a_piece + b_piece + a_piece + "\n"], "all",
        lambda m, b: [r[:3] for r in _rows(m, b)] == sorted([(_seg(m, a_piece), _seg(m, b_piece), 1), (_seg(m, b_piece), _seg(m, a_piece), 1)])
        and all(r[3] > 0 for r in _rows(m, b)))               # (misses in the middle: the windows over each seam)
    add("a-a", [a_piece + "N" + a_piece + "\n" + a_piece + b_piece[:K - 1] + a_piece + "\n"], "all", lambda m, b: _rows(m, b) == [])
    without_j = ("without", p["J"])                               # J's segment: its K + 9 - K = 9 edges, from the join to the fork
    add("non-unique-between", [xj + p["Y1"] + "\n"], without_j,
        lambda m, b: _rows(m, b, unique_of(without_j, m.entries, m), False) == [(_seg(m, p["X1"]), _seg(m, p["Y1"][-L:]), 1, 9)])
    add("join", [xj + "\n", jy2 + "\n"], "all", differ)
    add("join-lower-cr", [xj.lower() + "\r\n\n" + xj[:K] + "\n" + jy1], "all", differ)
    add("carry-across-n", [join_n + "\n"], "all",
        lambda m, b: m.thread_windows(b[0], carry=True) == [_seg(m, p["X1"][-L:])] * 2
        and m.thread_windows(b[0], carry=False)[1] == _seg(m, p["J"]))
    add("cycle-bubble-loop", [p["R"] + p["R"] + "\n" + p["S"] + "A" + p["T"] + "\n" + p["S"] + "C" + p["T"] + "\n" + "A" * (K + 9) + p["H"] + "\n"],
        "all", lambda m, b: lm.MISS in m.thread_windows(b[0], carry=False) and _records(m, b) >= 3)
    if "self" in p:
        add("self-complementary", [p["self"] + "\n" + rc_text(p["self"]) + "\n"], "all",
            lambda m, b: any(tm.revcomp(e, L) == e for e in lm.windows_of(p["self"], K)))
    add("around-2048", ["".join(contig[i:i + n] + "\n" for i, n in enumerate(range(2040, 2057)))], "all",
        lambda m, b: all(2040 <= len(r) <= 2056 for r in b[0].split("\n")[:-1]))
    add("long-read", [contig[:5000] + "\n" + cross + "\n"], "all", lambda m, b: len(b[0].split("\n")[0]) == 5000 and _records(m, b, carry=False) == 1)
    for n in (1, 63, 64, 65, 255, 256, 257):
        add("reads-%d" % n, [(a_piece + "\n") * (n - 1) + cross], "all",
            lambda m, b, n=n: m.read_links(b, carry=False)[1]["reads"] == n and _records(m, b, carry=False) == 1)
    for n in (0, 1, 63, 64, 65, 4095, 4096, 4097):
        add("records-%d" % n, [a_piece + "\n" + (cross + "\n") * n], "all", lambda m, b, n=n: _records(m, b, carry=False) == n)
    if K == PLANTED_K[0]:
        cases.append(("one-link-%d" % MANY, [(cross + "\n") * MANY], "all",
                      lambda m, b: [r[2] for r in _rows(m, b, carry=False)] == [MANY]))
    for pattern in UNIQUE_PATTERNS:
        add("unique-" + pattern, [xj + "\n" + jy1 + "\n" + a_piece + b_piece + "\n" + p["S"] + "A" + p["T"] + "\n" + p["S"] + "C" + p["T"] + "\n"
                                  + p["X2"] + p["J"] + p["Y2"] + "\n" + contig[:200] + "\n"], pattern,
            lambda m, b, pattern=pattern: _unique_condition(m, b, pattern))
    return cases
