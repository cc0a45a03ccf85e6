"""The fixtures the match tests share: (name, K, graph?, normalize?, seed).  The seeds were chosen on the CPU so that
every fixture's input is not vacuous (test_match_cpu.py checks it): between 20 % and 80 % of the reads match, and at
least one read has some but not all of its windows in the object."""
import functools

import match_model as mm

CASES = [
    ("graph27", 27, True, False, 11),
    ("graph40", 40, True, False, 12),
    ("kmers25", 25, False, False, 13),
    ("kmers25n", 25, False, True, 13),
    ("kmers33n", 33, False, True, 14),
]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(K, graph, normalize, L, the reads the object is built from, the object's keys, the bytes to match)"""
    _, K, graph, normalize, seed = next(c for c in CASES if c[0] == name)
    L = K + 1 if graph else K
    gen, built = mm.build_reads(seed)
    # (every second fixture ends without its '\n')
    query = mm.query_reads(seed, gen, L, trailing_newline=seed % 2 == 1)
    return K, graph, normalize, L, built, mm.object_keys(built, K, graph), query


@functools.lru_cache(maxsize=None)
def expected(name, any_mode):
    K, graph, normalize, L, built, keys, query = fixture(name)
    return mm.match(query, L, keys, normalize=normalize, any=any_mode)
