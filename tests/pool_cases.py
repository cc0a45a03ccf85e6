"""The corpus of pool-samples: the smallest shapes at which pool_rows_kernel, pool_pairs_kernel and pool_positions_kernel
(gossamer_amd/csrc/kernels_pool.hpp) can go wrong.  Every case is planned (pool_model.py): z masks of S bits, so the
expected rows are known by construction.

  z     1, 63, 64, 65 (a word and its neighbours), 4095, 4096, 4097, and the last size that one visit of a workgroup
        of pool_pairs_kernel (POOL_PAIR_WORDS words) / one workgroup of pool_positions_kernel (POOL_POS_WORDS words)
        covers and the first that needs a second one
  S     1, 2, 31, 32, 33 (one call of add_masks and its neighbours), 63, 64, 65 (POOL_TILE rows of the pair tile and its
        neighbours: the second tile, the tile pairs (0, 0) (0, 1) (1, 1))
  masks by sample index, mixed in every case with enough samples (KINDS): all ones, all zeros, the first k-mer only,
        the last k-mer only (the last bit of the last word: the padding beyond z stays 0), random, a copy of the random
        one (similarity exactly 1), its complement (0), a subset of it (nested), then random masks of growing density;
        the seed is fixed per case
  slabs every case is added in calls of up to 32 samples and again in an odd partition: calls of 1, 31 and 32 samples
        with first_set not a multiple of 32, given out of order, with bits set above nbits that must be ignored

Two cases exist for the text only: third (a pair with inter / union = 1 / 3) and tiny (1 / 100000, which a stream prints
as 1e-05).  The second needs 100 000 k-mers -- of two samples: a fifth of the bits of the largest case, 65 x 8 193.

The command's cases carry keys as well (K = 25, and 31 / 32 / 33 for the one-word / two-word forms): S = 3, S = 9 (more
than --max-merge 8: the staged union), S = 33 and S = 65 (the slabs with the union merged in); among the samples an empty
one, a duplicate, and one object named twice."""
import random
from collections import namedtuple

from gossamer_amd.binding import POOL_PAIR_WORDS, POOL_POS_WORDS, POOL_TILE

import pool_model as pm

CmdCase = namedtuple("CmdCase", "name K keys masks nsets twice")          # twice: (i, j) sample j is sample i's object named again

Z_WORD = (1, 63, 64, 65)
Z_4096 = (4095, 4096, 4097)
Z_PAIR_BLOCK = (POOL_PAIR_WORDS * 64, POOL_PAIR_WORDS * 64 + 1)
Z_POS_BLOCK = (POOL_POS_WORDS * 64, POOL_POS_WORDS * 64 + 1)
ZS = tuple(sorted(set(Z_WORD + Z_4096 + Z_PAIR_BLOCK + Z_POS_BLOCK)))
S_CALL = (1, 2, 31, 32, 33)
S_TILE = (POOL_TILE - 1, POOL_TILE, POOL_TILE + 1)
SS = tuple(sorted(set(S_CALL + S_TILE)))
MAX_SETS, MAX_Z = 65, 8193

KINDS = ("ones", "zeros", "first", "last", "random", "copy", "complement", "nested")


def kinds_of(nsets):
    """the mask kinds a case of nsets samples mixes"""
    return frozenset(KINDS[:nsets]) | (frozenset({"random"}) if nsets > len(KINDS) else frozenset())


def _density(rng, z, d):
    """a random z-bit row of density d / 8: three random bit planes read as a number n per position, the bit set where n < d"""
    full = (1 << z) - 1
    a, b, c = rng.getrandbits(z), rng.getrandbits(z), rng.getrandbits(z)
    d2, d1, d0 = (full if d & 4 else 0), (full if d & 2 else 0), (full if d & 1 else 0)
    lt0 = ~c & d0
    lt1 = (~b & d1) | (~(b ^ d1) & lt0)
    return ((~a & d2) | (~(a ^ d2) & lt1)) & full


def plan_rows(nsets, z, seed):
    """row i (a Python integer, bit r: k-mer r is in sample i) is of kind KINDS[i]; samples beyond them are random rows of
    density (i % 7 + 1) / 8"""
    rng = random.Random(seed)
    full = (1 << z) - 1
    base = rng.getrandbits(z)
    rows = []
    for i in range(nsets):
        kind = KINDS[i] if i < len(KINDS) else "random"
        if kind == "ones":
            r = full
        elif kind == "zeros":
            r = 0
        elif kind == "first":
            r = 1
        elif kind == "last":
            r = 1 << (z - 1)
        elif kind in ("copy", "random") and i < len(KINDS):
            r = base
        elif kind == "complement":
            r = full & ~base
        elif kind == "nested":
            r = base & rng.getrandbits(z)
        else:
            r = _density(rng, z, i % 7 + 1)
        rows.append(r)
    return rows


def masks_of_rows(rows, z):
    """one mask per k-mer (bit i: in sample i) from the rows"""
    import numpy as np
    lo = np.zeros(z, dtype=np.uint64)
    hi = np.zeros(z, dtype=np.uint64)
    for i, r in enumerate(rows):
        bits = np.unpackbits(np.frombuffer(r.to_bytes((z + 7) // 8, "little"), dtype=np.uint8), bitorder="little")[:z].astype(np.uint64)
        if i < 64:
            lo |= bits << np.uint64(i)
        else:
            hi |= bits << np.uint64(i - 64)
    return [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]


def plan_masks(nsets, z, seed):
    return masks_of_rows(plan_rows(nsets, z, seed), z)


class Case:
    """name, nsets, z, tags; masks are planned when first asked for"""

    def __init__(self, name, nsets, z, tags, seed=None, masks=None):
        self.name, self.nsets, self.z, self.tags, self._seed, self._masks = name, nsets, z, tags, seed, masks

    @property
    def masks(self):
        if self._masks is None:
            self._masks = plan_masks(self.nsets, self.z, self._seed)
        return self._masks


def _library_cases():
    out = []
    pairs = []
    for n, z in enumerate(ZS):                                   # every z, with two S each that walk through SS
        pairs += [(SS[n % len(SS)], z), (SS[(n + 4) % len(SS)], z)]
    for s in SS:                                                 # every S at a z off the word and at the largest z
        pairs += [(s, 65), (s, MAX_Z)]
    seen = set()
    for s, z in pairs:
        if (s, z) in seen:
            continue
        seen.add((s, z))
        out.append(Case("s%d_z%d" % (s, z), s, z, kinds_of(s), seed=1000 * s + z))
    # the text: 1 / 3, and 1 / 100000
    out.append(Case("third", 2, 3, frozenset({"third"}), masks=[1, 3, 2]))
    out.append(Case("tiny", 2, 100000, frozenset({"tiny"}), masks=[3] + [1] * 49999 + [2] * 50000))
    return out


CASES = _library_cases()
_BY_NAME = {c.name: c for c in CASES}


def names():
    return [c.name for c in CASES]


def case(name):
    return _BY_NAME[name]


def slabs_whole(nsets):
    """calls of up to 32 samples, in order"""
    return [(f, min(32, nsets - f)) for f in range(0, nsets, 32)]


def slabs_odd(nsets):
    """calls of 1, 31, 32, 1, 31, 32 ... samples (the last one cut), last call first"""
    out, f, sizes = [], 0, (1, 31, 32)
    while f < nsets:
        n = min(sizes[len(out) % 3], nsets - f)
        out.append((f, n))
        f += n
    return out[::-1]


# ---- the command ----------------------------------------------------------------------------------------------------------

def _keys(K, n, seed):
    rng = random.Random(seed)
    ks = set()
    while len(ks) < n:
        ks.add(rng.getrandbits(2 * K))
    ks = sorted(ks)
    ks[0], ks[-1] = 0, (1 << (2 * K)) - 1                        # both ends of the key space: every word of a two-word key in use
    return ks


def _cmd_case(name, K, nsets, z, seed, twice=None):
    """a planned case whose keys are all in some sample (the union is the keys), with an empty sample from S = 9 on"""
    masks = plan_masks(nsets, z, seed)
    if nsets <= 3:
        # ones / zeros / first would leave nothing to compare: three overlapping random samples instead
        rng = random.Random(seed)
        masks = [rng.randrange(1, 8) for _ in range(z)]
    return CmdCase(name, K, _keys(K, z, seed + 1), masks, nsets, twice)


CMD_CASES = [
    _cmd_case("cmd_s3_k31", 31, 3, 200, 31),
    _cmd_case("cmd_s3_k32", 32, 3, 200, 32),
    _cmd_case("cmd_s3_k33", 33, 3, 200, 33),
    _cmd_case("cmd_s9", 25, 9, 300, 9, twice=(4, 8)),
    _cmd_case("cmd_s33", 25, 33, 300, 330),
    _cmd_case("cmd_s65", 25, 65, 500, 650, twice=(10, 64)),
]
_CMD_BY_NAME = {c.name: c for c in CMD_CASES}


def cmd_names():
    return [c.name for c in CMD_CASES]


def cmd_case(name):
    return _CMD_BY_NAME[name]


def cmd_samples(c):
    """the samples of a command case as lists of keys; with `twice` = (i, j), sample j is sample i"""
    samples = pm.planned_samples(c.keys, c.masks, c.nsets)
    if c.twice:
        samples[c.twice[1]] = list(samples[c.twice[0]])
    return samples
