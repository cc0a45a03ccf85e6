"""compute-near-kmers without a device: the model of the reference's loop (tests/near_model.py) on cases worked out by
hand at K = 3, the equivalence of the reference's 3K masks and the 2K + 1 distinct ones the kernel walks, the bitmap
helpers against the files the oracle's merge-and-annotate writes, and the command's usage errors.

K = 3: a key has 6 bits, base 0 in bits 5-4, base 1 in bits 3-2, base 2 in bits 1-0 (A=0 C=1 G=2 T=3).
The reference's masks b << j (j = 0..2, b = 1..3) are 1 2 3 | 2 4 6 | 4 8 12: bits 0..3 only -- base 0 is never touched,
and 6 = 0110 straddles bases 1 and 2.  GOSS_NEAR_WHOLE_BASES: b << 2j = 1 2 3 | 4 8 12 | 16 32 48.
Every case is run under the four flag combinations, in the order (default, NORMALIZE, WHOLE_BASES, both)."""
import os
import random
import subprocess

import pytest

import near_model as nm
import oracle_lib as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
K = 3
FLAGS = [(False, False), (False, True), (True, False), (True, True)]          # (whole_bases, normalize)
L, R, BOTH, NONE = (1, 0), (0, 1), (1, 1), (0, 0)


def run_case(members):
    """members: {k-mer string: (lhs bit, rhs bit)}, every k-mer canonical as stored -> per flag combination
    ({k-mer: new (lhs, rhs)}, gray)"""
    names = sorted(members, key=o.kmer_value)
    keys = [o.kmer_value(s) for s in names]
    for s, v in zip(names, keys):
        assert o.normalize(v, K) == v, "%s is not the form a k-mer set stores" % s
    lhs = [members[s][0] for s in names]
    rhs = [members[s][1] for s in names]
    out = []
    for wb, nz in FLAGS:
        nl, nr, gray = nm.near_kmers(keys, lhs, rhs, K, whole_bases=wb, normalize=nz)
        out.append(({s: (a, b) for s, a, b in zip(names, nl, nr)}, gray))
    return out


def test_the_masks_at_k3():
    assert nm.reference_masks(3) == [1, 2, 3, 2, 4, 6, 4, 8, 12]
    assert nm.reference_masks(3, whole_bases=True) == [1, 2, 3, 4, 8, 12, 16, 32, 48]
    assert sorted(nm.distinct_masks(3)) == [1, 2, 3, 4, 6, 8, 12]           # 2K + 1 = 7: bits 0..3, pairs 3<<0, 3<<1, 3<<2
    for k in (1, 2, 3, 5, 25, 31, 32, 63):
        assert sorted(set(nm.reference_masks(k))) == sorted(nm.distinct_masks(k)) and len(nm.distinct_masks(k)) == 2 * k + 1
        assert max(nm.reference_masks(k)).bit_length() == k + 1             # bits 0 .. K
        assert max(nm.reference_masks(k, True)).bit_length() == 2 * k       # always a valid key


def test_pair_that_differs_in_the_last_base():
    # AGA = 001000 (left only), AGC = 001001 (right only): AGA ^ 1 == AGC, mask 1 is in both families, and AGC is
    # canonical as it stands, so the plain lookup sees it; normalising changes nothing.  Both are gray under every flag.
    for after, gray in run_case({"AGA": L, "AGC": R}):
        assert after == {"AGA": NONE, "AGC": NONE} and gray == 2


def test_pair_that_differs_only_in_the_first_base():
    # ACA = 000100, CCA = 010100: they differ by 1 << 4.  The reference's masks stop at bit 3, so it never looks CCA up;
    # b << 2j reaches 16.  Normalising alone does not help: no ACA ^ m with m in {1,2,3,4,6,8,12} (ACC ACG ACT AAA
    # AAG AGA ATA) has CCA or its reverse complement TGG as a strand, nor does any CCA ^ m reach ACA / TGT.
    res = run_case({"ACA": L, "CCA": R})
    assert [g for _, g in res] == [0, 0, 2, 2]
    for (after, _), (wb, _nz) in zip(res, FLAGS):
        assert after == ({"ACA": NONE, "CCA": NONE} if wb else {"ACA": L, "CCA": R})


def test_pair_joined_only_through_a_reverse_complement():
    # ACA = 000100, TTT = 111111.  ACA ^ 4 == AAA (mask 4 = 1 << 2 is in both families), AAA is not stored: its canonical
    # form is TTT.  From the other end TTT ^ 4 == TGT = 111011, whose canonical form is ACA.  No mask joins 000100 and
    # 111111 directly (they differ in five bits).  Gray only when the neighbour is normalised before the lookup.
    assert o.normalize(o.kmer_value("AAA"), K) == o.kmer_value("TTT") and o.normalize(o.kmer_value("TGT"), K) == o.kmer_value("ACA")
    res = run_case({"ACA": L, "TTT": R})
    assert [g for _, g in res] == [0, 2, 0, 2]
    for (after, _), (_wb, nz) in zip(res, FLAGS):
        assert after == ({"ACA": NONE, "TTT": NONE} if nz else {"ACA": L, "TTT": R})


def test_pair_joined_only_by_a_mask_that_straddles_two_bases():
    # AGA = 001000, ATG = 001110: they differ by 6 = 3 << 1, which only the reference's shift by bits produces (it changes
    # base 1 and base 2 at once).  Gray by default, not with whole bases.
    res = run_case({"AGA": L, "ATG": R})
    assert [g for _, g in res] == [2, 2, 0, 0]


def test_neighbour_on_the_same_side_is_not_gray():
    for after, gray in run_case({"AGA": L, "AGC": L}):
        assert after == {"AGA": L, "AGC": L} and gray == 0
    for after, gray in run_case({"AGA": R, "AGC": R}):
        assert after == {"AGA": R, "AGC": R} and gray == 0


def test_neighbour_with_both_bits_or_neither_is_not_gray():
    # AGA (left only) has AGC = AGA ^ 1 (in both sets) and AGT = AGA ^ 3 (in neither: lhs == rhs) as neighbours; neither
    # belongs to the other side ONLY, and neither is a candidate itself.  Nothing changes.
    members = {"AGA": L, "AGC": BOTH, "AGT": NONE}
    for after, gray in run_case(members):
        assert after == members and gray == 0


def test_chain_reads_old_bits_only():
    # AGA (left) - AGC (right) - AGT (left), ranks 0 1 2: AGC = AGA ^ 1, AGT = AGC ^ 2.  All three are gray.  A loop that
    # cleared bits in place would find AGA and AGC gray and then see AGC with lhs == rhs when it came to AGT.
    for after, gray in run_case({"AGA": L, "AGC": R, "AGT": L}):
        assert after == {"AGA": NONE, "AGC": NONE, "AGT": NONE} and gray == 3


@pytest.mark.parametrize("k", [1, 2, 3, 5, 13, 32])
def test_distinct_masks_give_what_the_3k_masks_give(k):
    rng = random.Random(1000 + k)
    universe = 4 ** k
    n = min(universe, 400)
    if universe <= 4096:
        canon = sorted({o.normalize(v, k) for v in range(universe)})
        keys = canon if k < 3 else sorted(rng.sample(canon, len(canon) * 2 // 3))
    else:
        base = [rng.randrange(universe) for _ in range(n // 8)]
        near = [v ^ rng.choice(nm.reference_masks(k) + nm.reference_masks(k, True)) for v in base for _ in range(7)]
        keys = sorted({o.normalize(v, k) for v in base + near})
    lhs = [rng.randrange(2) for _ in keys]
    rhs = [rng.randrange(2) for _ in keys]
    grays = []
    for nz in (False, True):
        a = nm.near_kmers(keys, lhs, rhs, k, normalize=nz)
        b = nm.near_kmers(keys, lhs, rhs, k, normalize=nz, masks=nm.distinct_masks(k))
        assert a == b
        grays.append(a[2])
    assert k < 3 or max(grays) > 0             # (dense enough for the comparison to mean something; K < 3: 2 or 10 k-mers)


def test_bit_helpers_match_the_annotation_files():
    rng = random.Random(7)
    k = 5
    canon = sorted({o.normalize(v, k) for v in range(4 ** k)})
    a = sorted(rng.sample(canon, 150))
    b = sorted(rng.sample(canon, 150))
    files = dict(o.write_kmer_set(a, k, out="a"))
    files.update(o.write_kmer_set(b, k, out="b"))
    out, (na, nb, common) = o.merge_and_annotate(files, "a", "b", "u")
    union = sorted(set(a) | set(b))
    assert (na, nb, common) == (150, 150, len(set(a) & set(b))) and len(union) > 192          # (more than three words)
    sa, sb = set(a), set(b)
    lhs = [int(x in sa) for x in union]
    rhs = [int(x in sb) for x in union]
    assert nm.words_to_bytes(nm.pack_bits(lhs)) == out["u.lhs-bits"]
    assert nm.words_to_bytes(nm.pack_bits(rhs)) == out["u.rhs-bits"]
    assert nm.unpack_bits(nm.bytes_to_words(out["u.lhs-bits"]), len(union)) == lhs
    assert nm.pack_bits([]) == [0] and nm.pack_bits([1] * 64) == [2 ** 64 - 1] and nm.pack_bits([1] * 65) == [2 ** 64 - 1, 1]


def test_near_symbols_are_declared_and_exported():
    """include/goss_gpu_near.h, included by goss_gpu.h: what it declares is what the binding lists and the library exports"""
    import re
    import gossamer_amd as g
    text = open(os.path.join(ROOT, "include", "goss_gpu_near.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(goss_gpu_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(g.NEAR_SYMBOLS) == ["goss_gpu_object_near_kmers", "goss_gpu_object_near_kmers_host"]
    assert '#include "goss_gpu_near.h"' in open(os.path.join(ROOT, "include", "goss_gpu.h")).read()
    assert "GOSS_NEAR_WHOLE_BASES = 1" in text and "GOSS_NEAR_NORMALIZE = 2" in text
    assert (g.NEAR_WHOLE_BASES, g.NEAR_NORMALIZE) == (1, 2)
    L = g.load()
    for n in names:
        assert hasattr(L, n), n
    # refusals that come before any device is touched
    import ctypes as C
    gray = C.c_uint64(5)
    L.goss_gpu_object_near_kmers.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 2 + [C.POINTER(C.c_uint64)]
    L.goss_gpu_object_near_kmers_host.argtypes = L.goss_gpu_object_near_kmers.argtypes
    assert L.goss_gpu_object_near_kmers(None, None, None, 0, None, None, C.byref(gray)) == -1
    assert L.goss_gpu_object_near_kmers_host(None, None, None, 0, None, None, C.byref(gray)) == -1


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def test_cli_usage_errors(tmp_path):
    """GossCmdFactoryComputeNearKmers::create (GossCmdComputeNearKmers.cc:230-243): getRepeatingOnce("graph-in")"""
    tail = "use\n\tgoss compute-near-kmers -h\nfor more usage information.\n"
    rc, _, err = run_goss("compute-near-kmers")
    assert rc == 1 and err == "mandatory option graph-in was not given.\n" + tail
    rc, _, err = run_goss("compute-near-kmers", "-G", "a", "-G", "b")
    assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + tail
    rc, _, err = run_goss("compute-near-kmers", "-G", "a", "--bogus")
    assert rc == 1 and err == "unknown option '--bogus'\n" + tail
    rc, _, err = run_goss("compute-near-kmers", "-h")
    assert rc == 1 and "compute-near-kmers  Decorate a graph with an assignment of kmers to graphs." in err
    # -T is accepted; a set that is not there is an error that names the file, not a usage error
    missing = str(tmp_path / "nothing")
    rc, _, err = run_goss("compute-near-kmers", "-G", missing, "-T", "3")
    assert rc == 1 and err.startswith("error performing compute-near-kmers:\n") and "'%s.header'" % missing in err
    assert "for more usage information" not in err


def test_cli_names_a_missing_or_mis_sized_bitmap(tmp_path):
    """the files are checked before the device is asked for"""
    keys = sorted({o.normalize(v, 5) for v in range(0, 1024, 3)})
    base = str(tmp_path / "u")
    for name, data in o.write_kmer_set(keys, 5, out=base).items():
        open(name, "wb").write(data)
    rc, _, err = run_goss("compute-near-kmers", "-G", base)
    assert rc == 1 and "'%s.lhs-bits'" % base in err and "No such file" in err
    nwords = (len(keys) - 1) // 64 + 1
    open(base + ".lhs-bits", "wb").write(bytes(8 * nwords))
    rc, _, err = run_goss("compute-near-kmers", "-G", base)
    assert rc == 1 and "'%s.rhs-bits'" % base in err and "No such file" in err
    open(base + ".rhs-bits", "wb").write(bytes(8 * nwords + 8))
    rc, _, err = run_goss("compute-near-kmers", "-G", base)
    assert rc == 1 and "file '%s.rhs-bits' holds %d bytes" % (base, 8 * nwords + 8) in err
    assert open(base + ".lhs-bits", "rb").read() == bytes(8 * nwords)
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(n) for n in
                                                       list(o.write_kmer_set(keys, 5, out=base)) + [base + ".lhs-bits", base + ".rhs-bits"])
