"""pool-samples without a GPU: the model (pool_model.py) against cases worked out by hand, the corpus (pool_cases.py)
against its own stated conditions, the model's union and index composed from the oracle as it stands and read back, and
the usage errors of `goss pool-samples`, which need no device."""
import os
import re
import subprocess

import pytest

import gossamer_amd as g
import pool_cases as pc
import pool_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


# ---- the model, by hand ---------------------------------------------------------------------------------------------------

def test_the_model_on_three_samples_worked_out_by_hand():
    # union 10 20 30 40 50 (ranks 0..4); A = {10, 20, 40}, B = {20, 30, 40, 50}, C = {}
    a, b, c = [40, 10, 20], [20, 30, 40, 50], []
    assert pm.union_order([a, b, c]) == [10, 20, 30, 40, 50]
    assert pm.sizes([a, b, c]) == [3, 4, 0]
    assert pm.intersections([a, b, c]) == [[3, 2, 0], [2, 4, 0], [0, 0, 0]]
    # z = 5: A at 0 * 5 + {0, 1, 3}, B at 1 * 5 + {1, 2, 3, 4}
    assert pm.positions([a, b, c]) == [0, 1, 3, 6, 7, 8, 9]
    assert pm.index_shape([a, b, c]) == (15, 7, 15)
    # |A u B| = 5: 2 / 5; against the empty sample 0 / 3 and 0 / 4
    assert pm.sim_text(pm.intersections([a, b, c]), pm.sizes([a, b, c])) == "0\t1\t0.4\n0\t2\t0\n1\t2\t0\n"


def test_the_text_has_a_streams_six_significant_digits():
    assert pm.sim_text([[2, 1], [1, 2]], [2, 2]) == "0\t1\t0.333333\n"
    assert pm.sim_text([[7, 7], [7, 7]], [7, 7]) == "0\t1\t1\n"
    assert pm.sim_text([[50000, 1], [1, 50001]], [50000, 50001]) == "0\t1\t1e-05\n"
    assert pm.sim_text([[4096, 1], [1, 4098]], [4096, 4098]) == "0\t1\t0.000122055\n"
    assert g.pool_similarity_text([[2, 1], [1, 2]], [2, 2]) == "0\t1\t0.333333\n"
    assert pm.sim_text([[1]], [1]) == ""


def test_a_planned_case_by_hand():
    # k-mers 0..3 with masks 0b01, 0b11, 0b10, 0b00 (the last one in no sample: it still takes a rank)
    masks = [1, 3, 2, 0]
    assert pm.planned_rows(masks, 2) == [0b0011, 0b0110]
    assert pm.planned_sizes(masks, 2) == [2, 2]
    assert pm.planned_intersections(masks, 2) == [[2, 1], [1, 2]]
    assert pm.planned_positions(masks, 2) == [0, 1, 4 + 1, 4 + 2]
    assert pm.planned_samples([5, 6, 7, 8], masks, 2) == [[5, 6], [6, 7]]
    assert pm.slab_masks([0b101, 0b110], 1, 2) == [0b10, 0b11]
    assert pm.slab_masks([0b101, 0b110], 1, 1, junk=1) == [0b10, 0b11]
    assert pm.slab_masks([1, 0], 0, 31, junk=1) == [0x80000001, 0x80000000]


@pytest.mark.parametrize("name", ["s2_z65", "s33_z65", "s65_z65", "third"])
def test_planned_and_set_forms_of_the_model_agree(name):
    c = pc.case(name)
    keys = [3 * r + 1 for r in range(c.z)]
    samples = pm.planned_samples(keys, c.masks, c.nsets)
    assert pm.sizes(samples) == pm.planned_sizes(c.masks, c.nsets)
    assert pm.intersections(samples) == pm.planned_intersections(c.masks, c.nsets)
    if all(c.masks):                                             # (every key in the union: the ranks are the keys' indices)
        assert pm.positions(samples) == pm.planned_positions(c.masks, c.nsets)


# ---- the corpus against its own conditions ----------------------------------------------------------------------------------

def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gossamer_amd", "csrc", "kernels_pool.hpp")).read()
    for name, value in (("kPoolTile", g.POOL_TILE), ("kPoolPairWords", g.POOL_PAIR_WORDS), ("kPoolPosWords", g.POOL_POS_WORDS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == value, name


def test_the_corpus_holds_every_size_it_states():
    zs = {c.z for c in pc.CASES}
    ss = {c.nsets for c in pc.CASES}
    assert {1, 63, 64, 65, 4095, 4096, 4097} <= zs
    for words in (g.POOL_PAIR_WORDS, g.POOL_POS_WORDS):
        assert {words * 64, words * 64 + 1} <= zs
    assert {1, 2, 31, 32, 33, 63, 64, 65, g.POOL_TILE - 1, g.POOL_TILE + 1} <= ss
    for z in pc.ZS:                                             # every z with more than one tile's worth of pairs or a full call
        assert any(c.z == z and c.nsets >= 31 for c in pc.CASES), z
    assert all(c.nsets <= pc.MAX_SETS and (c.z <= pc.MAX_Z or c.name == "tiny") for c in pc.CASES)
    assert len(set(pc.names())) == len(pc.CASES)


def test_the_corpus_holds_every_mask_kind_it_states():
    c = pc.case("s65_z%d" % pc.MAX_Z)
    assert c.tags == frozenset(pc.KINDS) | {"random"}
    z, full = c.z, (1 << c.z) - 1
    rows = pm.planned_rows(c.masks, c.nsets)
    size, inter = pm.planned_sizes(c.masks, c.nsets), pm.planned_intersections(c.masks, c.nsets)
    k = {name: i for i, name in enumerate(pc.KINDS)}
    assert rows[k["ones"]] == full and rows[k["zeros"]] == 0 and rows[k["first"]] == 1 and rows[k["last"]] == 1 << (z - 1)
    assert z % 64 != 0                                           # the all-ones row ends inside a word: padding to keep zero
    assert rows[k["copy"]] == rows[k["random"]] and inter[k["copy"]][k["random"]] == size[k["copy"]] > 0          # sim exactly 1
    assert inter[k["complement"]][k["random"]] == 0 and size[k["complement"]] + size[k["random"]] == z           # sim 0
    assert rows[k["nested"]] & ~rows[k["random"]] == 0 and 0 < size[k["nested"]] < size[k["random"]]
    assert len({rows[i] for i in range(len(pc.KINDS), c.nsets)}) == c.nsets - len(pc.KINDS)                      # the random rows differ
    for cc in pc.CASES:                                          # kinds by sample index, in every case that has the samples
        assert cc.tags == pc.kinds_of(cc.nsets) or cc.name in ("third", "tiny")
    t = pc.case("third")
    assert pm.sim_text(pm.planned_intersections(t.masks, 2), pm.planned_sizes(t.masks, 2)) == "0\t1\t0.333333\n"
    t = pc.case("tiny")
    assert pm.sim_text(pm.planned_intersections(t.masks, 2), pm.planned_sizes(t.masks, 2)) == "0\t1\t1e-05\n"


def test_the_slabs_are_partitions_with_the_stated_calls():
    for n in pc.SS:
        for slabs in (pc.slabs_whole(n), pc.slabs_odd(n)):
            assert sorted(i for f, b in slabs for i in range(f, f + b)) == list(range(n))
            assert all(1 <= b <= 32 for f, b in slabs)
    odd = pc.slabs_odd(65)
    assert {b for f, b in odd} == {1, 31, 32} and any(f % 32 for f, b in odd if b in (31, 32)) and odd[0][0] > odd[-1][0]


def test_the_commands_cases_are_what_they_state():
    by = {c.name: c for c in pc.CMD_CASES}
    assert [by[n].K for n in ("cmd_s3_k31", "cmd_s3_k32", "cmd_s3_k33")] == [31, 32, 33]
    assert [by[n].nsets for n in ("cmd_s3_k31", "cmd_s9", "cmd_s33", "cmd_s65")] == [3, 9, 33, 65]
    for c in pc.CMD_CASES:
        samples = pc.cmd_samples(c)
        assert pm.union_order(samples) == c.keys and c.keys == sorted(set(c.keys)) and c.keys[-1] < 1 << (2 * c.K)
        if c.nsets >= 9:
            assert [] in samples and samples[4] == samples[5]
        if c.twice:
            assert samples[c.twice[0]] == samples[c.twice[1]]


# ---- the union and the index composed from the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cmd_s3_k33", "cmd_s9"])
def test_the_models_union_and_index_read_back_from_the_oracles_files(oracle, name):
    c = pc.cmd_case(name)
    samples = pc.cmd_samples(c)
    files, names = {}, []
    for i, s in enumerate(samples):
        files.update(oracle.write_kmer_set(s, c.K, out="s%d" % i))
        names.append("s%d" % i)
    union = oracle.merge(files, names, 0, "out-union", max_merge=8)
    assert oracle.kmer_set_header(union, "out-union") == (c.K, len(pm.union_order(samples)))
    rd = oracle.SparseReader(union, "out-union.kmers")
    assert [rd.select(r) for r in range(rd.count())] == pm.union_order(samples)
    pos = pm.positions(samples)
    N, M, N_end = pm.index_shape(samples)
    index = oracle.write_sparse_array(pos, N, M, base="out-index", N_end=N_end)
    rd = oracle.SparseReader(index, "out-index")
    assert rd.count() == M == len(pos) and rd.size() == N
    assert [rd.select(r) for r in range(M)] == pos
    z = len(c.keys)
    for i, s in enumerate(samples):                              # row i of the array is sample i's membership in the union
        assert [r for r in range(z) if rd.access(i * z + r)] == [r for r, k in enumerate(c.keys) if k in set(s)]


# ---- the command's usage errors ------------------------------------------------------------------------------------------

def run(args):
    return subprocess.run([GOSS] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_pool_samples_needs_an_output_name(tmp_path):
    p = run(["pool-samples", "--kmer-set-in", str(tmp_path / "a")])
    assert p.returncode == 1
    assert "mandatory option graph-out was not given." in p.stderr.decode() and "goss pool-samples -h" in p.stderr.decode()
    assert os.listdir(tmp_path) == []


def test_pool_samples_without_samples_says_so_and_writes_nothing(tmp_path):
    p = run(["pool-samples", "-O", str(tmp_path / "out"), "-v"])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stderr.decode().rstrip("\n").endswith("\tinfo\tno samples")
    assert os.listdir(tmp_path) == []


def test_pool_samples_is_listed_and_refuses_an_unreadable_input(tmp_path):
    assert "pool-samples" in run(["help"]).stderr.decode()
    p = run(["pool-samples", "-O", str(tmp_path / "out"), "-I", str(tmp_path / "missing.fa")])
    assert p.returncode == 1 and "cannot open file" in p.stderr.decode()
