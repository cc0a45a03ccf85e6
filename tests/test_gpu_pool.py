"""pool-samples on the device.  Through the binding, for every case of pool_cases.py: the samples' sizes and the common
k-mers of every pair are the model's integers (no tolerance), the index files are the oracle's bytes, whether the masks
come in calls of up to 32 samples or in the odd partition with set bits above nbits; the rows' padding shows as the sizes
and counts of the all-ones sample at z % 64 != 0.  Then the refusals, and `goss pool-samples` itself on files the oracle
wrote: <out>-union.*, <out>-index.*, <out>-a0.*, <out>-q0.* are the oracle's bytes and <out>.sim is the model's text."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import gossamer_amd as g
import pool_cases as pc
import pool_model as pm

pytestmark = pytest.mark.gpu

BUDGET = 256 << 20
ERR_INVALID_ARG, ERR_OOM, ERR_STATE = -1, -3, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


@pytest.fixture(scope="module")
def ctx():
    with g.Context(25, g.MODE_KMER_SET, hbm_budget=BUDGET) as c:
        yield c


@functools.lru_cache(maxsize=None)
def expected(name):
    """(sizes, inter, positions) of a case, planned: computed once, shared, never changed"""
    c = pc.case(name)
    return (tuple(pm.planned_sizes(c.masks, c.nsets)), tuple(map(tuple, pm.planned_intersections(c.masks, c.nsets))),
            tuple(pm.planned_positions(c.masks, c.nsets)))


def device_masks(values):
    a = np.array(values, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def add(ctx, c, slabs, junk=0):
    for first, nbits in slabs:
        t = device_masks(pm.slab_masks(c.masks, first, nbits, junk if nbits < 32 else 0))
        ctx.pool_add_masks(first, nbits, t.data_ptr(), c.z)


def first_difference(got, exp):
    if sorted(got) != sorted(exp):
        return "file sets differ: %s vs %s" % (sorted(got), sorted(exp))
    for n in sorted(exp):
        if got[n] != exp[n]:
            at = next((i for i, (a, b) in enumerate(zip(got[n], exp[n])) if a != b), min(len(got[n]), len(exp[n])))
            return "%s differs at byte %d (%d vs %d bytes)" % (n, at, len(got[n]), len(exp[n]))
    return None


def strip(files, base):
    return {n[len(base):]: b for n, b in files.items()}


# ---- through the binding ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.names())
def test_sizes_pairs_and_index_are_the_models(oracle, ctx, name):
    c = pc.case(name)
    sizes, inter, pos = expected(name)
    index = strip(oracle.write_sparse_array(list(pos), c.z * c.nsets, len(pos), base="x", N_end=c.z * c.nsets), "x")
    for how, slabs, junk in (("whole", pc.slabs_whole(c.nsets), 0), ("odd", pc.slabs_odd(c.nsets), 0x5A5A5A5A)):
        ctx.pool_begin(c.nsets, c.z)
        try:
            add(ctx, c, slabs, junk)
            got_sizes, got_inter = ctx.pool_sizes(), ctx.pool_intersections()
            assert tuple(got_sizes) == sizes, (name, how, next(i for i in range(c.nsets) if got_sizes[i] != sizes[i]))
            bad = next(((i, j, got_inter[i][j], inter[i][j]) for i in range(c.nsets) for j in range(c.nsets) if got_inter[i][j] != inter[i][j]), None)
            assert bad is None, (name, how, bad)
            assert [got_inter[i][i] for i in range(c.nsets)] == list(sizes)
            diff = first_difference(ctx.pool_emit_index(), index)
            assert diff is None, (name, how, diff)
            assert ctx.pool_intersections() == got_inter, (name, how, "the rows outlive the index")
        finally:
            ctx.pool_release()


def test_the_padding_of_the_last_word_is_zero(ctx):
    """all masks 0xFFFFFFFF at z % 64 != 0: every sample's size and every pair's count is z, not a multiple of 64"""
    for z in (1, 65, pc.MAX_Z):
        ctx.pool_begin(32, z)
        try:
            ctx.pool_add_masks(0, 32, device_masks([0xFFFFFFFF] * z).data_ptr(), z)
            assert ctx.pool_sizes() == [z] * 32
            assert ctx.pool_intersections() == [[z] * 32] * 32
        finally:
            ctx.pool_release()


def test_the_text_of_the_formatting_cases(ctx):
    for name, text in (("third", "0\t1\t0.333333\n"), ("tiny", "0\t1\t1e-05\n")):
        c = pc.case(name)
        ctx.pool_begin(c.nsets, c.z)
        try:
            add(ctx, c, pc.slabs_whole(c.nsets))
            assert g.pool_similarity_text(ctx.pool_intersections(), ctx.pool_sizes()) == text
        finally:
            ctx.pool_release()


def test_a_sample_that_was_never_added_is_empty(ctx):
    c = pc.case("s33_z65")
    sizes, inter, _ = expected(c.name)
    ctx.pool_begin(c.nsets, c.z)
    try:
        add(ctx, c, [(0, 32)])
        assert ctx.pool_sizes() == list(sizes[:32]) + [0]
        got = ctx.pool_intersections()
        assert [row[:32] for row in got[:32]] == [list(row[:32]) for row in inter[:32]] and got[32] == [0] * 33
    finally:
        ctx.pool_release()


# ---- refusals -------------------------------------------------------------------------------------------------------------

def refused(status, call, *args):
    with pytest.raises(g.GossGpuError) as e:
        call(*args)
    assert e.value.status == status, e.value
    return e.value


def test_rows_that_do_not_fit_the_budget_are_refused_and_nothing_is_held():
    with g.Context(25, g.MODE_KMER_SET, hbm_budget=16 << 20) as small:
        refused(ERR_OOM, small.pool_begin, 64, 1 << 24)          # 64 rows of 2 MiB
        t = device_masks([1])
        refused(ERR_STATE, small.pool_add_masks, 0, 1, t.data_ptr(), 1)
        small.pool_begin(64, 1 << 12)                           # ... and rows that fit are taken
        assert small.pool_sizes() == [0] * 64


def test_calls_out_of_order_and_bad_arguments_are_refused(ctx):
    c = pc.case("s33_z65")
    sizes, inter, _ = expected(c.name)
    t = device_masks(pm.slab_masks(c.masks, 0, 32))
    ctx.pool_release()
    refused(ERR_STATE, ctx.pool_add_masks, 0, 32, t.data_ptr(), c.z)          # before begin
    refused(ERR_STATE, ctx.pool_sizes)
    refused(ERR_STATE, ctx.pool_intersections)
    refused(ERR_STATE, ctx.pool_emit_index)
    refused(ERR_INVALID_ARG, ctx.pool_begin, 0, 10)
    refused(ERR_INVALID_ARG, ctx.pool_begin, 3, 0)
    refused(ERR_INVALID_ARG, ctx.pool_begin, 3, 1 << 63)                      # z * nsets >= 2^64
    ctx.pool_begin(c.nsets, c.z)
    try:
        refused(ERR_INVALID_ARG, ctx.pool_add_masks, 0, 32, t.data_ptr(), c.z + 1)      # a z that differs from begin's
        refused(ERR_INVALID_ARG, ctx.pool_add_masks, 0, 33, t.data_ptr(), c.z)
        refused(ERR_INVALID_ARG, ctx.pool_add_masks, 0, 0, t.data_ptr(), c.z)
        refused(ERR_INVALID_ARG, ctx.pool_add_masks, 2, 32, t.data_ptr(), c.z)          # sets past the end
        ctx.pool_add_masks(0, 32, t.data_ptr(), c.z)
        refused(ERR_STATE, ctx.pool_add_masks, 0, 32, t.data_ptr(), c.z)                # a range added twice
        refused(ERR_STATE, ctx.pool_add_masks, 31, 2, t.data_ptr(), c.z)                # ... or in part
        add(ctx, c, [(32, 1)])
        assert tuple(ctx.pool_sizes()) == sizes                  # the refused calls changed nothing
        assert tuple(map(tuple, ctx.pool_intersections())) == inter
    finally:
        ctx.pool_release()


def test_begin_is_refused_while_a_count_is_in_progress():
    with g.Context(25, g.MODE_KMER_SET, hbm_budget=BUDGET) as busy:
        busy.push_host(g.synth_reads_host(50, 100, 2000, seed=3))
        refused(ERR_STATE, busy.pool_begin, 2, 100)
        busy.finish()
        busy.pool_begin(2, 100)                                 # after finish the context may hold a pool
        assert busy.pool_sizes() == [0, 0]


def test_the_masks_may_be_another_contexts_merged_counts(oracle, ctx):
    """what the command does: the samples merged as runs of weights 1 << i in a second context, whose d_counts are the masks;
    that context is reset at once"""
    c = pc.cmd_case("cmd_s9")
    samples = pc.cmd_samples(c)
    with g.Context(c.K, g.MODE_KMER_SET, hbm_budget=BUDGET) as merger:
        for i, s in enumerate(samples):
            if s:
                keys = np.array(s, dtype=np.uint64)
                counts = np.full(len(s), 1 << i, dtype=np.uint32)
                merger.push_run_host(keys.ctypes.data, counts.ctypes.data, len(s))
        merger.finish()
        _, d_counts, z = merger.result_ptrs()
        assert z == len(c.keys)
        ctx.pool_begin(c.nsets, z)
        try:
            ctx.pool_add_masks(0, c.nsets, d_counts, z)
            merger.reset()
            assert ctx.pool_sizes() == pm.sizes(samples)
            assert ctx.pool_intersections() == pm.intersections(samples)
            N, M, N_end = pm.index_shape(samples)
            exp = strip(oracle.write_sparse_array(pm.positions(samples), N, M, base="x", N_end=N_end), "x")
            assert first_difference(ctx.pool_emit_index(), exp) is None
        finally:
            ctx.pool_release()


# ---- through the command --------------------------------------------------------------------------------------------------

def run(args):
    return subprocess.run([GOSS] + args + ["--hbm-budget", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def write(tmp_path, files):
    for n, b in files.items():
        (tmp_path / n).write_bytes(b)


def disk(tmp_path, base):
    return {n[len(base):]: (tmp_path / n).read_bytes() for n in os.listdir(tmp_path) if n.startswith(base + ".") or n.startswith(base + "-")}


def pooled(oracle, files, names, samples):
    """what pool-samples leaves under "out" for the samples `names` (objects in `files`): the oracle's union and index, the
    model's text"""
    exp = strip(oracle.merge(files, names, 0, "out-union", max_merge=8), "out")
    N, M, N_end = pm.index_shape(samples)
    exp.update(strip(oracle.write_sparse_array(pm.positions(samples), N, M, base="out-index", N_end=N_end), "out"))
    exp[".sim"] = pm.sim_text(pm.intersections(samples), pm.sizes(samples)).encode()
    return exp


@pytest.mark.parametrize("name", pc.cmd_names())
def test_the_command_writes_the_oracles_union_and_index_and_the_models_text(oracle, tmp_path, name):
    c = pc.cmd_case(name)
    samples = pc.cmd_samples(c)
    files, names = {}, []
    for i, s in enumerate(samples):
        if c.twice and i == c.twice[1]:
            names.append("s%d" % c.twice[0])                    # the same object named again
            continue
        files.update(oracle.write_kmer_set(s, c.K, out="s%d" % i))
        names.append("s%d" % i)
    write(tmp_path, files)
    args = ["pool-samples", "-O", str(tmp_path / "out")]
    if c.nsets > 32:
        (tmp_path / "list.txt").write_text("".join("%s\n" % (tmp_path / n) for n in names[1:]))
        args += ["--kmer-set-in", str(tmp_path / names[0]), "--kmer-sets-in", str(tmp_path / "list.txt")]
    else:
        for n in names:
            args += ["--kmer-set-in", str(tmp_path / n)]
    p = run(args)
    assert p.returncode == 0, p.stderr.decode()
    diff = first_difference(disk(tmp_path, "out"), pooled(oracle, files, names, samples))
    assert diff is None, (name, diff)


def test_the_command_on_a_kmer_set_a_fasta_and_a_fastq_file(oracle, tmp_path):
    K = 25
    reads = g.synth_reads_host(40, 80, 1500, seed=11).decode().split("\n")[:-1]
    fa = "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads[:25]))
    fq = "".join("@q%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads[15:]))
    (tmp_path / "c.fa").write_text(fa)
    (tmp_path / "d.fq").write_text(fq)
    ka = oracle.count([(oracle.FASTA, "c.fa", fa)], K, 0)[0]
    kq = oracle.count([(oracle.FASTQ, "d.fq", fq)], K, 0)[0]
    ks = sorted(set(ka[::3]) | set(kq[1::4]) | {5, 1 << 49})
    files = oracle.write_kmer_set(ks, K, out="a")
    write(tmp_path, files)
    built = {}
    built.update(oracle.build_kmer_set([(oracle.FASTA, "c.fa", fa)], K, out="out-a0")[0])
    built.update(oracle.build_kmer_set([(oracle.FASTQ, "d.fq", fq)], K, out="out-q0")[0])
    files.update(built)
    p = run(["pool-samples", "-O", str(tmp_path / "out"), "--kmer-set-in", str(tmp_path / "a"), "-I", str(tmp_path / "c.fa"), "-i", str(tmp_path / "d.fq")])
    assert p.returncode == 0, p.stderr.decode()
    exp = pooled(oracle, files, ["a", "out-a0", "out-q0"], [ks, ka, kq])
    exp.update(strip(built, "out"))
    diff = first_difference(disk(tmp_path, "out"), exp)
    assert diff is None, diff
    assert len(set(ka) & set(kq)) > 0 and set(ks) - set(ka) - set(kq)


def test_the_command_refuses_samples_of_different_k(oracle, tmp_path):
    write(tmp_path, oracle.write_kmer_set([1, 2, 3], 25, out="a"))
    write(tmp_path, oracle.write_kmer_set([2, 3, 4], 27, out="b"))
    p = run(["pool-samples", "-O", str(tmp_path / "out"), "--kmer-set-in", str(tmp_path / "a"), "--kmer-set-in", str(tmp_path / "b")])
    assert p.returncode == 1 and "all samples must have the same kmer-size." in p.stderr.decode(), p.stderr.decode()
    assert disk(tmp_path, "out") == {}
