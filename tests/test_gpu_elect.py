"""Reads against up to 64 references on the device (goss_gpu_object_colour_reads, Object.colours / colours_from_index /
colour_reads, `goss elect-reads`) against the model (tests/elect_model.py) over the corpus of tests/elect_cases.py, which
test_elect_cpu.py holds to its claims.  Sets are written with the oracle and opened with Object.open."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import classify_cases as cc
import elect_cases as ec
import elect_model as em
import gossamer_amd as g
import match_model as mm
import near_model as nm
import oracle_lib as o
import pool_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
LIBRARY_CASES = [n for n in ec.NAMES if not n.startswith("pool") and n != "command"]


def open_set(keys, K):
    return g.Object.open(o.write_kmer_set(list(keys), K, out="ks"), "ks", g.OBJECT_KMER_SET)


def lists(t, dtype):
    import torch
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy().view(dtype)
    assert t.dtype == dtype
    return t.tolist()


def check_info(info, words, nwin, by_count):
    assert {k: info[k] for k in ("reads", "windows", "by_count")} == {"reads": len(words), "windows": sum(nwin), "by_count": by_count}
    assert sum(info["by_count"]) == info["reads"] and info["ms"] >= 0


@pytest.mark.parametrize("name", LIBRARY_CASES)
def test_corpus(name):
    import torch
    c = ec.fixture(name)
    K, keys, data = c["K"], c["keys"], c["data"]
    words, nwin, by_count = ec.expected(name)
    starts = mm.read_starts(data)
    with open_set(keys, K) as obj:
        assert obj.count == len(keys)
        obj.colours(c["colours"], c["ncolours"])
        # bytes in, numpy out
        gc, gw, gs, info = obj.colour_reads(data, starts=True)
        assert (lists(gc, np.uint64), lists(gw, np.uint32), lists(gs, np.uint64)) == (words, nwin, starts)
        check_info(info, words, nwin, by_count)
        # the same input gives the same arrays
        gc2, gw2, _ = obj.colour_reads(np.frombuffer(data, dtype=np.uint8))
        assert (gc2.tolist(), gw2.tolist()) == (words, nwin)
        # what match_reads says of the same bytes, no model in between: a word with a bit is a hit
        aw, ah, _ = obj.match_reads(data, normalize=True, any=True)
        assert aw.tolist() == gw.tolist()
        if 0 not in c["colours"]:
            assert [1 if x else 0 for x in gc.tolist()] == ah.tolist()
        else:
            assert all(h for x, h in zip(gc.tolist(), ah.tolist()) if x)
        # a device tensor that begins at 1 mod 8; tensors come back
        t1 = torch.from_numpy(np.frombuffer(b"\n" + data, dtype=np.uint8).copy()).cuda()[1:]
        assert t1.data_ptr() % 8 == 1
        gc, gw, gs, info = obj.colour_reads(t1, starts=True)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (gc, gw, gs))
        assert (lists(gc, np.uint64), lists(gw, np.uint32), lists(gs, np.uint64)) == (words, nwin, starts)
        check_info(info, words, nwin, by_count)
        # only the counts are wanted
        inf = g.binding.ElectInfo()
        assert obj._L.goss_gpu_object_colour_reads(obj._h, t1.data_ptr(), t1.numel(), g.ELECT_NORMALIZE, 0, None, None, None, C.byref(inf)) == 0
        check_info(inf.as_dict(), words, nwin, by_count)
        # the host form, which the command uses
        hc, hw = np.zeros(len(words), dtype=np.uint64), np.zeros(len(words), dtype=np.uint32)
        hs = np.zeros(len(words) + 1, dtype=np.uint64)
        assert obj._L.goss_gpu_object_colour_reads_host(obj._h, data, len(data), g.ELECT_NORMALIZE, len(words), hc.ctypes.data, hw.ctypes.data,
                                                        hs.ctypes.data, C.byref(inf)) == 0
        assert (hc.tolist(), hw.tolist(), hs.tolist()) == (words, nwin, starts)
        check_info(inf.as_dict(), words, nwin, by_count)


def key_reads(keys, K):
    """every key's K bases as a read: read r has one window, the key at rank r"""
    return ("\n".join(cc.key_text(x, K) for x in keys) + "\n").encode()


@pytest.mark.parametrize("S", ec.POOL_SIZES)
def test_colours_from_a_pool(S):
    keys, masks = ec.pool(S)
    samples = ec.pool_samples(S)
    N, M, N_end = pm.index_shape(samples)
    z = len(keys)
    assert N == S * z
    index_files = o.write_sparse_array(pm.positions(samples), N, M, base="p-index", N_end=N_end)
    c = ec.fixture("pool%d" % S)
    words, nwin, by_count = ec.expected("pool%d" % S)
    with open_set(keys, 5) as obj, g.Object.open(index_files, "p-index", g.OBJECT_SPARSE_ARRAY) as index:
        assert obj.colours_from_index(index) == S
        # the word of every rank is the model's membership
        gc, gw, _ = obj.colour_reads(key_reads(keys, 5))
        assert gc.tolist() == list(masks) and gw.tolist() == [1] * z
        gc, gw, info = obj.colour_reads(c["data"])
        assert (gc.tolist(), gw.tolist()) == (words, nwin)
        check_info(info, words, nwin, by_count)
        # the same bytes on every run
        assert obj.colours_from_index(index) == S
        assert obj.colour_reads(key_reads(keys, 5))[0].tolist() == list(masks)


def test_colours_from_index_refusals():
    S = 2
    keys, masks = ec.pool(S)
    samples = ec.pool_samples(S)
    z = len(keys)
    pos = pm.positions(samples)
    probe = key_reads(keys, 5)
    with open_set(keys, 5) as obj:
        kept = [1 << (r % 7) for r in range(z)]
        obj.colours(kept, 7)

        def refused(files, base, kind, *needles):
            with g.Object.open(files, base, kind) as other:
                with pytest.raises(g.GossGpuError) as e:
                    obj.colours_from_index(other)
            assert e.value.status == -1 and all(n in str(e.value) for n in needles), str(e.value)
            assert obj.colour_reads(probe)[0].tolist() == kept                   # the result kept
        # a universe that is not S * z
        refused(o.write_sparse_array(pos, S * z + 1, len(pos), base="x", N_end=S * z + 1), "x", g.OBJECT_SPARSE_ARRAY, "universe", "S * count")
        # S = 65
        refused(o.write_sparse_array(pos, 65 * z, len(pos), base="x", N_end=65 * z), "x", g.OBJECT_SPARSE_ARRAY, "S = 65", "1 .. 64")
        # an object of the wrong kind
        refused(o.write_kmer_set(list(keys), 5, out="k2"), "k2", g.OBJECT_KMER_SET, "SparseArray")
        assert obj._L.goss_gpu_object_colours_from_index(obj._h, None, None) == -1
        # and a graph cannot carry colours
    edges = sorted({v for x in cc.genomes(25)[2][:100] for v in (x, o.revcomp(x, 25))})
    with g.Object.open(o.write_graph(edges, [1] * len(edges), 24, out="gr"), "gr", g.OBJECT_GRAPH) as gr:
        for call in (lambda: gr.colours([0] * gr.count, 1), lambda: gr.colour_reads(b"ACGT\n")):
            with pytest.raises(g.GossGpuError) as e:
                call()
            assert e.value.status == -1 and "KmerSet" in str(e.value)


def test_edges_of_the_call():
    c = ec.fixture("ranks129")
    K, keys, data = c["K"], c["keys"], c["data"]
    words, nwin, by_count = ec.expected("ranks129")
    n = len(keys)
    with open_set(keys, K) as obj:
        # no colours set
        with pytest.raises(g.GossGpuError) as e:
            obj.colour_reads(data)
        assert e.value.status == -1 and "no colours kept" in str(e.value)
        # ncolours out of range; a word with a bit at or above ncolours names the rank, and nothing is kept
        for bad in (0, 65):
            with pytest.raises(g.GossGpuError) as e:
                obj.colours(c["colours"], bad)
            assert e.value.status == -1 and "1 .. 64" in str(e.value)
        with pytest.raises(g.GossGpuError) as e:
            obj.colours(c["colours"], 63)
        assert e.value.status == -1 and "rank 63 " in str(e.value) and "ncolours = 63" in str(e.value)
        with pytest.raises(g.GossGpuError):
            obj.colour_reads(data)
        with pytest.raises(ValueError):
            obj.colours(c["colours"][:-1], 64)
        obj.colours(c["colours"], 64)
        # nbytes = 0; reads without windows
        gc, gw, gs, info = obj.colour_reads(b"", starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == ([], [], [0]) and info["reads"] == 0 and info["by_count"] == [0] * 65
        gc, gw, gs, info = obj.colour_reads(b"\nACGT\n\n", starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == ([0, 0, 0], [0, 0, 0], [0, 1, 6, 6]) and info["by_count"] == [3] + [0] * 64
        # a last read without its newline
        gc, gw, gs, info = obj.colour_reads(data[:-1], starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == (words, nwin, mm.read_starts(data[:-1])) and gs.tolist()[-1] == len(data) - 1
        # max_reads one too small: the need comes back, and the object still answers, with room to spare too
        with pytest.raises(g.GossGpuError) as e:
            obj.colour_reads(data, max_reads=n - 1)
        assert e.value.status == g.binding.ERR_BUFFER and "max_reads = %d" % n in str(e.value)
        gc, gw, info = obj.colour_reads(data, max_reads=n + 5)
        assert (gc.tolist(), gw.tolist(), info["by_count"]) == (words, nwin, by_count)
        # an unknown flag
        for flags in (2, 4, 1 << 31):
            assert obj._L.goss_gpu_object_colour_reads(obj._h, None, 0, flags, 0, None, None, None, None) == -1
            assert b"flag" in obj._L.goss_gpu_object_last_error(obj._h)
        # a second call replaces the words
        obj.colours([1 << (63 - r % 64) for r in range(n)], 64)
        assert obj.colour_reads(data)[0].tolist() == [1 << (63 - r % 64) for r in range(n)]
        obj.colours([3] * n, 2)
        gc, _, info = obj.colour_reads(data)
        assert gc.tolist() == [3] * n and info["by_count"][2] == n
        # without normalize the windows are looked up as they stand
        rank_of = {x: i for i, x in enumerate(keys)}
        rc_data = ("\n".join(mm.rc_text(cc.key_text(x, K)) for x in keys) + "\n").encode()
        exp = [3 if mm.windows(rc_data[b:e], K)[0][1] in rank_of else 0 for b, e in mm.read_spans(rc_data)]
        assert 0 in exp and obj.colour_reads(rc_data)[0].tolist() == [3] * n
        assert obj.colour_reads(rc_data, normalize=False)[0].tolist() == exp
    # an empty set: nothing is in it, with no colours, and with colours of no words
    with open_set([], 25) as obj:
        assert obj.count == 0
        gc, gw, info = obj.colour_reads(data)
        assert gc.tolist() == [0] * n and gw.tolist() == nwin and info["by_count"] == [n] + [0] * 64
        obj.colours([], 1)
        assert obj.colour_reads(data)[0].tolist() == [0] * n


def test_two_colours_are_the_classes_of_classify_reads():
    """S = 2 with the colours made of a pair of bitmaps: bit 0 = lhs, bit 1 = rhs.  On reads whose windows share one class
    c = 2 * lhs + rhs, classify_reads' mask is 1 << c and the word is the two bits of c exchanged; no model in between."""
    for name in ("ranks129", "sixteen25"):
        c = cc.fixture(name)
        n = len(c["keys"])
        wl, wr = (np.array(nm.pack_bits(b)[:(n + 63) // 64], dtype=np.uint64) for b in (c["lhs"], c["rhs"]))
        with open_set(c["keys"], 25) as obj:
            obj.classify_bits(wl, wr)
            obj.colours([a | (b << 1) for a, b in zip(c["lhs"], c["rhs"])], 2)
            classes, cw, _ = obj.classify_reads(c["data"])
            words, ww, _ = obj.colour_reads(c["data"])
            assert cw.tolist() == ww.tolist()
            one_class = 0
            for m, w in zip(classes.tolist(), words.tolist()):
                # the word is the OR, over the classes in the mask, of the class's two bits
                assert w == (1 if m & 0b1100 else 0) | (2 if m & 0b1010 else 0)
                if m in (1, 2, 4, 8):
                    one_class += 1
                    cls = m.bit_length() - 1
                    assert w == (cls >> 1) | ((cls & 1) << 1)
            assert one_class >= 12


# ---- the command -------------------------------------------------------------------------------------------------------

def run_goss(args, cwd, env_extra=None):
    env = dict(os.environ)
    env.update({k: str(v) for k, v in (env_extra or {}).items()})
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env, cwd=str(cwd))
    return p.returncode, p.stdout, p.stderr.decode()


def outputs(folder, before):
    return {f: (folder / f).read_bytes() for f in os.listdir(str(folder)) if f not in before}


FLAG = {"line": "--line-in", "fasta": "-I", "fastq": "-i"}
AS = {"line": lambda r: b"\n".join(r) + b"\n", "fasta": mm.as_fasta, "fastq": mm.as_fastq}


def write_references(folder):
    """r0.fa, r1.fa and the k-mer set r2: the arguments that name them, in colour order"""
    texts, ref_sets, _, _ = ec.command_refs()
    for i in (0, 1):
        (folder / ("r%d.fa" % i)).write_bytes((">r%d\n%s\n" % (i, texts[i])).encode())
    for name, data in o.write_kmer_set(sorted(ref_sets[2]), 25, out="r2").items():
        (folder / name).write_bytes(data)
    return ["--ref-fasta", "r0.fa", "--ref-index", "r2", "--ref-fasta", "r1.fa"]


def single_items(folder):
    reads = [t.encode() for _, t in cc.sixteen_reads(25) if t]
    third = len(reads) // 3
    items = [("fastq", mm.as_fastq(reads[:third])), ("line", AS["line"](reads[third:2 * third])), ("fasta", mm.as_fasta(reads[2 * third:])),
             ("line", AS["line"](reads[5:25]))]
    args = []
    for i, (fmt, text) in enumerate(items):
        (folder / ("in%d" % i)).write_bytes(text)
        args += [FLAG[fmt], "in%d" % i]
    return items, args


def pair_items(folder):
    a, b = ec.command_pairs()
    items = [("fastq", mm.as_fastq(a)), ("fastq", mm.as_fastq(b)), ("line", AS["line"](b[:20])), ("line", AS["line"](a[:20])),
             ("fasta", mm.as_fasta(a[20:])), ("fasta", mm.as_fasta(b[20:]))]
    args = []
    for i, (fmt, text) in enumerate(items):
        (folder / ("pin%d" % i)).write_bytes(text)
        args += [FLAG[fmt], "pin%d" % i]
    return items, args + ["--pairs"]


@pytest.mark.parametrize("threshold", [None, 0, 1, 2])
def test_command_on_single_reads(tmp_path, threshold):
    refs = write_references(tmp_path)
    items, ins = single_items(tmp_path)
    _, _, keys, colours = ec.command_refs()
    before = set(os.listdir(str(tmp_path)))
    extra = [] if threshold is None else ["--ref-threshold", threshold]
    # which prefixes are given varies with the threshold: both, both, the match prefix only, the other only
    match, non_match = {None: ("m", "out.n"), 0: ("m", "n"), 1: ("m", ""), 2: ("", "n")}[threshold]
    for p, v in (("--match-prefix", match), ("--non-match-prefix", non_match)):
        extra += [p, v] if v else []
    want, matched, unmatched = em.elect_reads(items, 25, keys, colours, t=threshold, nrefs=3, match_prefix=match, non_match_prefix=non_match)
    assert len(want) == 3 * (bool(match) + bool(non_match)) and matched and unmatched
    env = {"GOSS_MATCH_BATCH": 1500} if threshold in (None, 1) else None
    rc, out, err = run_goss(["elect-reads", "-K", 25] + refs + ins + extra + ["-M", "1.5", "-T", "2", "--preserve-read-order", "-v"], tmp_path, env)
    assert rc == 0, err
    assert out == b""
    assert outputs(tmp_path, before) == want                                     # (and no temporary object is left)
    msgs = [line.split("\t", 2)[2] for line in err.splitlines() if line.count("\t") >= 2]
    assert "matched %d reads, unmatched %d" % (matched, unmatched) in msgs
    words = [w for fmt in em.KINDS for f, t in items if f == fmt for w in em.colour_reads(AS["line"](mm.PARSERS[f](t)), 25, keys, colours)[0]]
    hist = ", ".join("%d: %d" % (j, sum(1 for w in words if em.popcount(w) == j)) for j in range(4) if any(em.popcount(w) == j for w in words))
    assert "reads by the number of references hit: " + hist in msgs


@pytest.mark.parametrize("threshold", [None, 0, 1, 2])
def test_command_on_pairs(tmp_path, threshold):
    refs = write_references(tmp_path)
    items, ins = pair_items(tmp_path)
    _, _, keys, colours = ec.command_refs()
    tmp = tmp_path / "scratch"
    tmp.mkdir()
    before = set(os.listdir(str(tmp_path)))
    extra = [] if threshold is None else ["--ref-threshold", threshold]
    match, non_match = {None: ("m", "n"), 0: ("", "n"), 1: ("m", ""), 2: ("m.x", "n")}[threshold]
    for p, v in (("--match-prefix", match), ("--non-match-prefix", non_match)):
        extra += [p, v] if v else []
    want, matched, unmatched = em.elect_reads(items, 25, keys, colours, t=threshold, nrefs=3, pairs=True, match_prefix=match, non_match_prefix=non_match)
    assert len(want) == 6 * (bool(match) + bool(non_match)) and matched and unmatched
    assert sum(1 for n in want if n.endswith("_1.fasta")) == sum(1 for n in want if n.endswith("_2.fasta")) == bool(match) + bool(non_match)
    if threshold == 2:
        # the numeric rule decides some pair differently from the count of bits
        assert want != em.elect_reads(items, 25, keys, colours, t=2, pairs=True, match_prefix=match, non_match_prefix=non_match,
                                      numeric_second_mate=False)[0]
    env = {"GOSS_MATCH_BATCH": 1500} if threshold in (0, 2) else None
    rc, out, err = run_goss(["elect-reads"] + refs + ins + extra + ["--tmp-dir", "scratch", "--dont-write-reads"], tmp_path, env)
    assert rc == 0, err
    assert out == b"" and err == ""
    assert outputs(tmp_path, before) == want and os.listdir(str(tmp)) == []


def test_command_on_a_pool_and_its_refusals(tmp_path):
    refs = write_references(tmp_path)
    items, ins = single_items(tmp_path)
    _, _, keys, colours = ec.command_refs()
    # pool-samples takes the k-mer sets first, then the FASTA files: the colours are then r2, r0, r1
    rc, out, err = run_goss(["pool-samples", "-k", 25, "--kmer-set-in", "r2", "-I", "r0.fa", "-I", "r1.fa", "-O", "pool"], tmp_path)
    assert rc == 0, err
    pooled = [((w >> 2) & 1) | ((w & 3) << 1) for w in colours]
    before = set(os.listdir(str(tmp_path)))
    for threshold in (None, 2):
        want, matched, unmatched = em.elect_reads(items, 25, keys, pooled, t=threshold, nrefs=3, match_prefix="m", non_match_prefix="n")
        extra = [] if threshold is None else ["--ref-threshold", threshold]
        rc, out, err = run_goss(["elect-reads", "--pool", "pool"] + ins + extra + ["--match-prefix", "m", "--non-match-prefix", "n"], tmp_path)
        assert rc == 0 and out == b"", err
        assert outputs(tmp_path, before) == want
        for f in want:
            os.remove(str(tmp_path / f))
    # the sets the pool built, given one by one in the command's own colour order
    rc, out, err = run_goss(["elect-reads", "--ref-index", "pool-a0", "--ref-index", "pool-a1", "--ref-index", "r2", "--ref-threshold", 2] + ins
                            + ["--match-prefix", "m"], tmp_path)
    assert rc == 0, err
    assert outputs(tmp_path, before) == {k: v for k, v in em.elect_reads(items, 25, keys, colours, t=2, match_prefix="m")[0].items()}
    for f in outputs(tmp_path, before):
        os.remove(str(tmp_path / f))
    # a pool of another K; pair files of unequal length name both; an odd number of pair files
    rc, out, err = run_goss(["elect-reads", "--pool", "pool", "-K", 24] + ins + ["--match-prefix", "m"], tmp_path)
    assert rc == 1 and "has k=25, but --kmer-size is 24" in err
    a, b = ec.command_pairs()
    (tmp_path / "a.fq").write_bytes(mm.as_fastq(a))
    (tmp_path / "c.fq").write_bytes(mm.as_fastq(b[:-1]))
    rc, out, err = run_goss(["elect-reads", "--pool", "pool", "-i", "a.fq", "-i", "c.fq", "--pairs", "--match-prefix", "m"], tmp_path)
    assert rc == 1 and "'a.fq' holds 46 reads, 'c.fq' 45" in err
    rc, out, err = run_goss(["elect-reads", "--pool", "pool", "-i", "a.fq", "--pairs", "--match-prefix", "m"], tmp_path)
    assert rc == 1 and "even number" in err
