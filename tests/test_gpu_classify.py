"""Reads classified on the device (goss_gpu_object_classify_reads, Object.classify_reads / classify_bits,
`goss group-reads`) against the model (tests/classify_model.py) over the corpus of tests/classify_cases.py, which
test_classify_cpu.py holds to its claims.  Sets are written with the oracle and opened with Object.open."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import classify_cases as cc
import classify_model as cm
import gossamer_amd as g
import match_model as mm
import near_model as nm
import oracle_lib as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


def open_set(keys, K):
    return g.Object.open(o.write_kmer_set(keys, K, out="ks"), "ks", g.OBJECT_KMER_SET)


def words(bits, n):
    """(count + 63) // 64 words: what the calls take (the files hold one word for an empty set)"""
    return np.array(nm.pack_bits(bits)[:(n + 63) // 64], dtype=np.uint64)


def lists(t, dtype):
    import torch
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy().view(dtype)
    assert t.dtype == dtype
    return t.tolist()


def check_info(info, classes, nwin, counts):
    assert {k: info[k] for k in ("reads", "windows", "counts")} == {"reads": len(classes), "windows": sum(nwin), "counts": counts}
    assert sum(info["counts"]) == info["reads"] and info["ms"] >= 0


@pytest.mark.parametrize("name", cc.NAMES)
def test_corpus(name):
    import torch
    c = cc.fixture(name)
    K, keys, data = c["K"], c["keys"], c["data"]
    classes, nwin, counts = cc.expected(name)
    starts = mm.read_starts(data)
    n = len(keys)
    wl, wr = words(c["lhs"], n), words(c["rhs"], n)
    with open_set(keys, K) as obj:
        assert obj.count == n
        # bytes in, numpy out, the bitmaps per call
        gc, gw, gs, info = obj.classify_reads(data, wl, wr, starts=True)
        assert (lists(gc, np.uint32), lists(gw, np.uint32), lists(gs, np.uint64)) == (classes, nwin, starts)
        check_info(info, classes, nwin, counts)
        # what match_reads says of the same bytes
        mw, mh, _ = obj.match_reads(data, normalize=True)
        assert mw.tolist() == nwin
        aw, ah, _ = obj.match_reads(data, normalize=True, any=True)
        assert [1 if x else 0 for x in classes] == ah.tolist() == [1 if h else 0 for h in mh.tolist()]
        # the pair kept; numpy in; the bitmaps as the bytes of their files
        obj.classify_bits(wl.tobytes(), wr.tobytes())
        gc, gw, info = obj.classify_reads(np.frombuffer(data, dtype=np.uint8))
        assert (lists(gc, np.uint32), lists(gw, np.uint32)) == (classes, nwin)
        check_info(info, classes, nwin, counts)
        # a device tensor that begins at 1 mod 8, device bitmaps; tensors come back
        t1 = torch.from_numpy(np.frombuffer(b"\n" + data, dtype=np.uint8).copy()).cuda()[1:]
        assert t1.data_ptr() % 8 == 1
        tl, tr = (torch.from_numpy(w.view(np.int64).copy()).cuda() for w in (wl, wr))
        gc, gw, gs, info = obj.classify_reads(t1, tl, tr, starts=True)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (gc, gw, gs))
        assert (lists(gc, np.uint32), lists(gw, np.uint32), lists(gs, np.uint64)) == (classes, nwin, starts)
        check_info(info, classes, nwin, counts)
        # only the counts are wanted
        inf = g.binding.ClassifyInfo()
        assert obj._L.goss_gpu_object_classify_reads(obj._h, t1.data_ptr(), t1.numel(), None, None, g.CLASSIFY_NORMALIZE, 0, None, None, None,
                                                     C.byref(inf)) == 0
        check_info(inf.as_dict(), classes, nwin, counts)


def test_without_normalize_the_windows_are_looked_up_as_they_stand():
    c = cc.fixture("sixteen25")
    keys = c["keys"]
    rank_of = {x: i for i, x in enumerate(keys)}
    exp = []
    for b, e in mm.read_spans(c["data"]):
        m = 0
        for _, x, _ in mm.windows(c["data"][b:e], 25):
            if x in rank_of:
                m |= 1 << ((c["lhs"][rank_of[x]] << 1) | c["rhs"][rank_of[x]])
        exp.append(m)
    assert exp != cc.expected("sixteen25")[0]
    with open_set(keys, 25) as obj:
        gc, _, _ = obj.classify_reads(c["data"], words(c["lhs"], len(keys)), words(c["rhs"], len(keys)), normalize=False)
        assert gc.tolist() == exp


def test_special_inputs():
    c = cc.fixture("sixteen25")
    n = len(c["keys"])
    wl, wr = words(c["lhs"], n), words(c["rhs"], n)
    with open_set(c["keys"], 25) as obj:
        obj.classify_bits(wl, wr)
        gc, gw, gs, info = obj.classify_reads(b"", starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == ([], [], [0]) and info["reads"] == 0 and info["counts"] == [0] * 16
        gc, gw, gs, info = obj.classify_reads(b"\n\n\n", starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == ([0, 0, 0], [0, 0, 0], [0, 1, 2, 2]) and info["counts"] == [3] + [0] * 15
        # a last read without its newline
        classes, nwin, counts = cc.expected("sixteen25")
        last = cc.genomes(25)[0][3][100:160].encode()
        data = c["data"] + last
        gc, gw, gs, info = obj.classify_reads(data, starts=True)
        assert (gc.tolist(), gw.tolist(), gs.tolist()) == (classes + [8], nwin + [36], mm.read_starts(data))
        assert gs.tolist()[-1] == len(data) and info["counts"] == [x + (m == 8) for m, x in enumerate(counts)]
    # an empty set: nothing is in it, with bitmaps, without, and with a kept pair
    with open_set([], 25) as obj:
        assert obj.count == 0
        empty = np.zeros(0, dtype=np.uint64)
        for args in ((empty, empty), ()):
            gc, gw, info = obj.classify_reads(c["data"], *args)
            assert gc.tolist() == [0] * len(classes) and gw.tolist() == nwin and info["counts"] == [len(classes)] + [0] * 15
        obj.classify_bits(nm.words_to_bytes(nm.pack_bits([])), nm.words_to_bytes(nm.pack_bits([])))
        assert obj.classify_reads(c["data"])[0].tolist() == [0] * len(classes)


def test_refusals():
    c = cc.fixture("sixteen25")
    K, keys, data = 25, c["keys"], c["data"]
    n = len(keys)
    wl, wr = words(c["lhs"], n), words(c["rhs"], n)
    classes, nwin, counts = cc.expected("sixteen25")
    # a graph object
    edges = sorted({v for x in keys[:200] for v in (x, o.revcomp(x, K))})
    with g.Object.open(o.write_graph(edges, [1] * len(edges), K - 1, out="gr"), "gr", g.OBJECT_GRAPH) as gr:
        z = np.zeros((gr.count + 63) // 64, dtype=np.uint64)
        with pytest.raises(g.GossGpuError) as e:
            gr.classify_reads(data, z, z)
        assert e.value.status == -1 and "KmerSet" in str(e.value)
        with pytest.raises(g.GossGpuError) as e:
            gr.classify_bits(z, z)
        assert e.value.status == -1 and "KmerSet" in str(e.value)
    with open_set(keys, K) as obj:
        # no kept pair
        with pytest.raises(g.GossGpuError) as e:
            obj.classify_reads(data)
        assert e.value.status == -1 and "none kept" in str(e.value)
        # one bitmap NULL
        for a, b in ((wl, None), (None, wr)):
            with pytest.raises(g.GossGpuError) as e:
                obj.classify_reads(data, a, b)
            assert e.value.status == -1 and "one bitmap" in str(e.value)
        # an unknown flag
        for flags in (2, 4, 1 << 31):
            with pytest.raises(g.GossGpuError) as e:
                obj.classify_reads(data, wl, wr, flags=flags)
            assert e.value.status == -1 and "flag" in str(e.value)
        # max_reads one too small: the need comes back
        with pytest.raises(g.GossGpuError) as e:
            obj.classify_reads(data, wl, wr, max_reads=len(classes) - 1)
        assert e.value.status == g.binding.ERR_BUFFER and "max_reads = %d" % len(classes) in str(e.value)
        # and the object still answers, with room to spare too
        gc, gw, info = obj.classify_reads(data, wl, wr, max_reads=len(classes) + 5)
        assert (gc.tolist(), gw.tolist(), info["counts"]) == (classes, nwin, counts)


def test_classify_bits_twice_replaces_the_pair():
    c = cc.fixture("ranks129")
    n = len(c["keys"])
    classes = cc.expected("ranks129")[0]
    with open_set(c["keys"], 25) as obj:
        obj.classify_bits(words(c["lhs"], n), words(c["rhs"], n))
        assert obj.classify_reads(c["data"])[0].tolist() == classes
        obj.classify_bits(words(c["rhs"], n), words(c["lhs"], n))                # the two sides exchanged
        swap = {1: 1, 2: 4, 4: 2, 8: 8}
        assert obj.classify_reads(c["data"])[0].tolist() == [swap[m] for m in classes]
        obj.classify_bits(words([1] * n, n), words([1] * n, n))
        assert obj.classify_reads(c["data"])[0].tolist() == [8] * n
        # a pair given with the call is used for that call only
        assert obj.classify_reads(c["data"], words(c["lhs"], n), words(c["rhs"], n))[0].tolist() == classes
        assert obj.classify_reads(c["data"])[0].tolist() == [8] * n


# ---- the command -------------------------------------------------------------------------------------------------------

def run_goss(args, cwd, env_extra=None):
    env = dict(os.environ)
    env.update({k: str(v) for k, v in (env_extra or {}).items()})
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env, cwd=str(cwd))
    return p.returncode, p.stdout, p.stderr.decode()


def write_index(folder, base, keys, K, lhs, rhs):
    files = dict(o.write_kmer_set(keys, K, out=base))
    files.update(cm.bitmap_files(base, lhs, rhs))
    for name, data in files.items():
        (folder / name).write_bytes(data)


def outputs(folder, before):
    return {f: (folder / f).read_bytes() for f in os.listdir(str(folder)) if f not in before}


def sixteen_command_reads():
    """the reads of sixteen25 that are not empty (how the parsers frame an empty record is their business)"""
    return [t.encode() for _, t in cc.sixteen_reads(25) if t]


FLAG = {"line": "--line-in", "fasta": "-I", "fastq": "-i"}
AS = {"line": lambda r: b"\n".join(r) + b"\n", "fasta": mm.as_fasta, "fastq": mm.as_fastq}


@pytest.mark.parametrize("fmt", ["line", "fasta", "fastq"])
def test_command_on_sixteen(tmp_path, fmt):
    _, _, keys, lhs, rhs = cc.genomes(25)
    write_index(tmp_path, "u", keys, 25, lhs, rhs)
    reads = sixteen_command_reads()
    halves = [reads[:len(reads) // 2], reads[len(reads) // 2:]]
    items = [(fmt, AS[fmt](h)) for h in halves]
    args = ["group-reads", "-G", "u"]
    for i, (_, text) in enumerate(items):
        (tmp_path / ("r%d" % i)).write_bytes(text)
        args += [FLAG[fmt], "r%d" % i]
    before = set(os.listdir(str(tmp_path)))
    total = sum(len(r) + 1 for r in reads)
    assert total // 1024 >= 4
    variants = [({}, {}, {"GOSS_MATCH_BATCH": 1024}),
                ({"prefix": "p", "lhs_name": "graft", "rhs_name": "host"}, {}, None),
                ({"lhs_name": ""}, {}, {"GOSS_MATCH_BATCH": 1500})]
    for kw, _, env in variants:
        extra = []
        if "prefix" in kw:
            extra += ["--output-filename-prefix", kw["prefix"]]
        if "lhs_name" in kw:
            extra += ["--lhs-name", kw["lhs_name"]]
        if "rhs_name" in kw:
            extra += ["--rhs-name", kw["rhs_name"]]
        want_files, want_out = cm.group_reads(items, 25, keys, lhs, rhs, **kw)
        assert len(want_files) == 5 and all(want_files.values())
        rc, out, err = run_goss(args + extra + ["-M", "1.5", "-T", "2", "--preserve-read-order"], tmp_path, env)
        assert rc == 0, err
        assert out == want_out
        assert outputs(tmp_path, before) == want_files
        for f in want_files:
            os.remove(str(tmp_path / f))
    # -v: the messages, in the reference's order
    rc, out, err = run_goss(args + ["-v"], tmp_path)
    assert rc == 0 and out == cm.group_reads(items, 25, keys, lhs, rhs)[1], err
    msgs = [line.split("\t", 2)[2] for line in err.splitlines() if line.count("\t") >= 2]
    suf = cm.SUFFIX[fmt]
    assert msgs[:7] == ["performing 1 pass"] + ["writing to %s.%s" % (n, suf) for n in ("neither", "both", "lhs", "rhs", "ambiguous")] + ["pass 0"]
    assert msgs[-1].startswith("total elapsed time: ")
    for f in outputs(tmp_path, before):
        os.remove(str(tmp_path / f))
    # --dont-write-reads: one line, no file
    rc, out, err = run_goss(args + ["--dont-write-reads"], tmp_path, {"GOSS_MATCH_BATCH": 1024})
    assert rc == 0 and out == cm.group_reads(items, 25, keys, lhs, rhs, dont_write=True)[1], err
    assert out.count(b"\n") == 1 and out.count(b"\t") == 4
    assert outputs(tmp_path, before) == {}


def test_command_processes_one_group_of_inputs(tmp_path):
    _, _, keys, lhs, rhs = cc.genomes(25)
    write_index(tmp_path, "u", keys, 25, lhs, rhs)
    reads = sixteen_command_reads()
    items = [("fastq", mm.as_fastq(reads[:30])), ("line", AS["line"](reads[30:50])), ("fasta", mm.as_fasta(reads[50:60]))]
    for i, (_, text) in enumerate(items):
        (tmp_path / ("r%d" % i)).write_bytes(text)
    before = set(os.listdir(str(tmp_path)))
    # lines and FASTQ (and FASTA) given: only the lines are processed
    want_files, want_out = cm.group_reads(items, 25, keys, lhs, rhs)
    assert sum(v.count(b"\n") for v in want_files.values()) == 20 and all(n.endswith(".txt") for n in want_files)
    rc, out, err = run_goss(["group-reads", "-G", "u", "-i", "r0", "--line-in", "r1", "-I", "r2"], tmp_path)
    assert rc == 0 and out == want_out, err
    assert outputs(tmp_path, before) == want_files
    for f in want_files:
        os.remove(str(tmp_path / f))
    # FASTA wins over FASTQ
    want_files, want_out = cm.group_reads([items[0], items[2]], 25, keys, lhs, rhs)
    assert sum(v.count(b"\n") for v in want_files.values()) == 10 and all(n.endswith(".fasta") for n in want_files)
    rc, out, err = run_goss(["group-reads", "-G", "u", "-i", "r0", "-I", "r2"], tmp_path)
    assert rc == 0 and out == want_out, err
    assert outputs(tmp_path, before) == want_files


def test_command_on_pairs(tmp_path):
    _, _, keys, lhs, rhs = cc.genomes(25)
    write_index(tmp_path, "u", keys, 25, lhs, rhs)
    a, b, _ = cc.pairs()
    items = [("fastq", mm.as_fastq(a)), ("fastq", mm.as_fastq(b))]
    (tmp_path / "a.fq").write_bytes(items[0][1])
    (tmp_path / "b.fq").write_bytes(items[1][1])
    before = set(os.listdir(str(tmp_path)))
    args = ["group-reads", "-G", "u", "-i", "a.fq", "-i", "b.fq", "--pairs"]
    assert sum(len(r) + 1 for r in a) // 1500 >= 3
    for kw, extra, env in (({}, [], {"GOSS_MATCH_BATCH": 1500}), ({"prefix": "x", "rhs_name": ""}, ["--output-filename-prefix", "x", "--rhs-name", ""], None)):
        want_files, want_out = cm.group_reads(items, 25, keys, lhs, rhs, pairs=True, **kw)
        assert len(want_files) == 10 and all(want_files.values())
        rc, out, err = run_goss(args + extra, tmp_path, env)
        assert rc == 0 and out == want_out, err
        assert outputs(tmp_path, before) == want_files
        for f in want_files:
            os.remove(str(tmp_path / f))
    rc, out, err = run_goss(args + ["-v"], tmp_path)
    assert rc == 0, err
    msgs = [line.split("\t", 2)[2] for line in err.splitlines() if line.count("\t") >= 2]
    assert msgs[1:11] == ["writing to %s_%d.fastq" % (n, h) for n in ("neither", "both", "ambiguous", "lhs", "rhs") for h in (1, 2)]
    for f in outputs(tmp_path, before):
        os.remove(str(tmp_path / f))
    rc, out, err = run_goss(args + ["--dont-write-reads"], tmp_path)
    assert rc == 0 and out == cm.group_reads(items, 25, keys, lhs, rhs, pairs=True, dont_write=True)[1], err
    assert outputs(tmp_path, before) == {}
    # files of unequal length: an error that names both; an odd number of files: an error
    (tmp_path / "c.fq").write_bytes(mm.as_fastq(b[:-1]))
    rc, out, err = run_goss(["group-reads", "-G", "u", "-i", "a.fq", "-i", "c.fq", "--pairs", "--dont-write-reads"], tmp_path)
    assert rc == 1 and "'a.fq' holds 40 reads, 'c.fq' 39" in err
    rc, out, err = run_goss(["group-reads", "-G", "u", "-i", "a.fq", "--pairs"], tmp_path)
    assert rc == 1 and "even number" in err


def test_index_then_classify_end_to_end(tmp_path):
    """build-kmer-set twice, merge-and-annotate-kmer-sets, compute-near-kmers, group-reads: what `xenome index` and
    `xenome classify` run.  The class files and the table equal the model applied to the model's index."""
    K = 25
    rng = random.Random(7)
    A = [rng.randrange(4) for _ in range(1500)]
    B = list(A)
    for p in range(25, 1500, 50):
        B[p] = (B[p] + rng.randrange(1, 4)) % 4
    for p in range(700, 1000):                                    # a stretch of B's own
        B[p] = rng.randrange(4)
    text = {"a": "".join("ACGT"[c] for c in A), "b": "".join("ACGT"[c] for c in B)}
    files = {}
    for name in ("a", "b"):
        fa = (">%s\n%s\n" % (name, text[name])).encode()
        (tmp_path / (name + ".fa")).write_bytes(fa)
        rc, _, err = run_goss(["build-kmer-set", "-k", K, "-I", name + ".fa", "-O", name], tmp_path)
        assert rc == 0, err
        files.update(o.build_kmer_set([(o.FASTA, name + ".fa", fa)], K, out=name)[0])
    rc, _, err = run_goss(["merge-and-annotate-kmer-sets", "-G", "a", "-G", "b", "-O", "u"], tmp_path)
    assert rc == 0, err
    rc, _, err = run_goss(["compute-near-kmers", "-G", "u"], tmp_path)
    assert rc == 0, err
    # the model's index
    exp, _ = o.merge_and_annotate(files, "a", "b", "u")
    rd = o.SparseReader(exp, "u.kmers")
    n = rd.count()
    keys = [rd.select(i) for i in range(n)]
    lhs, rhs, gray = nm.near_kmers(keys, nm.unpack_bits(nm.bytes_to_words(exp["u.lhs-bits"]), n),
                                   nm.unpack_bits(nm.bytes_to_words(exp["u.rhs-bits"]), n), K)
    assert gray >= 20 and {(x, y) for x, y in zip(lhs, rhs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # reads of 100 and of 30 bases (the short ones fit between two differences) from either genome, either strand, and
    # from neither
    reads = []
    for i in range(120):
        src = (text["a"], text["b"], mm.genome(rng, 1500))[i % 3]
        p = rng.randrange(1400)
        r = src[p:p + (100 if i % 4 < 2 else 30)]
        reads.append((r if i % 2 else mm.rc_text(r)).encode())
    items = [("fastq", mm.as_fastq(reads))]
    (tmp_path / "r.fq").write_bytes(items[0][1])
    want_files, want_out = cm.group_reads(items, K, keys, lhs, rhs, lhs_name="graft", rhs_name="host")
    assert sum(1 for v in want_files.values() if v) >= 4
    before = set(os.listdir(str(tmp_path)))
    rc, out, err = run_goss(["group-reads", "-G", "u", "-i", "r.fq", "--lhs-name", "graft", "--rhs-name", "host"], tmp_path,
                            {"GOSS_MATCH_BATCH": 4096})
    assert rc == 0 and out == want_out, err
    assert outputs(tmp_path, before) == want_files
