"""Reads against objects resident in HBM (goss_gpu_object_match_reads, Object.match_reads) and the two commands on
top of it (goss extract-reads, goss filter-reads), against the plain-Python model in match_model.py: per-read windows
and hits in both modes, read starts and the sums, for both object kinds and both key widths; the special inputs; the
refusals; the commands' bytes."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import gossamer_amd as g
import match_cases as mc
import match_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")


def _status(f):
    with pytest.raises(g.GossGpuError) as e:
        f()
    return e.value.status, str(e.value)


def check(obj, data, L, keys, normalize, want=None):
    """both modes of one input against the model; returns the count-mode answer"""
    out = None
    for any_mode in (False, True):
        ew, eh, es, einfo = want[any_mode] if want else mm.match(data, L, keys, normalize=normalize, any=any_mode)
        w, h, s, info = obj.match_reads(data, normalize=normalize, any=any_mode, starts=True)
        assert w.dtype == np.uint32 and h.dtype == np.uint32 and s.dtype == np.uint64
        assert w.tolist() == ew, "windows"
        assert h.tolist() == eh, "hits (any=%s)" % any_mode
        assert s.tolist() == es, "starts"
        assert {n: info[n] for n in einfo} == einfo
        assert info["ms"] >= 0
        out = out or (w, h, s, info)
    return out


# ---- both object kinds, both key widths ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in mc.CASES])
def test_match_against_model(name, oracle):
    import torch
    K, graph, normalize, L, built, keys, query = mc.fixture(name)
    want = {a: mc.expected(name, a) for a in (False, True)}
    # the model's object is the oracle's
    okeys, _, _, _ = oracle.count([(oracle.LINE, "reads", built)], L, 1 if graph else 0)
    assert set(okeys) == keys
    files, _ = (oracle.build_graph if graph else oracle.build_kmer_set)([(oracle.LINE, "reads", built)], K, out="x")
    kind = g.OBJECT_GRAPH if graph else g.OBJECT_KMER_SET
    with g.Context(K, g.MODE_GRAPH if graph else g.MODE_KMER_SET, hbm_budget=256 << 20) as ctx:
        ctx.push_host(built)
        ctx.finish()
        ctx.emit()
        a = g.Object.from_context(ctx)
    with a, g.Object.open(files, "x", kind) as b:
        assert a.key_words == b.key_words == (1 if 2 * L <= 62 else 2)
        for obj in (a, b):
            w, h, s, info = check(obj, query, L, keys, normalize, want)
        # the same input gives the same arrays; a device tensor in, device tensors out
        t = torch.from_numpy(np.frombuffer(query, dtype=np.uint8).copy()).cuda()
        for any_mode in (False, True):
            tw, th, ts, tinfo = a.match_reads(t, normalize=normalize, any=any_mode, starts=True)
            assert isinstance(tw, torch.Tensor) and tw.is_cuda and th.is_cuda and ts.is_cuda
            assert tw.cpu().numpy().view(np.uint32).tolist() == want[any_mode][0]
            assert th.cpu().numpy().view(np.uint32).tolist() == want[any_mode][1]
            assert ts.cpu().numpy().view(np.uint64).tolist() == want[any_mode][2]
        # an input that does not begin on an 8-byte boundary
        t1 = torch.from_numpy(np.frombuffer(b"\n" + query, dtype=np.uint8).copy()).cuda()[1:]
        assert t1.data_ptr() % 8 == 1
        uw, uh, _ = a.match_reads(t1, normalize=normalize)
        assert uw.cpu().numpy().view(np.uint32).tolist() == want[False][0]
        assert uh.cpu().numpy().view(np.uint32).tolist() == want[False][1]
        # numpy in, without the starts
        got = b.match_reads(np.frombuffer(query, dtype=np.uint8), normalize=normalize, any=True)
        assert len(got) == 3 and got[1].tolist() == want[True][1]


# ---- special cases ---------------------------------------------------------------------------------------------------

def test_special_inputs(oracle):
    K = 25
    _, _, _, L, built, keys, query = mc.fixture("kmers25n")
    files = oracle.write_kmer_set(sorted(keys), K, out="ks")
    empty = oracle.write_kmer_set([], K, out="e")
    with g.Object.open(files, "ks", g.OBJECT_KMER_SET) as obj, g.Object.open(empty, "e", g.OBJECT_KMER_SET) as eobj:
        # an empty object: the windows are still exact
        w, h, s, info = check(eobj, query, L, set(), True)
        assert info["windows"] > 0 and info["hits"] == 0 and info["matched_reads"] == 0
        # an empty input, an input of only '\n'
        for o in (obj, eobj):
            w, h, s, info = o.match_reads(b"", starts=True)
            assert len(w) == 0 and len(h) == 0 and s.tolist() == [0] and info["reads"] == 0 and info["windows"] == 0
            w, h, s, info = o.match_reads(b"\n\n\n", starts=True)
            assert w.tolist() == [0, 0, 0] and h.tolist() == [0, 0, 0] and s.tolist() == [0, 1, 2, 2] and info["reads"] == 3
            w, h, s, info = o.match_reads(b"\n", any=True, starts=True)
            assert w.tolist() == [0] and s.tolist() == [0, 0]
        # small inputs around the window length and the tile's edge
        rng = random.Random(5)
        gen = built.split(b"\n")[0]
        for text in (gen[:L - 1], gen[:L], gen[:L] + b"\n", gen[:L + 1] + b"\n\n" + gen[:L],
                     b"N" * 2047 + gen[:L + 3], b"\n" * 2040 + gen[:60] + b"\n" + gen[10:70], gen[:60] * 70):
            check(obj, text, L, keys, True)
        # the long read alone: spread over many workgroups, one pair of counters
        spans = mm.read_spans(query)
        b0, e0 = max(spans, key=lambda se: se[1] - se[0])
        assert e0 - b0 >= 200000
        w, h, s, info = check(obj, query[b0:e0], L, keys, True)
        assert len(w) == 1 and 0 < int(h[0]) < int(w[0])
    # a set that contains every window of the input: every read with a window matches; a disjoint set: none does
    short = mm.query_reads(77, mm.genome(random.Random(1), 5000), L, nreads=200, long_read=30000)
    every = mm.object_keys(short, K, False)
    other = mm.object_keys(mm.build_reads(99)[1], K, False)
    assert not (every & other)
    with g.Object.open(oracle.write_kmer_set(sorted(every), K, out="a"), "a", g.OBJECT_KMER_SET) as obj:
        w, h, info = obj.match_reads(short, normalize=True, any=True)
        assert (h == (w > 0)).all() and info["matched_reads"] == int((w > 0).sum()) > 100
        w2, h2, info2 = obj.match_reads(short, normalize=True)
        assert (h2 == w2).all() and (w2 == w).all() and info2["hits"] == info2["windows"]
    with g.Object.open(oracle.write_kmer_set(sorted(other), K, out="d"), "d", g.OBJECT_KMER_SET) as obj:
        for any_mode in (False, True):
            w, h, info = obj.match_reads(short, normalize=True, any=any_mode)
            assert not h.any() and info["matched_reads"] == 0 and info["windows"] == int(w.sum()) > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    K, graph, normalize, L, built, keys, query = mc.fixture("graph27")
    elems = sorted(keys)
    files = oracle.write_graph(elems, [1] * len(elems), K, out="gr")
    nreads = len(mm.read_spans(query))
    with g.Object.open(files, "gr", g.OBJECT_GRAPH) as obj:
        st, msg = _status(lambda: obj.match_reads(query, max_reads=nreads - 1))
        assert st == -9 and "needs max_reads = %d" % nreads in msg
        w, h, info = obj.match_reads(query, max_reads=nreads + 5)
        assert len(w) == nreads and info["reads"] == nreads
        for bad in (2, 8, 1 << 31):
            st, msg = _status(lambda: obj.match_reads(query, flags=bad))
            assert st == -1 and "flag" in msg
        assert obj.match_reads(b"ACGT\n")[2]["reads"] == 1             # (the object still answers)
    sa = oracle.write_sparse_array([1, 5, 9], 1 << 40, 3, base="sa")
    with g.Object.open(sa, "sa", g.OBJECT_SPARSE_ARRAY) as obj:
        st, msg = _status(lambda: obj.match_reads(b"ACGT\n"))
        assert st == -1 and "SparseArray" in msg
    # A truncated low-bits image whose header's count follows it opens (every size agrees with its header), but the
    # groups of the high-bits index now end past the count: a walk into such a group cannot answer, the call fails
    # and names the first such window instead of answering.
    keep = len(elems) // 2
    low = sorted(n for n in files if n.startswith("gr-edges.low-bits"))
    hdr = bytearray(files["gr-edges.header"])
    assert struct.unpack_from("<Q", hdr, 56)[0] == len(elems)
    D = struct.unpack_from("<Q", hdr, 8)[0]
    struct.pack_into("<Q", hdr, 56, keep)
    damaged = dict(files)
    damaged["gr-edges.header"] = bytes(hdr)
    for n in low:
        width = len(files[n]) // len(elems)
        damaged[n] = files[n][:keep * width]
    highs = np.array([e >> D for e in elems], dtype=np.uint64)

    def fails(x):
        # the group of x's high part ends after the elements whose high part is <= it
        return x < 4 ** L and int(np.searchsorted(highs, np.uint64(x >> D), side="right")) > keep

    with g.Object.open(damaged, "gr", g.OBJECT_GRAPH) as obj:
        at = mm.first_failing_window(query, L, fails)
        assert at is not None
        for any_mode in (False, True):
            st, msg = _status(lambda: obj.match_reads(query, any=any_mode))
            assert st == -1 and "cannot answer" in msg
            if not any_mode:
                assert "byte %d:" % at in msg, (at, msg)
        head = query[:at + L - 1]                                       # every window before it can be answered
        w, h, info = obj.match_reads(head)
        assert info["windows"] > 0 or at == 0


# ---- the commands ------------------------------------------------------------------------------------------------------

def run_goss(args, env_extra=None):
    env = dict(os.environ)
    env.update({k: str(v) for k, v in (env_extra or {}).items()})
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def write_files(folder, files):
    for n, b in files.items():
        with open(os.path.join(folder, n), "wb") as f:
            f.write(b)


def command_inputs(seed, gen, L):
    """four sets of reads (no empty ones: how the parsers frame an empty record is their business, not this test's)"""
    sets = []
    for i in range(4):
        text = mm.query_reads(seed + i, gen, L, nreads=150, long_read=20000 if i == 1 else 0)
        sets.append([r for r in text.split(b"\n") if r])
    return sets


def test_goss_extract_reads(oracle, tmp_path):
    K, graph, _, L, built, keys, _ = mc.fixture("graph27")
    files, _ = oracle.build_graph([(oracle.LINE, "reads", built)], K, out="gr")
    write_files(tmp_path, files)
    gen, _ = mm.build_reads(11)
    sets = command_inputs(300, gen, L)
    inputs = {"a.txt": ("line", b"\n".join(sets[0]) + b"\n"), "b.fa": ("fasta", mm.as_fasta(sets[1])),
              "c.fq": ("fastq", mm.as_fastq(sets[2])), "d.txt": ("line", b"\n".join(sets[3]))}
    write_files(tmp_path, {n: b for n, (_, b) in inputs.items()})
    # the command line's order is not the item order
    order = ["c.fq", "a.txt", "b.fa", "d.txt"]
    args = ["extract-reads", "-G", tmp_path / "gr", "-v"]
    for n in order:
        args += [{"line": "--line-in", "fasta": "--fasta-in", "fastq": "--fastq-in"}[inputs[n][0]], tmp_path / n]
    want, m, n = mm.extract_reads([inputs[x] for x in order], K, keys)
    assert 0.2 * n < m < 0.8 * n
    total = sum(len(r) + 1 for s in sets for r in s)
    batch = 16384
    assert total // batch >= 5
    rc, out, err = run_goss(args, {"GOSS_MATCH_BATCH": batch})
    assert rc == 0, err
    assert out == want
    assert err.strip().splitlines()[-1].endswith("extracted %d reads, out of %d" % (m, n)), err
    rc, out2, err = run_goss(args + ["-o", tmp_path / "out.txt"])          # one batch, a file
    assert rc == 0 and out2 == b"", err
    assert open(tmp_path / "out.txt", "rb").read() == want
    assert err.strip().splitlines()[-1].endswith("extracted %d reads, out of %d" % (m, n))
    # the option table: graph-in exactly once
    rc, _, err = run_goss(["extract-reads", "--line-in", tmp_path / "a.txt"])
    assert rc == 1 and "mandatory option graph-in was not given." in err
    rc, _, err = run_goss(["extract-reads", "-G", tmp_path / "gr", "-G", tmp_path / "gr"])
    assert rc == 1 and "exactly once" in err
    # an asymmetric graph is refused with the reference's message
    hdr = bytearray(files["gr.header"])
    struct.pack_into("<Q", hdr, 16, struct.unpack_from("<Q", hdr, 16)[0] | 1)
    asym = {("as" + n[2:]): b for n, b in files.items()}
    asym["as.header"] = bytes(hdr)
    write_files(tmp_path, asym)
    rc, _, err = run_goss(["extract-reads", "-G", tmp_path / "as", "--line-in", tmp_path / "a.txt"])
    assert rc == 1 and "Asymmetric graphs not yet handled" in err


def test_goss_filter_reads(oracle, tmp_path):
    K, graph, _, L, built, keys, _ = mc.fixture("kmers25n")
    files, _ = oracle.build_kmer_set([(oracle.LINE, "reads", built)], K, out="ks")
    write_files(tmp_path, files)
    gen, _ = mm.build_reads(13)
    sets = command_inputs(400, gen, L)
    sets[1] = sets[1][:len(sets[0])]
    sets[0] = sets[0][:len(sets[1])]
    sets[3] = sets[3][:len(sets[2])]
    sets[2] = sets[2][:len(sets[3])]
    inputs = {"a.fq": ("fastq", mm.as_fastq(sets[0])), "b.fq": ("fastq", mm.as_fastq(sets[1])),
              "c.txt": ("line", b"\n".join(sets[2]) + b"\n"), "d.txt": ("line", b"\n".join(sets[3]) + b"\n")}
    write_files(tmp_path, {n: b for n, (_, b) in inputs.items()})
    order = ["a.fq", "b.fq", "c.txt", "d.txt"]
    items = [inputs[x] for x in order]
    flag = {"line": "--line-in", "fasta": "--fasta-in", "fastq": "--fastq-in"}
    base = ["filter-reads", "-G", tmp_path / "ks", "-v", "--count", "-T", "3"]
    for n in order:
        base += [flag[inputs[n][0]], tmp_path / n]
    env = {"GOSS_MATCH_BATCH": 16384}

    def read(name):
        with open(tmp_path / name, "rb") as f:
            return f.read()

    # unpaired: every read in exactly one of the two files, in input order
    want = mm.filter_reads(items, K, keys, match_name="m.x.txt", non_match_name="n.x.txt")
    rc, out, err = run_goss(base + ["--match-file", tmp_path / "m.x.txt", "--non-match-file", tmp_path / "n.x.txt"], env)
    assert rc == 0 and out == b"", err
    got = {n: read(n) for n in want}
    assert got == want
    every = [r for fmt, text in mm.item_order(items) for r in mm.PARSERS[fmt](text)]
    m, n = got["m.x.txt"].split(b"\n")[:-1], got["n.x.txt"].split(b"\n")[:-1]
    assert len(m) + len(n) == len(every) and 0.2 * len(every) < len(m) < 0.8 * len(every)
    it_m, it_n = iter(m), iter(n)
    hit = {True: it_m, False: it_n}
    for r in every:                                                   # a partition that keeps the order
        assert next(hit[mm._matches(r, K, keys, True)]) == r
    # only one of the two files asked for
    rc, _, err = run_goss(base + ["--non-match-file", tmp_path / "only_n.txt"], env)
    assert rc == 0 and read("only_n.txt") == want["n.x.txt"] and not os.path.exists(tmp_path / "m.txt")
    # pairs: files 2i and 2i + 1 in lockstep, a pair matches when either mate does
    want = mm.filter_reads(items, K, keys, pairs=True, match_name="pm.x.txt", non_match_name="pn.x.txt")
    assert sorted(want) == ["pm.x_1.txt", "pm.x_2.txt", "pn.x_1.txt", "pn.x_2.txt"]
    rc, out, err = run_goss(base + ["--pairs", "--match-file", tmp_path / "pm.x.txt", "--non-match-file", tmp_path / "pn.x.txt"], env)
    assert rc == 0, err
    got = {n: read(n) for n in want}
    assert got == want
    assert got["pm.x_1.txt"].count(b"\n") == got["pm.x_2.txt"].count(b"\n") > 0
    assert got["pn.x_1.txt"].count(b"\n") == got["pn.x_2.txt"].count(b"\n") > 0
    mates1 = [r for x in ("a.fq", "c.txt") for r in mm.PARSERS[inputs[x][0]](inputs[x][1])]
    assert sorted(got["pm.x_1.txt"].split(b"\n")[:-1] + got["pn.x_1.txt"].split(b"\n")[:-1]) == sorted(mates1)
    # an odd number of files, and files of unequal read counts
    rc, _, err = run_goss(base[:-2] + ["--pairs", "--match-file", tmp_path / "q.txt"], env)
    assert rc == 1 and "an even number of input files is required" in err
    write_files(tmp_path, {"short.txt": b"\n".join(sets[3][:-1]) + b"\n"})
    rc, _, err = run_goss(base[:-2] + ["--line-in", tmp_path / "short.txt", "--pairs", "--match-file", tmp_path / "q.txt"], env)
    assert rc == 1 and "reads" in err
