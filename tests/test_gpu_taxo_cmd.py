"""`goss annotate-kmers` followed by `goss classify-reads` against the model (tests/taxo_model.py) on cases of
tests/taxo_cases.py: the bytes of <set>.annotation, the phylogeny written back, the table on standard output, and the
annotation file loaded through Object.taxo_annotation."""
import os
import subprocess

import numpy as np
import pytest

import gossamer_amd as g
import match_model as mm
import oracle_lib as o
import taxo_cases as tc
import taxo_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
KINDS = ("root", "clade", "species")


def run_goss(args, cwd, env_extra=None):
    env = dict(os.environ)
    env.update({k: str(v) for k, v in (env_extra or {}).items()})
    p = subprocess.run([GOSS] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env, cwd=str(cwd))
    return p.returncode, p.stdout, p.stderr.decode()


def reads_of(data):
    """the reads that are not empty (how the parsers frame an empty record is their business)"""
    return [data[b:e] for b, e in mm.read_spans(data) if e > b]


def phylogeny_of(t):
    """the tree as a parsed phylogeny with a kind and a stray annotation on every node, and its text, loosely laid out"""
    names = ["taxon_%d" % x for x in t.ids]
    kinds = [KINDS[min(t.depth(x), 2)] for x in t.ids]
    root = tm.nested(t, names, kinds)
    nodes, _ = tm.flatten(root)
    for i, n in enumerate(nodes):
        if i % 3 == 0:
            n["anns"]["Zone"] = "z%d" % i       # (sorts before every lower-case key)
    toks = []

    def walk(n):
        toks.append("(")
        for k in sorted(n["anns"], reverse=True):
            toks.extend([k, n["anns"][k]])
        for c in n["kids"]:
            walk(c)
        toks.append(")")
    walk(root)
    text = "".join(tok + (" ", "\n", "\t", "  ")[i % 4] for i, tok in enumerate(toks))
    return root, text


@pytest.mark.parametrize("name,K,pairs", [("star70", 15, False), ("bin127", 31, False), ("rand1000", 32, True)])
def test_annotate_then_classify(tmp_path, name, K, pairs):
    c, exp = tc.fixture(name, K), tc.expected(name, K)
    t, keys = c["tree"], c["keys"]
    for fname, data in o.write_kmer_set(keys, K, out="u").items():
        (tmp_path / fname).write_bytes(data)
    root, text = phylogeny_of(t)
    (tmp_path / "phylo.txt").write_text(text)
    # the annotation list: a FASTA file per item, the wave lines a file each; the first file is listed twice, and its last
    # id holds
    listing, n = [], 0
    for data, ids in tc.batches(name, K):
        spans = mm.read_spans(data)
        groups = [(data, ids[0])] if len(set(ids)) == 1 else [(data[b:e], x) for (b, e), x in zip(spans, ids)]
        for d, node in groups:
            (tmp_path / ("g%d.fa" % n)).write_bytes(mm.as_fasta(reads_of(d)))
            listing.append("g%d.fa %d" % (n, node))
            n += 1
    wrong = next(x for x in t.ids if x != int(listing[0].split()[1]))
    (tmp_path / "list.txt").write_text("g0.fa %d\n" % wrong + "\n".join(listing[1:]) + "\t" + listing[0] + "\n")
    assert n > 100 or not c["W"]

    rc, out, err = run_goss(["annotate-kmers", "-G", "u", "--annotation-list", "list.txt", "--phylogeny", "phylo.txt", "-T", "2"], tmp_path,
                            {"GOSS_MATCH_BATCH": 700})
    assert rc == 0 and out == b"", err
    ann_bytes = (tmp_path / "u.annotation").read_bytes()
    assert ann_bytes == np.array(exp["ann"], dtype=np.uint32).tobytes()
    want = g.format_phylogeny(tm.with_counts(g.parse_phylogeny(text), t, exp["counts"]))
    got = (tmp_path / "phylo.txt").read_text()
    assert got == want == tm.format_phylogeny(tm.with_counts(root, t, exp["counts"]))
    assert "\n count\t%d\n" % exp["counts"][t.root] in got and "\n total\t%d\n" % sum(exp["counts"]) in got
    # once more over its own output, in one batch: the same bytes
    rc, out, err = run_goss(["annotate-kmers", "-G", "u", "--annotation-list", "list.txt", "--phylogeny", "phylo.txt"], tmp_path)
    assert rc == 0, err
    assert (tmp_path / "u.annotation").read_bytes() == ann_bytes and (tmp_path / "phylo.txt").read_text() == want

    (tmp_path / "u.taxo").write_text(got)
    if not pairs:
        reads = reads_of(c["data"])
        cut = [0, len(reads) // 4, len(reads) // 2, len(reads)]
        # given as FASTQ, FASTA, lines; read as lines, FASTA, FASTQ
        (tmp_path / "r.fq").write_bytes(mm.as_fastq(reads[cut[2]:]))
        (tmp_path / "r.fa").write_bytes(mm.as_fasta(reads[cut[1]:cut[2]]))
        (tmp_path / "r.txt").write_bytes(b"\n".join(reads[:cut[1]]) + b"\n")
        args = ["-i", "r.fq", "-I", "r.fa", "--line-in", "r.txt"]
        results = [r for r, (b, e) in zip(exp["result"], mm.read_spans(c["data"])) if e > b]
    else:
        a, b = c["pairs"]
        h = len(a) // 2
        (tmp_path / "a1.fa").write_bytes(mm.as_fasta([x.encode() for x in a[:h]]))
        (tmp_path / "b1.fa").write_bytes(mm.as_fasta([x.encode() for x in b[:h]]))
        (tmp_path / "a2.fq").write_bytes(mm.as_fastq([x.encode() for x in a[h:]]))
        (tmp_path / "b2.fq").write_bytes(mm.as_fastq([x.encode() for x in b[h:]]))
        args = ["--pairs", "-I", "a1.fa", "-I", "b1.fa", "-i", "a2.fq", "-i", "b2.fq"]
        results = exp["pair"]
        assert tm.MANY in results and tm.NONE in results
    want_out = tm.table(g.parse_phylogeny(got), t, tm.node_counts(t, results)).encode()
    assert want_out.count(b"\n") >= 2
    for env in ({"GOSS_MATCH_BATCH": 900}, None):
        rc, out, err = run_goss(["classify-reads", "-G", "u", "-B", "1", "-T", "3"] + args, tmp_path, env)
        assert rc == 0, err
        assert out == want_out
    if pairs:
        (tmp_path / "b2.fq").write_bytes(mm.as_fastq([x.encode() for x in b[h:-1]]))
        rc, out, err = run_goss(["classify-reads", "-G", "u"] + args, tmp_path)
        assert rc == 1 and out == b"" and "'a2.fq' holds %d reads, 'b2.fq' %d" % (len(a) - h, len(a) - h - 1) in err

    # the file the command wrote, loaded through the binding, classifies as the annotation made in memory does
    with g.Object.open(o.write_kmer_set(keys, K, out="ks"), "ks", g.OBJECT_KMER_SET) as obj:
        obj.taxo_tree(t.ids, t.parent)
        obj.taxo_annotation(ann_bytes)
        res, nwin, info = obj.taxo_classify_reads(c["data"])
        assert (res.tolist(), nwin.tolist()) == (exp["result"], exp["windows"])
        assert obj.taxo_read_annotation()[1].tolist() == exp["counts"]
        # an annotation with an id the phylogeny lacks: the command names the id and the rank
        missing = next(x for x in range(1, 1 << 20) if x not in t.index)
        bad = np.frombuffer(ann_bytes, dtype=np.uint32).copy()
        bad[[9, 800]] = missing
    (tmp_path / "u.annotation").write_bytes(bad.tobytes())
    rc, out, err = run_goss(["classify-reads", "-G", "u"] + args, tmp_path)
    assert rc == 1 and out == b"" and "rank 9 has node id %d" % missing in err
