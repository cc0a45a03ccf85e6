"""`electus index` and `electus classify` against the goss commands they are: the index the files of build-kmer-set over
all the reference files, the elected reads the files of elect-reads with the same line, single and in pairs.  The inputs
are checked on the model (elect_model.py) first: both output sides hold reads."""
import os
import random
import subprocess

import pytest

import elect_model as em
import gossamer_amd as g
import match_model as mm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
ELECTUS = os.path.join(ROOT, "gossamer_amd", "electus")
K = 9


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(g.binding.LIB_PATH) and os.path.exists(GOSS) and os.path.exists(ELECTUS)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])


@pytest.fixture(scope="module")
def world():
    """three references of 300 bases, 40 reads of 30 to 50 bases (half from the references, half from elsewhere) and their
    mates, and what the model elects at --ref-threshold 1 against {c.fa, the index of a.fa and b.fa}"""
    rng = random.Random(31)
    refs = {n: mm.genome(rng, 300) for n in "abc"}
    elsewhere = mm.genome(rng, 3000)

    def draw(src):
        L = rng.randrange(30, 51)
        p = rng.randrange(0, len(src) - L)
        r = src[p:p + L]
        return (mm.rc_text(r) if rng.randrange(2) else r).encode()
    reads = [draw(refs["abc"[i % 3]]) if i % 2 else draw(elsewhere) for i in range(40)]
    mates = [draw(elsewhere) for _ in range(40)]
    files = {n + ".fa": mm.as_fasta([refs[n].encode()]) for n in "abc"}
    files.update({"r.fq": mm.as_fastq(reads), "m.fq": mm.as_fastq(mates)})
    sets = {n: mm.object_keys(refs[n].encode() + b"\n", K, False) for n in "abc"}
    # the references in the command's order: the set built of c.fa, then the index
    keys, colours = em.references([sets["c"], sets["a"] | sets["b"]])
    single = em.elect_reads([("fastq", files["r.fq"])], K, keys, colours, t=1, match_prefix="m", non_match_prefix="n")
    paired = em.elect_reads([("fastq", files["r.fq"]), ("fastq", files["m.fq"])], K, keys, colours, t=1, pairs=True, match_prefix="m",
                            non_match_prefix="n")
    for model_files, matched, unmatched in (single, paired):
        assert matched >= 5 and unmatched >= 5 and all(len(v) > 0 for v in model_files.values()), (matched, unmatched)
    assert sorted(single[0]) == ["m.fastq", "n.fastq"] and sorted(paired[0]) == ["m_1.fastq", "m_2.fastq", "n_1.fastq", "n_2.fastq"]
    return {"files": files, "index_keys": sets["a"] | sets["b"], "single": single, "paired": paired}


def run(exe, args, cwd):
    p = subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def write(world, d):
    for name, data in world["files"].items():
        with open(os.path.join(str(d), name), "wb") as f:
            f.write(data)


def produced(d, world):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in os.listdir(str(d)) if f not in world["files"]}


@pytest.fixture(scope="module")
def indexed(world, tmp_path_factory):
    e, s = tmp_path_factory.mktemp("e"), tmp_path_factory.mktemp("s")
    write(world, e)
    write(world, s)
    rc, eout, eerr = run(ELECTUS, ["index", "-P", "idx", "--ref-fasta", "a.fa", "--ref-fasta", "b.fa", "-K", K, "-M", "1.5", "-v"], e)
    assert rc == 0, eerr
    rc, sout, serr = run(GOSS, ["build-kmer-set", "-k", K, "-I", "a.fa", "-I", "b.fa", "-O", "idx"], s)
    assert rc == 0, serr
    return {"e": e, "s": s, "eout": eout, "eerr": eerr}


def test_index_is_build_kmer_set_over_all_the_references(world, indexed):
    got, want = produced(indexed["e"], world), produced(indexed["s"], world)
    assert sorted(got) == sorted(want) and all(f.startswith("idx.") for f in got) and "idx.kmers.high-bits" in got
    assert all(got[f] == want[f] for f in want)
    assert indexed["eout"] == b""
    # the header's count is the model's: the k-mers of either file
    assert int.from_bytes(got["idx.header"][16:24], "little") == len(world["index_keys"])
    msgs = [line.split("\t", 2)[2] for line in indexed["eerr"].splitlines() if line.count("\t") >= 2]
    assert msgs[0] == "building reference kmer set" and msgs[-1].startswith("total elapsed time: ")
    assert [m.split(" (")[0] for m in msgs if m.startswith("GPU context ")] == ["GPU context created"]


@pytest.mark.parametrize("pairs", [False, True])
def test_classify_is_elect_reads(world, indexed, pairs):
    line = ["--ref-index", "idx", "--ref-fasta", "c.fa", "-K", K, "--ref-threshold", 1, "--match-prefix", "m", "--non-match-prefix", "n"]
    line += ["--pairs", "-i", "r.fq", "-i", "m.fq"] if pairs else ["-i", "r.fq"]
    e, s = indexed["e"], indexed["s"]
    before = {d: set(os.listdir(str(d))) for d in (e, s)}
    try:
        rc, eout, eerr = run(ELECTUS, ["classify"] + line, e)
        assert rc == 0 and eerr == "", eerr
        rc, sout, serr = run(GOSS, ["elect-reads"] + line, s)
        assert rc == 0 and serr == "", serr
        got = {f: v for f, v in produced(e, world).items() if f not in before[e]}
        want = {f: v for f, v in produced(s, world).items() if f not in before[s]}
        assert eout == sout and sorted(got) == sorted(want) and all(got[f] == want[f] for f in want)
        # ... and the model's: the reads' bases, one read per line, in input order
        model_files, matched, unmatched = world["paired" if pairs else "single"]
        assert got == model_files
    finally:
        for d in (e, s):
            for f in set(os.listdir(str(d))) - before[d]:
                os.unlink(os.path.join(str(d), f))
