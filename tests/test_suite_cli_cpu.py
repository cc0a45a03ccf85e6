"""CPU-only: the surface of the `xenome` and `electus` executables -- their command lists, every command's options, and the
answers to unknown commands, unknown options, missing mandatory options and non-numbers -- each held against what `goss`
answers in the same place, and `goss help` / `translucent help` byte for byte what they were.  Every answer here is
decided before a command object does any device work, so none needs a GPU."""
import os
import subprocess
import sys

import pytest

import gossamer_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = {n: os.path.join(ROOT, "gossamer_amd", n) for n in ("goss", "translucent", "xenome", "electus")}
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_cli_surface as surface  # noqa: E402

# the commands in help order (XenoApp.cc:274-276, ElectApp.cc:802-804) and their sentences
LISTS = {
    "xenome": [("index", "build an index for classifying reads"), ("classify", "classify reads according to index"),
               ("help", "print a summary of all the commands.")],
    "electus": [("classify", "classify reads according to reference"), ("index", "build an index for classifying reads"),
                ("help", "print a summary of all the commands.")],
}
GLOBAL = ["debug", "help", "log-file", "tmp-dir", "num-threads", "verbose", "version"]
GPU = ["device", "devices", "hbm-budget"]
# every command's own options, in the order -h prints them between goss's global options and this build's three
OPTIONS = {
    ("xenome", "index"): ["prefix", "max-memory", "kmer-size", "graft", "host"],
    ("xenome", "classify"): ["fasta-in", "fastq-in", "line-in", "prefix", "max-memory", "pairs", "graft-name", "host-name",
                             "output-filename-prefix", "dont-write-reads", "preserve-read-order"],
    ("electus", "index"): ["ref-fasta", "max-memory", "kmer-size", "prefix"],
    ("electus", "classify"): ["ref-fasta", "ref-index", "pool", "fasta-in", "fastq-in", "line-in", "max-memory", "kmer-size", "pairs",
                              "dont-write-reads", "preserve-read-order", "ref-threshold", "match-prefix", "non-match-prefix"],
}
SHORT = {"prefix": "P", "max-memory": "M", "kmer-size": "K", "graft": "G", "host": "H", "fasta-in": "I", "fastq-in": "i"}
APPS = sorted(LISTS)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(g.binding.LIB_PATH) and all(os.path.exists(b) for b in BIN.values())):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])


def run(exe, *args, cwd=None):
    p = subprocess.run([BIN[exe]] + [str(a) for a in args], cwd=cwd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def listing(app):
    """what `<app> help` prints, from the table above, in the layout of goss's own list"""
    text = "%s <command> [options]\n\ncommands implemented by this build:\n" % app
    for name, summary in LISTS[app]:
        text += "  " + name.ljust(max(17, len(name) + 2)) + summary + "\n"
    return text


def use(app, cmd):
    return "use\n\t%s %s -h\nfor more usage information.\n" % (app, cmd)


def option_names(help_text, cmd):
    """the long names of the options in a command's -h text, in order"""
    body = help_text.split("\n%s\n" % cmd, 1)[1]
    names = []
    for line in body.splitlines():
        if line.startswith("  "):
            names.append(line.split("--", 1)[1].split()[0])
    return names


@pytest.fixture(scope="module")
def goss_entries():
    return {tuple(e["argv"]): e for e in surface.load()}


# ---- the lists -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("app", APPS)
def test_help_lists_exactly_the_commands_in_the_reference_order(app):
    for args in ((), ("help",), ("-h",), ("--help",)):
        rc, out, err = run(app, *args)
        assert (rc, out) == (0, "") and err == listing(app), args
        assert "goss" not in err


@pytest.mark.parametrize("app", APPS)
def test_version_is_answered_under_the_own_name(app):
    rc, out, err = run(app, "--version")
    grc, gout, gerr = run("goss", "--version")
    assert (rc, err) == (grc, gerr) == (0, "") and out.startswith(app + " version ")
    assert out == gout.replace("goss", app, 1)
    assert run(app, "index", "--version")[1] == out


@pytest.mark.parametrize("app", APPS)
def test_an_unknown_command_is_answered_as_goss_answers_one(app, goss_entries):
    e = goss_entries[("nosuch",)] if ("nosuch",) in goss_entries else None
    grc, gout, gerr = run("goss", "nosuch")
    assert (grc, gout) == (0, "") and gerr == "unknown command 'nosuch'\n" + goss_entries[("help",)]["stderr"]
    assert e is None or e["stderr"] == gerr
    rc, out, err = run(app, "nosuch")
    assert (rc, out) == (0, "") and err == "unknown command 'nosuch'\n" + listing(app)


@pytest.mark.parametrize("app", APPS)
def test_every_goss_command_is_unknown_and_goss_knows_neither_index_nor_classify(app, goss_entries):
    assert len(surface.COMMANDS) == 28
    for cmd in surface.COMMANDS + ["synth-reads", "dump-bases", "trim-relative"]:
        rc, out, err = run(app, cmd, "-h")
        assert (rc, out) == (0, "") and err == "unknown command '%s'\n" % cmd + listing(app), cmd
    for cmd in ("index", "classify"):
        rc, out, err = run("goss", cmd)
        assert (rc, out) == (0, "") and err == "unknown command '%s'\n" % cmd + goss_entries[("help",)]["stderr"]


# ---- every command's options -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("app,cmd", sorted(OPTIONS))
def test_dash_h_shows_exactly_the_commands_options(app, cmd):
    rc, out, err = run(app, cmd, "-h")
    assert (rc, out) == (1, "") and err.startswith(listing(app) + "\n%s\n" % cmd)
    assert option_names(err, cmd) == GLOBAL + OPTIONS[(app, cmd)] + GPU
    for name in OPTIONS[(app, cmd)]:
        if name in SHORT:
            assert "  -%s [ --%s ]" % (SHORT[name], name) in err, name
    assert "goss" not in err
    # the same asked by its long name, beside another option
    assert run(app, cmd, "--help", "-T", "2")[2] == err


def test_electus_classify_is_elect_reads_under_another_name(goss_entries):
    theirs = goss_entries[("elect-reads", "-h")]["stderr"]
    rc, out, err = run("electus", "classify", "-h")
    assert rc == goss_entries[("elect-reads", "-h")]["status"] == 1
    assert err.split("\nclassify\n", 1)[1] == theirs.split("\nelect-reads\n", 1)[1]
    assert "--single-seq-refs" not in err and "--pool arg" in err


@pytest.mark.parametrize("app,cmd", sorted(OPTIONS))
def test_unknown_options_are_answered_as_goss_answers_them(app, cmd, goss_entries):
    theirs = goss_entries[("build-kmer-set", "--bogus")]
    assert theirs["stderr"] == "unknown option '--bogus'\n" + "use\n\tgoss build-kmer-set -h\nfor more usage information.\n"
    rc, out, err = run(app, cmd, "--bogus")
    assert (rc, out) == (theirs["status"], "") and err == "unknown option '--bogus'\n" + use(app, cmd)
    theirs = goss_entries[("build-kmer-set", "--bogus", "-h")]
    assert theirs["stderr"] == "unknown option '--bogus'\n" + goss_entries[("build-kmer-set", "-h")]["stderr"]
    rc, out, err = run(app, cmd, "--bogus", "-h")
    assert (rc, out) == (theirs["status"], "") and err == "unknown option '--bogus'\n" + run(app, cmd, "-h")[2]


# ---- mandatory options, in the reference's order ---------------------------------------------------------------------

def missing(*names):
    return "".join("repeating option %s must be given at least once.\n" % n[1:] if n.startswith("+")
                   else "mandatory option %s was not given.\n" % n for n in names)


def test_xenome_index_reports_graft_host_prefix(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    given = {"graft": ["-G", fa], "host": ["-H", fa], "prefix": ["-P", tmp_path / "idx"]}
    for absent in (["graft", "host", "prefix"], ["graft", "host"], ["graft", "prefix"], ["host", "prefix"], ["graft"], ["host"], ["prefix"]):
        args = [a for name in ("prefix", "host", "graft") if name not in absent for a in given[name]]
        rc, out, err = run("xenome", "index", *args, cwd=tmp_path)
        assert (rc, out) == (1, "") and err == missing(*absent) + use("xenome", "index"), absent
    assert sorted(os.listdir(tmp_path)) == ["g.fa"]


def test_xenome_classify_reports_prefix(tmp_path):
    rc, out, err = run("xenome", "classify", cwd=tmp_path)
    assert (rc, out) == (1, "") and err == missing("prefix") + use("xenome", "classify")
    rc, out, err = run("xenome", "classify", "--pairs", "--graft-name", "human", cwd=tmp_path)
    assert (rc, out) == (1, "") and err == missing("prefix") + use("xenome", "classify")
    # an input that cannot be read is goss's message for one, after the missing prefix
    rc, out, err = run("xenome", "classify", "-i", "missing.fq", cwd=tmp_path)
    grc, gout, gerr = run("goss", "group-reads", "-i", "missing.fq", cwd=tmp_path)
    assert rc == grc == 1 and err == gerr.replace("mandatory option graph-in", "mandatory option prefix").replace("goss group-reads", "xenome classify")
    assert "cannot open file 'missing.fq' for reading" in err


def test_electus_index_reports_ref_fasta_then_prefix(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    rc, out, err = run("electus", "index", cwd=tmp_path)
    assert (rc, out) == (1, "") and err == missing("+ref-fasta", "prefix") + use("electus", "index")
    rc, out, err = run("electus", "index", "-P", "idx", cwd=tmp_path)
    assert (rc, out) == (1, "") and err == missing("+ref-fasta") + use("electus", "index")
    rc, out, err = run("electus", "index", "--ref-fasta", fa, "--ref-fasta", fa, cwd=tmp_path)
    assert (rc, out) == (1, "") and err == missing("prefix") + use("electus", "index")
    rc, out, err = run("electus", "index", "--ref-fasta", "missing.fa", "-P", "idx", cwd=tmp_path)
    assert (rc, out) == (1, "") and "cannot open file 'missing.fa' for reading" in err and "idx" not in "".join(os.listdir(tmp_path))


def test_electus_classify_answers_as_elect_reads(tmp_path, goss_entries):
    for argv in ([], ["--match-prefix", "m"], ["--ref-index", "a", "--pool", "p"], ["-K", "0", "--ref-index", "a"], ["-K", "64", "--ref-index", "a"]):
        grc, gout, gerr = run("goss", "elect-reads", *argv, cwd=tmp_path)
        rc, out, err = run("electus", "classify", *argv, cwd=tmp_path)
        assert grc == rc == 1 and out == gout == "" and use("goss", "elect-reads") in gerr, argv
        assert err == gerr.replace(use("goss", "elect-reads"), use("electus", "classify")), argv


# ---- numbers that are none -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("app,cmd,opt,long_", [
    ("xenome", "index", "-K", "kmer-size"), ("xenome", "index", "-M", "max-memory"), ("xenome", "classify", "-M", "max-memory"),
    ("electus", "index", "-K", "kmer-size"), ("electus", "index", "-M", "max-memory"), ("electus", "classify", "-K", "kmer-size"),
    ("electus", "classify", "-M", "max-memory"), ("electus", "classify", "--ref-threshold", "ref-threshold"),
    ("xenome", "index", "-T", "num-threads"), ("electus", "index", "--hbm-budget", "hbm-budget")])
def test_a_non_number_is_reported_as_goss_reports_one(app, cmd, opt, long_, goss_entries):
    theirs = goss_entries[("elect-reads", "--kmer-size", "x")]
    assert theirs["stderr"] == "the argument ('x') for option '--kmer-size' is invalid\n" + use("goss", "elect-reads")
    rc, out, err = run(app, cmd, opt, "x")
    assert (rc, out) == (theirs["status"], "") and err == "the argument ('x') for option '--%s' is invalid\n" % long_ + use(app, cmd)
    # -M is read before -h is looked at, as in group-reads and elect-reads
    if long_ == "max-memory":
        assert run(app, cmd, opt, "x", "-h")[2] == err
        grc, gout, gerr = run("goss", "elect-reads", "-M", "x", "-h")
        assert gerr == err.replace(use(app, cmd), use("goss", "elect-reads"))


def test_max_memory_takes_a_double(tmp_path):
    for v in ("2", "0.5", "1e3"):
        rc, out, err = run("xenome", "index", "-M", v, cwd=tmp_path)
        assert rc == 1 and err == missing("graft", "host", "prefix") + use("xenome", "index"), v


# ---- the index that is not there -------------------------------------------------------------------------------------

def test_xenome_classify_names_the_both_set(tmp_path):
    (tmp_path / "r.fq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGT\n+\n" + "I" * 32 + "\n")
    rc, out, err = run("xenome", "classify", "-P", "nowhere", "-i", "r.fq", cwd=tmp_path)
    assert rc == 1 and out == "" and err.startswith("error performing classify:\n") and "'nowhere-both" in err
    grc, gout, gerr = run("goss", "group-reads", "-G", "nowhere-both", "-i", "r.fq", cwd=tmp_path)
    assert grc == 1 and err == gerr.replace("error performing group-reads:", "error performing classify:")
    assert sorted(os.listdir(tmp_path)) == ["r.fq"]


# ---- what was there before -------------------------------------------------------------------------------------------

def test_goss_help_and_translucent_help_have_not_moved(goss_entries):
    import test_relative_cpu as rel

    for args in (("help",), ()):
        rc, out, err = run("goss", *args)
        assert (rc, out, err) == (0, "", goss_entries[("help",)]["stderr"])
    summaries = {}
    for line in goss_entries[("help",)]["stderr"].split("commands implemented by this build:\n")[1].splitlines():
        summaries[line.split()[0]] = line[2:]
    assert len(summaries) == 29        # the 28 commands and help
    own = "create a new graph from an existing graph, using coverage information from a reference graph"
    want = "translucent <command> [options]\n\ncommands implemented by this build:\n"
    for name in ["help"] + rel.SIX:
        want += "  " + (summaries[name] if name in summaries else name.ljust(max(17, len(name) + 2)) + own) + "\n"
    for args in (("help",), ()):
        assert run("translucent", *args) == (0, "", want)
