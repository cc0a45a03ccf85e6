#!/usr/bin/env python3
"""Regenerates tests/golden/cli_surface.json: what the `goss` command line answers before any command object runs.

Every entry is one invocation, run in a fresh empty directory with relative names only (so no temporary path enters a
message), after the files it names have been created there.  Recorded per entry: the argv, the exit status, stdout,
stderr and the sorted listing of the directory afterwards (the option checks have side effects: `-O o` probes and removes
`o.test`, `-o out.txt` leaves an empty `out.txt`).

Every entry must be decided inside the front end: a command that starts would answer differently on a machine with a
GPU.  The generator refuses to write an entry that

* says `error performing` on stderr (a command object ran), except for dump-bases and print-contigs' supergraph refusal;
* has a logger line (`<asctime>\\t<severity>\\t...`) on stderr;
* ends with status 0, except `help`, no arguments, an unknown command, `--version`, dump-bases and synth-reads.

tests/test_cli_surface.py replays the entries against the built `goss` (or GOSS_BIN).

Run from the repo root:  python tests/golden/make_cli_surface.py
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "cli_surface.json")

READS = "ACGTACGTACGTACGTACGTACGTACGTACGT\n"
TWO_FQ = "@a\nACGTA\n+\nIIIII\n@b\nTTTTT\n+\nIIIII\n"

# the 28 commands of the help list; what each one's table holds decides its entries below
BUILD = ["build-graph", "build-kmer-set"]
FAMILY = ["dump-graph", "dump-kmer-set", "lint-graph", "restore-graph", "intersect-kmer-sets", "merge-and-annotate-kmer-sets",
          "compute-near-kmers", "merge-graphs", "merge-kmer-sets", "subtract-kmer-set", "graph-to-kmer-set", "trim-graph",
          "prune-tips", "trim-paths", "clip-links", "print-contigs", "build-entry-edge-set"]
READERS = ["count-components", "build-subgraph", "extract-reads", "filter-reads", "group-reads", "pool-samples",
           "annotate-kmers", "classify-reads", "elect-reads"]
COMMANDS = BUILD + FAMILY + READERS
NO_G = BUILD + ["pool-samples", "elect-reads"]              # their tables have no graph-in

# numeric options beyond --num-threads / --device / --hbm-budget, which every table has (parseArgs validates them all,
# also where the command then ignores them)
NUMERIC = {
    "build-graph": ["--kmer-size", "--buffer-size"],
    "build-kmer-set": ["--kmer-size", "--buffer-size", "--log-hash-slots"],
    "trim-graph": ["--cutoff", "--scale-cutoff-by-k", "--iterate"],
    "prune-tips": ["--cutoff", "--scale-cutoff-by-k", "--iterate"],
    "trim-paths": ["--cutoff"],
    "print-contigs": ["--min-length", "--min-coverage"],
    "build-subgraph": ["--buffer-size", "--radius"],
    "pool-samples": ["--kmer-size", "--buffer-size"],
    "classify-reads": ["--buffer-size"],
    "elect-reads": ["--kmer-size", "--ref-threshold"],
}
for _c in FAMILY:
    NUMERIC.setdefault(_c, []).insert(0, "--max-merge")

# -G a -G b "plus whatever else it needs" to reach the check and to fail there (never all options valid)
TWICE_EXTRA = {
    "merge-and-annotate-kmer-sets": ["-G", "c", "-O", "o"],       # three: "exactly twice"
    "graph-to-kmer-set": ["-O", "o"], "trim-graph": ["-O", "o", "-C", "2"], "prune-tips": ["-O", "o"],
    "trim-paths": ["-O", "o", "-C", "2"], "clip-links": ["-O", "o"], "build-subgraph": ["-O", "o"],
    "annotate-kmers": ["--annotation-list", "l", "--phylogeny", "p"],
}


def invocations():
    """[(argv, files)]: files maps a relative name to the text to put there beforehand."""
    inv = []

    def add(*argv, **files):
        inv.append(([str(a) for a in argv], {k.replace("__", "."): v for k, v in files.items()}))

    # ---- every command: help, nothing, unknown options, -G twice, every numeric option with a non-number ----
    for c in COMMANDS:
        add(c, "-h")
        add(c)
        add(c, "--bogus")
        add(c, "--bogus", "-h")
        if c not in NO_G:
            add(c, "-G", "a", "-G", "b", *TWICE_EXTRA.get(c, []))
        for opt in ["--num-threads", "--device", "--hbm-budget"] + NUMERIC.get(c, []):
            add(c, opt, "x")

    # ---- the build commands ----
    for c in BUILD:
        add(c, "-O", "o")                                         # no -k; and no o.test afterwards
        add(c, "-k", "25")                                        # no -O
        add(c, "-k", "64")
        add(c, "-k", "63")
        add(c, "-k", "25", "--line-in", "r.txt", r__txt=READS)    # --line-in is accepted
        add(c, "-k", "25", "-O", "o", "--line-in", "missing.txt")
        add(c, "-k", "25", "-O", "o", "-i", "missing.fq", "-I", "missing.fa")
        add(c, "-k", "25", "-O", "o", "--line-in", "r.txt", "--devices", "0,,1", r__txt=READS)
        add(c, "-k", "25", "-O", "o", "--line-in", "r.txt", "--devices", "0,x", r__txt=READS)
        add(c, "-k", "25", "-O", "o", "--line-in", "r.txt", "--tmp-dir", "nowhere", r__txt=READS)
        add(c, "-k", "25", "-O", "o", "--line-in", "r.txt", "--tmp-dir", "file", r__txt=READS, file="x")
        add(c, "-O", "/nonexistent-dir/x")                        # together with a missing -k
        add(c, "-k", "25", "-O", "/nonexistent-dir/x")
        add(c, "--kmer", "25")                                    # a unique prefix
        add(c, "--log-file", "log.txt", "--debug", "foo")         # the warning goes to the file
        add(c, "--log-file", "/nonexistent-dir/log", "-k", "25")
        add(c, "-k")                                              # the argument is missing
        add(c, "-k", "-1")
        add(c, "-vh")                                             # a grouped flag
        add(c, "-k", "25", "--fastqs-in", "nolist")               # the list is read by the checks
    add("build-graph", "-S", "20")                                # -S is build-kmer-set's

    # ---- the file family ----
    for c in ("merge-kmer-sets", "merge-graphs"):
        add(c, "-O", "o")                                         # no inputs
        add(c, "-G", "a")
        add(c, "--graphs-in", "list", list="a")                   # the last line lacks '\n': no inputs
        add(c, "--graphs-in", "list", list="a\nb")
        add(c, "--graphs-in", "list", "-O", "o", list="a")
        add(c, "-G", "a", "-G", "b", "-O", "o", "--tmp-dir", "nowhere")
        add(c, "-G", "a", "-G", "b", "-O", "o", "--tmp-dir", "file", file="x")
        add(c, "-G", "a", "-O", "/nonexistent-dir/x", "--tmp-dir", "nowhere")
        add(c, "--log-file", "log.txt", "--debug", "foo")         # no warning here
    add("merge-graphs", "--graph", "a")                           # an ambiguous prefix
    add("merge-graphs", "--graph-o", "o")                         # a unique one
    add("intersect-kmer-sets", "-G", "a")
    add("intersect-kmer-sets", "-O", "/nonexistent-dir/x")
    add("subtract-kmer-set", "-G", "a", "-O", "o")                # one input: the message has no final newline
    add("subtract-kmer-set", "-G", "a", "-G", "b", "-G", "c", "-O", "o")
    add("subtract-kmer-set", "-G", "a", "-G", "b", "-G", "c")
    add("subtract-kmer-set", "--graphs-in", "list", list="a\nb\nc")
    add("merge-and-annotate-kmer-sets", "-G", "a", "-O", "o")
    add("merge-and-annotate-kmer-sets", "-G", "a", "-G", "b")
    add("merge-and-annotate-kmer-sets", "-O", "o")
    add("graph-to-kmer-set", "-G", "a")
    add("graph-to-kmer-set", "-O", "o")
    add("graph-to-kmer-set", "-O", "/nonexistent-dir/x")          # not probed: only its presence is asked for
    for c in ("dump-kmer-set", "dump-graph"):
        add(c, "-o", "out.txt")                                   # leaves an empty out.txt although -G is missing
        add(c, "-o", "-")
        add(c, "-G", "a", "-o", "/nonexistent-dir/x")
        add(c, "-G", "a", "-G", "b", "-o", "out.txt")
        add(c, "--graph-in=a", "-Gb")                             # both spellings counted
    add("restore-graph", "-O", "/nonexistent-dir/x")
    add("restore-graph", "-f", "in.txt")
    add("lint-graph", "--dump-properties")
    add("lint-graph", "--graph-in=a", "--bogus")
    add("trim-graph", "-G", "a")
    add("trim-graph", "-O", "o", "-C", "2")
    add("trim-graph", "-G", "a", "-O", "o")                       # no -C: not implemented
    add("trim-graph", "-Ga", "-Oo")
    add("trim-graph", "-G", "a", "-O", "o", "-C", "2", "--estimate-only")
    add("trim-graph", "-C", "2", "--estimate-only", "-h")         # thrown inside the checks: wins over help
    add("trim-graph", "-G", "a", "-O", "o", "--scale-cutoff-by-k", "21")
    add("trim-graph", "-G", "a", "-O", "o", "-C", "2", "--scale-cutoff-by-k", "21")
    add("trim-graph", "-G", "a", "-O", "o", "--estimate-only")
    add("trim-graph", "-G", "a", "-O", "o", "--tmp-dir", "nowhere")           # honours --tmp-dir: "not implemented" wins
    add("trim-graph", "-G", "a", "--tmp-dir", "nowhere")
    add("prune-tips", "-G", "a")
    add("prune-tips", "-O", "o")
    add("prune-tips", "-G", "a", "-O", "o", "--cutoff", "3")
    add("prune-tips", "-G", "a", "-O", "o", "--relative-cutoff", "0.5")
    add("prune-tips", "-G", "a", "--cutoff", "3")                 # the checker's errors come first
    add("trim-paths", "-G", "a", "-O", "o")                       # no -C
    add("trim-paths", "-G", "a", "-C", "1")
    add("trim-paths", "-O", "o", "-C", "1")
    add("trim-paths", "-G", "a", "-O", "o", "-C", "4294967296")
    add("trim-paths", "-G", "a", "-C", "4294967296")
    add("trim-paths", "-G", "a", "-O", "o", "-C", "4294967296", "--tmp-dir", "nowhere")
    add("clip-links", "-G", "a")
    add("clip-links", "-O", "o")
    add("clip-links", "-O", "o", "-C", "1")                       # -C is trim-paths'
    add("print-contigs", "-G", "a", "--print-entailed-contigs")
    add("print-contigs", "-G", "a", "--include-entailed-contigs")
    add("print-contigs", "--print-entailed-contigs")
    add("print-contigs", "-G", "a", **{"a-supergraph__header": "x"})
    add("print-contigs", "-G", "a", "--tmp-dir", "nowhere", **{"a-supergraph__header": "x"})
    add("print-contigs", "-G", "a", "--print-entailed-contigs", **{"a-supergraph__header": "x"})
    add("print-contigs", "-o", "out.txt")
    add("print-contigs", "-G", "a", "-o", "/nonexistent-dir/x")
    add("build-entry-edge-set", "-O", "o")
    add("compute-near-kmers", "-O", "o")

    # ---- the commands that read reads ----
    add("pool-samples", "--line-in", "r.txt", r__txt=READS)       # refused here, accepted by the build commands
    add("pool-samples", "-k", "64", "-O", "o")
    add("pool-samples", "-k", "64")
    add("pool-samples", "-O", "o", "-I", "missing.fa", "-i", "missing.fq")
    add("pool-samples", "-O", "/nonexistent-dir/x")
    add("pool-samples", "--kmer-sets-in", "list", list="a\nb")
    add("pool-samples", "-O", "o", "--fastas-in", "list", "-I", "missing.fa", list="r.fa")
    add("count-components", "-I", "missing.fa")                   # unreadable input together with a missing -G
    add("count-components", "-O", "/nonexistent-dir/x")           # graph-out is optional and not probed
    add("count-components", "-G", "a", "--line-in", "missing.txt")
    add("count-components", "--tmp-dir", "nowhere")
    add("build-subgraph", "-G", "a")
    add("build-subgraph", "-O", "o")
    add("build-subgraph", "-I", "missing.fa")
    add("build-subgraph", "-G", "a", "-O", "o", "-i", "missing.fq")
    add("build-subgraph", "-G", "a", "-O", "/nonexistent-dir/x")
    add("extract-reads", "-o", "out.txt")                         # leaves an empty out.txt although -G is missing
    add("extract-reads", "-G", "a", "-G", "b", "-o", "out.txt")
    add("extract-reads", "-G", "a", "-o", "/nonexistent-dir/x")
    add("extract-reads", "--tmp-dir", "nowhere")                  # ignores --tmp-dir: nothing about the directory is said
    add("extract-reads", "-G", "a", "-I", "missing.fa", "--tmp-dir", "nowhere")
    add("extract-reads", "-I", "missing.fa")
    add("extract-reads", "--match-file", "m")                     # filter-reads'
    add("filter-reads", "-o", "out.txt")                          # extract-reads'
    add("filter-reads", "--match-file", "m", "--non-match-file", "n", "--pairs", "--count")
    add("filter-reads", "-G", "a", "-i", "missing.fq")
    add("filter-reads", "--tmp-dir", "nowhere")
    for c in ("group-reads", "elect-reads"):
        add(c, "-M", "bad")
        add(c, "-M", "bad", "-h")                                 # the usage error wins over help
        add(c, "-M", "")
        add(c, "-M", "1.5")
        add(c, "-M", "1e3x")
    add("group-reads", "-G", "a", "-M", "bad")
    add("group-reads", "-G", "a", "--line-in", "missing.txt")
    add("group-reads", "--pairs", "--lhs-name", "l", "--rhs-name", "r", "--output-filename-prefix", "p", "--dont-write-reads",
        "--preserve-read-order")
    add("group-reads", "--tmp-dir", "nowhere")
    add("elect-reads", "--pool", "p", "--ref-fasta", "r.fa", r__fa=">r\n" + READS)
    add("elect-reads", "--pool", "p", "--ref-index", "x")
    add("elect-reads", *(["--ref-index", "x"] * 65))
    add("elect-reads", *(["--ref-index", "x"] * 65), "--pool", "p")
    add("elect-reads", "-K", "0")
    add("elect-reads", "-K", "0", "--pool", "p")
    add("elect-reads", "-K", "64", "--pool", "p")
    add("elect-reads", "-k", "25")                                # the short name is -K
    add("elect-reads", "--ref-fasta", "missing.fa")
    add("elect-reads", "--ref-fasta", "missing.fa", "--tmp-dir", "nowhere")
    add("elect-reads", "--pool", "p", "-i", "missing.fq")
    add("elect-reads", "-G", "a")                                 # no graph-in here
    add("annotate-kmers", "-G", "a")
    add("annotate-kmers", "-G", "a", "--annotation-list", "l")
    add("annotate-kmers", "-G", "a", "--phylogeny", "p")
    add("annotate-kmers", "--annotation-list", "l", "--phylogeny", "p")
    add("annotate-kmers", "-I", "r.fa")                           # classify-reads'
    add("classify-reads", "-I", "missing.fa")
    add("classify-reads", "-G", "a", "--line-in", "missing.txt", "--pairs")
    add("classify-reads", "--phylogeny", "p")                     # annotate-kmers'
    add("classify-reads", "--tmp-dir", "nowhere")

    # ---- the rest ----
    add()
    add("help")
    add("-h")
    add("--help")
    add("-h", "build-graph")
    add("frobnicate")
    add("frobnicate", "-h")
    add("-x")
    add("--version")
    add("build-graph", "-k", "25", "--version")
    add("help", "--version")
    add("synth-reads")
    add("synth-reads", "1", "2")
    add("synth-reads", "x", "10", "100", "1", "out.fq")
    add("synth-reads", "2", "10", "100", "x", "out.fq")
    add("synth-reads", "2", "10", "100", "1", "/nonexistent-dir/out.fq")
    add("synth-reads", "2", "10", "100", "1", "out.fq")
    add("dump-bases", "-h")
    add("dump-bases")
    add("dump-bases", "--bogus")
    add("dump-bases", "--device", "0")                            # its table has no device options
    add("dump-bases", "-T", "x")
    add("dump-bases", "-i", "missing.fq")
    add("dump-bases", "-i", "two.fq", two__fq=TWO_FQ)
    add("dump-bases", "-T", "4", "-i", "two.fq", two__fq=TWO_FQ)
    add("dump-bases", "-f", "list", two__fq=TWO_FQ, list="two.fq\ntwo.fq")
    return inv


def run_entry(goss, argv, files):
    """One invocation in a fresh directory: (status, stdout, stderr, sorted listing afterwards)."""
    with tempfile.TemporaryDirectory() as d:
        for name, text in files.items():
            with open(os.path.join(d, name), "w", newline="") as f:
                f.write(text)
        p = subprocess.run([goss] + argv, cwd=d, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        return p.returncode, p.stdout.decode(), p.stderr.decode(), sorted(os.listdir(d))


LOGGER_LINE = re.compile(r"^(Mon|Tue|Wed|Thu|Fri|Sat|Sun) (Jan|Feb|Mar|Apr|May|Jun|Jul|Aug|Sep|Oct|Nov|Dec) [ 0-9]\d \d\d:\d\d:\d\d \d{4}\t", re.M)


def refuse(argv, status, stderr, files):
    """Why this entry may not be recorded (a command object ran, or would answer differently elsewhere), or None."""
    cmd = argv[0] if argv else ""
    supergraph = cmd == "print-contigs" and any(n.endswith("-supergraph.header") for n in files)
    if "error performing" in stderr and cmd != "dump-bases" and not supergraph:
        return "a command object ran"
    if LOGGER_LINE.search(stderr):
        return "a logger line on stderr"
    if status == 0 and not (cmd in ("", "help", "dump-bases", "synth-reads") or cmd not in COMMANDS or "--version" in argv):
        return "status 0"
    return None


# The file holds one entry per line, [argv, files, status, stdout, stderr, listing], and three texts that recur in stderr
# are written once: {{commands}} is the list of commands (what `goss help` prints), {{help}} is everything the entry's
# command prints for -h, {{use}} is the "use goss <command> -h" trailer of a usage error.
def _use(argv):
    return "use\n\tgoss %s -h\nfor more usage information.\n" % (argv[0] if argv else "help")


def write(entries):
    commands = next(e["stderr"] for e in entries if e["argv"] == ["help"])
    helps = {e["argv"][0]: e["stderr"] for e in entries if len(e["argv"]) == 2 and e["argv"][1] == "-h" and e["argv"][0] in COMMANDS}
    assert not any("{{" in e["stderr"] for e in entries)
    lines = []
    for e in entries:
        argv, err = e["argv"], e["stderr"]
        if argv and argv[0] in helps and argv[1:] != ["-h"]:
            err = err.replace(helps[argv[0]], "{{help}}")
        if argv != ["help"]:
            err = err.replace(commands, "{{commands}}")
        err = err.replace(_use(argv), "{{use}}")
        lines.append(json.dumps([argv, e["files"], e["status"], e["stdout"], err, e["listing"]]))
    with open(JSON, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")
    assert load() == entries


def load():
    """The recorded entries as dicts, the shared texts put back."""
    with open(JSON) as f:
        rows = json.load(f)
    commands = next(r[4] for r in rows if r[0] == ["help"])
    helps = {r[0][0]: r[4].replace("{{commands}}", commands) for r in rows if r[0][1:] == ["-h"]}
    entries = []
    for argv, files, status, out, err, listing in rows:
        err = err.replace("{{use}}", _use(argv)).replace("{{help}}", helps.get(argv[0] if argv else "", "")).replace("{{commands}}", commands)
        entries.append({"argv": argv, "files": files, "status": status, "stdout": out, "stderr": err, "listing": listing})
    return entries


def main():
    goss = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
    entries = []
    for argv, files in invocations():
        status, out, err, listing = run_entry(goss, argv, files)
        why = refuse(argv, status, err, files)
        if why:
            sys.exit("refused (%s): goss %s\n%s" % (why, " ".join(argv), err))
        entries.append({"argv": argv, "files": files, "status": status, "stdout": out, "stderr": err, "listing": listing})
    write(entries)
    per = {}
    for e in entries:
        c = e["argv"][0] if e["argv"] else ""
        per[c] = per.get(c, 0) + 1
    print("wrote", len(entries), "entries;", ", ".join("%s %d" % (c, per[c]) for c in COMMANDS))


if __name__ == "__main__":
    main()
