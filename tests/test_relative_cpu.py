"""CPU-only: the model of trim-relative / merge-graph-with-reference (relative_model.py) against itself -- the reference's
block loop for every thread count against the order-free statement -- and against hand-worked cases, the corpus
(relative_cases.py) against vacuity, the declarations of include/goss_gpu_relative.h, and the surface of the
`translucent` executable, which is decided before a command object runs and needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import gossamer_amd as g
import relative_cases as rc
import relative_model as rm
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSLUCENT = os.environ.get("TRANSLUCENT_BIN") or os.path.join(ROOT, "gossamer_amd", "translucent")
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
SIX = ["build-graph", "lint-graph", "trim-graph", "trim-relative", "prune-tips", "merge-graph-with-reference"]
JS = (1, 2, 3, 4, 7)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(g.binding.LIB_PATH) and os.path.exists(TRANSLUCENT)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])


def case(name):
    return next(c for c in rc.corpus() if c.name == name)


def tr(c, rel):
    return rm.trim_relative(c.edges, c.counts, c.K, rel)


def with_tag(tag):
    return [c for c in rc.corpus() if tag in c.tags]


# ---- the two statements ----------------------------------------------------------------------------------------------

def test_the_block_loop_is_the_order_free_statement_for_every_thread_count():
    ran = 0
    for c in rc.corpus():
        n = len(c.edges)
        for rel in rc.RELS:
            e2, c2, rep, est = rm.trim_relative(c.edges, c.counts, c.K, rel)
            gone = set(c.edges) - set(e2)
            assert est == len(e2) == rep["edges_after"] == n - len(gone)
            assert rep["below"] + rep["mirror_only"] == len(gone)
            for J in JS + (n + 1, 3 * n + 5):
                zapped = rm.zapped_serial(c.edges, c.counts, c.K, rel, J)
                assert {c.edges[r] for r in zapped} == gone, (c.name, rel, J)
                ran += 1
    assert ran == 7 * 7 * len(rc.corpus()) >= 7 * 7 * 75


def test_the_survivors_stay_closed_under_reverse_complement():
    for c in rc.corpus():
        for rel in c.rels:
            e2, c2, _, _ = rm.trim_relative(c.edges, c.counts, c.K, rel)
            s = set(e2)
            assert all(tm.revcomp(e, c.K + 1) in s for e in e2) and e2 == sorted(e2) and len(c2) == len(e2), c.name


def test_an_absent_mirror_image_refuses_only_where_its_edge_is_below():
    c = case("exact-1-99")
    minor = c.counts.index(1)
    r = c.edges.index(tm.revcomp(c.edges[minor], c.K + 1))
    edges, counts = c.edges[:r] + c.edges[r + 1:], c.counts[:r] + c.counts[r + 1:]
    for fn in (lambda rel: rm.trim_relative(edges, counts, c.K, rel), lambda rel: rm.zapped_serial(edges, counts, c.K, rel, 3)):
        with pytest.raises(ValueError, match="edge %d has no reverse complement" % minor):
            fn(0.02)
        fn(0.0)                                           # (nothing is below: nothing is looked up)


# ---- hand-worked -------------------------------------------------------------------------------------------------------

def test_hand_worked_thresholds():
    below = lambda name, rel: tr(case(name), rel)[2]["below"]
    assert rm.is_below(1, 4, 0.25) is False and 4 * 0.25 == 1.0          # thresh 1.0: the comparison is strict
    assert below("exact-1-3", 0.25) == 0 and below("exact-1-3", 0.26) == 1
    assert 100 * 0.02 == 2.0
    assert below("exact-2-98", 0.02) == 0 and below("exact-1-99", 0.02) == 1
    # (c, c): rel 1.0 takes both, c < 2c; rel 0.5 takes neither, c < c is false
    assert below("equal-counts", 1.0) == 2 and below("equal-counts", 0.5) == 0
    for rel in (-1.0, 0.0):
        assert all(rm.trim_relative(c.edges, c.counts, c.K, rel)[2]["below"] == 0 for c in rc.corpus())
    for c in rc.corpus():                                 # rel > 1: every edge of every fork
        _, forks = rm.judge(c.edges, c.counts, 1.5)
        sizes = {}
        for e in c.edges:
            sizes[e >> 2] = sizes.get(e >> 2, 0) + 1
        assert rm.trim_relative(c.edges, c.counts, c.K, 1.5)[2]["below"] == sum(s for s in sizes.values() if s >= 2)
        assert forks == sum(1 for s in sizes.values() if s >= 2)


def test_hand_worked_graphs():
    # AA 10, AT 1, TT 10 at K = 1: node A holds AA and AT; AT is its own mirror image: one bit, counted once
    c = case("self-complementary-minor")
    e2, c2, rep, est = rm.trim_relative(c.edges, c.counts, 1, 0.25)
    assert (e2, c2, est) == ([tm.encode("AA"), tm.encode("TT")], [10, 10], 2)
    assert rep == {"edges_before": 3, "edges_after": 2, "forks": 1, "below": 1, "mirror_only": 0}
    # four edges near 2^32 - 2: the sum needs 34 bits; a sum that wrapped to 32 would cull all four or none
    c = case("total-over-32-bits")
    total = sum(sorted(c.counts)[-4:])
    assert total > 1 << 32 and rm.trim_relative(c.edges, c.counts, c.K, 0.25)[2]["below"] == 1
    assert not any(rm.is_below(x, total & 0xFFFFFFFF, 0.25) for x in c.counts[:4])
    # the merge: the reference's counts, the input's count as the estimate
    e, cn, rep, est = rm.merge_with_reference([1, 4, 9, 11], [5, 5, 5, 5], [0, 4, 11, 12], [7, 0, 9, 3])
    assert (e, cn, est) == ([4, 11], [0, 9], 4) and rep == {"edges_before": 4, "edges_after": 2}


# ---- the corpus is what it says ------------------------------------------------------------------------------------------

def test_corpus_meets_its_names():
    cases = rc.corpus()
    assert len({c.name for c in cases}) == len(cases) >= 75
    for c in cases:
        assert c.edges == sorted(set(c.edges)) and len(c.counts) == len(c.edges) and c.rels
        assert all(0 <= e < 1 << (2 * (c.K + 1)) for e in c.edges) and all(0 <= x <= rc.BIG for x in c.counts)
        s = set(c.edges)
        assert all(tm.revcomp(e, c.K + 1) in s for e in c.edges), c.name
    dense = with_tag("dense")
    assert len(dense) == 40 and {c.K for c in dense} == {1, 2, 3, 4, 5} and max(len(c.edges) for c in dense) == 4096
    minor_forks = sum(rm.trim_relative(c.edges, c.counts, c.K, 0.25)[2]["below"] > 0 for c in dense)
    assert minor_forks >= 20
    assert any(rm.trim_relative(c.edges, c.counts, c.K, 0.25)[2]["mirror_only"] > 0 for c in dense)
    # the groups start where the names say, and straddle the boundary
    seen = set()
    for c in with_tag("straddle"):
        off, size = int(c.name.split("-")[1]), int(c.name.split("-")[2])
        assert [e >> 2 for e in c.edges[off:off + size]] == [c.edges[off] >> 2] * size
        assert c.edges[off - 1] >> 2 != c.edges[off] >> 2 != c.edges[off + size] >> 2
        rep = rm.trim_relative(c.edges, c.counts, c.K, 0.02)[2]
        assert rep["forks"] == 1 and rep["below"] == 1 and rep["mirror_only"] == 1
        if off + size > (64 if off < 64 else 256):
            seen.add((off < 64, "crosses"))
        seen.add(off)
    assert seen >= {61, 62, 63, 253, 254, 255, (True, "crosses"), (False, "crosses")}
    c = case("first-group")
    assert c.edges[0] >> 2 == c.edges[2] >> 2 and tr(c, 0.02)[2]["below"] == 1
    c = case("last-group")
    assert c.edges[-1] >> 2 == c.edges[-3] >> 2 != c.edges[-4] >> 2 and tr(c, 0.02)[2]["below"] == 1
    assert len(c.edges) == len(case("first-group").edges)
    for n in (1, 2, 63, 64, 65, 257):
        assert len(with_tag("n%d" % n)[0].edges) == n
    assert {len(c.edges) for c in dense} >= {63, 64, 65}
    for c in with_tag("mutual"):
        below, forks = rm.judge(c.edges, c.counts, 0.25)
        a, b = sorted(below)
        assert forks == 2 and c.edges[b] == tm.revcomp(c.edges[a], c.K + 1) and c.edges[a] >> 2 != c.edges[b] >> 2
        assert tr(c, 0.25)[2]["mirror_only"] == 0
    planted = with_tag("planted")
    assert [c.K for c in planted] == list(rc.KS) and {1 if 2 * (c.K + 1) <= 62 else 2 for c in planted} == {1, 2}
    for c in planted:
        # 77 forward edges; (1, 99), (2, 70, 70, 70) and (50, 1, 50): at 0.02 the thresholds are 2.0, 4.24 and 2.02, one
        # edge each; at 0.5 they are 50, 106 and 50.5: one, four and three
        assert tr(c, 0.02)[2] == {"edges_before": 154, "edges_after": 148, "forks": 3, "below": 3, "mirror_only": 3}
        assert tr(c, 0.5)[2] == {"edges_before": 154, "edges_after": 138, "forks": 3, "below": 8, "mirror_only": 8}
    assert max(c.K for c in cases) == 62 and any(e >> 64 for e in case("planted-k62").edges)


def test_merge_corpus_meets_its_names():
    cases = rc.merge_corpus()
    tags = {t for c in cases for t in c.tags}
    assert tags >= {"ref_empty", "in_empty", "disjoint", "identical", "ref_subset", "in_subset", "interleaved", "one_edge",
                    "small_output", "zero_count"}
    assert {1 if 2 * (c.K + 1) <= 62 else 2 for c in cases} == {1, 2}
    for c in cases:
        e, cn, rep, est = rm.merge_with_reference(c.edges, c.counts, c.ref_edges, c.ref_counts)
        assert (e, cn) == rm.merge_serial(c.edges, c.counts, c.ref_edges, c.ref_counts), c.name
        assert est == len(c.edges) and rep == {"edges_before": len(c.edges), "edges_after": len(e)}
        both = set(c.edges) & set(c.ref_edges)
        assert e == sorted(both)
        if "disjoint" in c.tags or "ref_empty" in c.tags or "in_empty" in c.tags:
            assert not e and (c.edges or c.ref_edges or c.name == "both-empty")
        if "identical" in c.tags:
            assert c.edges == c.ref_edges == e and all(x != y for x, y in zip(c.counts, c.ref_counts)) and cn == c.ref_counts
        if "ref_subset" in c.tags:
            assert set(c.ref_edges) < set(c.edges) and e == c.ref_edges
        if "in_subset" in c.tags:
            assert set(c.edges) < set(c.ref_edges) and e == c.edges and cn != c.counts
        if "interleaved" in c.tags:
            assert both and set(c.edges) - both and set(c.ref_edges) - both
        if "one_edge" in c.tags:
            assert len(set(c.edges) - set(c.ref_edges)) == 1 and len(e) == len(c.edges) - 1
        if "small_output" in c.tags:
            assert est == 4096 and len(e) == 2
        if "zero_count" in c.tags:
            assert cn[0] == 0 and len(e) == len(c.edges)


# ---- the library's declarations ----------------------------------------------------------------------------------------

def test_relative_symbols_are_declared_and_exported():
    """include/goss_gpu_relative.h, included by goss_gpu.h after goss_gpu_elect.h: what it declares is what the binding
    lists and the library exports; the calls refuse NULL"""
    text = open(os.path.join(ROOT, "include", "goss_gpu_relative.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(goss_gpu_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(g.RELATIVE_SYMBOLS) == ["goss_gpu_recount_from", "goss_gpu_relative_timing", "goss_gpu_trim_relative"]
    top = open(os.path.join(ROOT, "include", "goss_gpu.h")).read()
    assert 0 < top.find('#include "goss_gpu_elect.h"') < top.find('#include "goss_gpu_relative.h"')
    assert re.search(r"uint64_t edges_before, edges_after;\s*uint64_t forks;\s*uint64_t below;\s*uint64_t mirror_only;\s*}\s*goss_gpu_relative_report;", text)
    assert re.search(r"typedef struct { uint64_t edges_before, edges_after; } goss_gpu_recount_report;", text)
    assert g.RELATIVE_REPORT_FIELDS == rm.REPORT_FIELDS and g.RECOUNT_REPORT_FIELDS == rm.RECOUNT_FIELDS
    L = g.load()
    for n in names:
        assert hasattr(L, n), n
    L.goss_gpu_trim_relative.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.goss_gpu_recount_from.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.goss_gpu_relative_timing.argtypes = [C.c_void_p, C.c_void_p]
    assert L.goss_gpu_trim_relative(None, 0.02, None) == -1
    assert L.goss_gpu_recount_from(None, None, None) == -1
    assert L.goss_gpu_relative_timing(None, None) == -1


# ---- the executable, before any device -------------------------------------------------------------------------------------

def run(*args, exe=None, cwd=None):
    p = subprocess.run([exe or TRANSLUCENT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode()


def listed(err):
    head, _, rest = err.partition("commands implemented by this build:\n")
    return head, [line.split()[0] for line in rest.split("\n\n")[0].splitlines() if line.startswith("  ")]


def sans_listing(err):
    """the text without the lines that list the executable's commands"""
    head, sep, rest = err.partition("commands implemented by this build:\n")
    lines = rest.splitlines(True)
    while lines and lines[0].startswith("  "):
        lines.pop(0)
    return head + sep + "".join(lines)


def usage(err, cmd):
    return err.endswith("use\n\ttranslucent %s -h\nfor more usage information.\n" % cmd)


def test_help_lists_the_six_commands_and_help():
    for args in ((), ("help",), ("-h",), ("--help",)):
        rcode, out, err = run(*args)
        head, names = listed(err)
        assert rcode == 0 and out == b"" and head == "translucent <command> [options]\n\n"
        assert names == ["help"] + SIX[:4] + SIX[4:] and [n for n in names if n != "help"] == SIX and len(SIX) == 6
        assert "goss" not in err
    rcode, out, err = run("--version")
    assert rcode == 0 and out.startswith(b"translucent version ") and err == ""
    # both of translucent's own commands carry the reference's one sentence
    assert run("help")[2].count("create a new graph from an existing graph, using coverage information from a reference graph") == 2


def test_commands_that_are_not_built_are_unknown():
    for cmd in ("pop-bubbles", "assemble", "trim-paths", "build-kmer-set"):
        rcode, out, err = run(cmd)
        assert rcode == 0 and out == b"" and err.startswith("unknown command '%s'\ntranslucent <command> [options]\n" % cmd)
        assert listed(err)[1] == ["help"] + SIX
    # and goss does not know translucent's
    for cmd in ("trim-relative", "merge-graph-with-reference"):
        assert run(cmd, exe=GOSS)[2].startswith("unknown command '%s'\ngoss <command> [options]\n" % cmd)


def test_trim_relative_surface(tmp_path):
    rcode, out, err = run("trim-relative", "-h")
    assert rcode == 1 and out == b"" and listed(err)[1] == ["help"] + SIX and "\ntrim-relative\n" in err
    for opt in ("-G [ --graph-in ] arg", "-O [ --graph-out ] arg", "--relative-cutoff arg", "-T [ --num-threads ] arg", "--device arg",
                "--hbm-budget arg", "-v [ --verbose ]", "-l [ --log-file ] arg"):
        assert "  " + opt in err, opt
    for opt in ("--cutoff", "--iterate", "--graph-ref", "--estimate-only", "--graphs-in"):
        assert opt not in err, opt
    rcode, _, err = run("trim-relative", "--bogus")
    assert rcode == 1 and err.startswith("unknown option '--bogus'\n") and usage(err, "trim-relative")
    rcode, _, err = run("trim-relative", "--bogus", "-h")
    assert rcode == 1 and err.startswith("unknown option '--bogus'\ntranslucent <command> [options]\n")
    rcode, _, err = run("trim-relative", "-G", "a", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-out was not given.\n") and usage(err, "trim-relative")
    rcode, _, err = run("trim-relative", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-in was not given.\n") and usage(err, "trim-relative")
    rcode, _, err = run("trim-relative", "-G", "a", "-G", "b", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-in must be supplied exactly once.\n") and usage(err, "trim-relative")
    rcode, _, err = run("trim-relative", "-G", "a", "-O", "no-such-dir/o", cwd=tmp_path)
    assert rcode == 1 and "cannot create filenames with prefix 'no-such-dir/o'" in err
    for bad in ("x", "1e999", "nan", "inf", "-inf", "0.02x", "", " 0.5", "-1e999"):
        rcode, _, err = run("trim-relative", "-G", "a", "-O", "o", "--relative-cutoff", bad, cwd=tmp_path)
        assert rcode == 1 and err.startswith("the argument ('%s') for option '--relative-cutoff' is invalid\n" % bad), (bad, err)
        assert usage(err, "trim-relative")
    rcode, _, err = run("trim-relative", "-G", "a", "-O", "o", "-T", "x", cwd=tmp_path)
    assert rcode == 1 and err.startswith("the argument ('x') for option '--num-threads' is invalid\n")
    # a number that is one: the command gets as far as its input, which is not there
    for ok in ("0.25", "-1", "1e-3", "2"):
        rcode, _, err = run("trim-relative", "-G", "a", "-O", "o", "--relative-cutoff", ok, "-T", "8", cwd=tmp_path)
        assert rcode == 1 and err.startswith("error performing trim-relative:\n") and "--relative-cutoff" not in err, err
    assert os.listdir(tmp_path) == []                     # (the create check removes its probe)


def test_merge_graph_with_reference_surface(tmp_path):
    rcode, out, err = run("merge-graph-with-reference", "-h")
    assert rcode == 1 and out == b"" and "\nmerge-graph-with-reference\n" in err
    for opt in ("-G [ --graph-in ] arg", "-O [ --graph-out ] arg", "--graph-ref arg", "--device arg", "--hbm-budget arg"):
        assert "  " + opt in err, opt
    assert "--relative-cutoff" not in err
    rcode, _, err = run("merge-graph-with-reference", "-G", "a", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-ref was not given.\n") and usage(err, "merge-graph-with-reference")
    rcode, _, err = run("merge-graph-with-reference", "-G", "a", "--graph-ref", "r", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-out was not given.\n")
    rcode, _, err = run("merge-graph-with-reference", "-G", "a", "-G", "b", "--graph-ref", "r", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("mandatory option graph-in must be supplied exactly once.\n")
    rcode, _, err = run("merge-graph-with-reference", "--graph-ref", "r", "-O", "o", "--bogus", cwd=tmp_path)
    assert rcode == 1 and err.startswith("unknown option '--bogus'\n") and usage(err, "merge-graph-with-reference")
    rcode, _, err = run("merge-graph-with-reference", "-G", "a", "--graph-ref", "r", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("error performing merge-graph-with-reference:\n")
    assert os.listdir(tmp_path) == []


def test_the_shared_commands_answer_as_goss_does(tmp_path):
    """the records are goss's own: the same refusals, under the other executable's name"""
    rcode, _, err = run("trim-graph", "-G", "a", "-O", "o", cwd=tmp_path)
    assert rcode == 1 and err.startswith("not implemented: give -C (the cutoff is not inferred by this build;") and usage(err, "trim-graph")
    rcode, _, err = run("prune-tips", "-G", "a", "-O", "o", "--relative-cutoff", "0.1", cwd=tmp_path)
    assert rcode == 1 and err.startswith("not implemented: --cutoff and --relative-cutoff") and usage(err, "prune-tips")
    for args in (("trim-graph", "-G", "a", "-O", "o"), ("prune-tips", "-G", "a", "-O", "o", "--cutoff", "3"), ("lint-graph",),
                 ("build-graph", "-O", "o"), ("trim-graph", "-h"), ("build-graph", "--bogus")):
        ours, theirs = run(*args, cwd=tmp_path), run(*args, exe=GOSS, cwd=tmp_path)
        assert ours[:2] == theirs[:2]
        assert sans_listing(ours[2]) == sans_listing(theirs[2]).replace("goss <command>", "translucent <command>").replace("\tgoss ", "\ttranslucent "), args
