"""trim-graph / prune-tips without a GPU: the pure-Python model (tips_model.py) on hand-made graphs whose answer
follows by construction (tips_cases.py), and the two commands' usage errors."""
import os
import subprocess

import pytest

import tips_cases
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.path.join(ROOT, "gossamer_amd", "goss")
KS = (15, 27, 30, 31, 55)
USE = "use\n\tgoss %s -h\nfor more usage information.\n"


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def check_symmetric(edges, counts, K):
    at = dict(zip(edges, counts))
    assert edges == sorted(at) and len(at) == len(edges)
    for e, c in at.items():
        assert at.get(tm.revcomp(e, K + 1)) == c


def check_piece(strings, expect, K):
    edges, counts = tm.graph_of(strings, K)
    check_symmetric(edges, counts, K)
    e2, c2, rep = tm.prune_once(edges, counts, K)
    for f in tips_cases.FIELDS:
        assert rep[f] == expect.get(f, 0), (f, rep, expect)
    assert rep["edges_before"] == len(edges) and rep["edges_after"] == len(e2) == len(edges) - expect.get("removed", 0)
    assert rep["joined_at_begin"] + rep["joined_at_end"] == rep["tips"]
    assert rep["candidates"] == sum(rep[f] for f in ("tips", "too_long", "both_joined", "isolated", "outweighed"))
    check_symmetric(e2, c2, K)
    return edges, counts, e2, c2, rep


def test_revcomp_and_trim():
    assert tm.revcomp(tm.encode("AACG"), 4) == tm.encode("CGTT")
    assert tm.revcomp(tm.encode("ACGT"), 4) == tm.encode("ACGT")
    assert tm.trim([1, 5, 9, 12], [1, 2, 3, 2], 2) == ([9], [3])
    assert tm.trim([1, 5], [1, 2], 0) == ([1, 5], [1, 2])


@pytest.mark.parametrize("K", KS)
def test_source_fork_loses_its_weaker_branch(K):
    strings, expect = tips_cases.Pieces(K).fork(3, 5)
    assert (expect["joined_at_begin"], expect["joined_at_end"], expect["outweighed"]) == (1, 1, 2)
    _, _, e2, c2, _ = check_piece(strings, expect, K)
    assert set(c2) == {5} and len(e2) == 2 * (K + 3)              # the stronger branch, both strands
    # what is left is a lone path of K + 3 <= 2K edges: two candidates, joined nowhere, nothing removed
    e3, c3, rep = tm.prune_once(e2, c2, K)
    assert (rep["candidates"], rep["isolated"], rep["tips"]) == (2, 2, 0) and (e3, c3) == (e2, c2)


@pytest.mark.parametrize("K", KS)
def test_even_fork_goes_entirely(K):
    strings, expect = tips_cases.Pieces(K).fork(4, 4)
    assert expect["tips"] == 4 and expect["outweighed"] == 0
    _, _, e2, c2, rep = check_piece(strings, expect, K)
    assert e2 == [] and c2 == [] and rep["edges_after"] == 0
    assert tm.prune_once([], [], K)[2]["candidates"] == 0


@pytest.mark.parametrize("K", KS)
def test_spur_length_and_weight(K):
    p = tips_cases.Pieces(K)
    # 2K edges: cut, and the path it hung on is whole afterwards
    strings, expect = p.spur(2 * K, 2, 5)
    assert expect["tips"] == 1
    _, _, e2, c2, _ = check_piece(strings, expect, K)
    assert set(c2) == {5} and len(e2) == 2 * (4 * K + 11)
    assert tm.prune_once(e2, c2, K)[2]["too_long"] == 2
    # 2K + 1 edges: too long
    strings, expect = p.spur(2 * K + 1, 2, 5)
    assert expect["too_long"] == 3 and "tips" not in expect
    check_piece(strings, expect, K)
    # stronger than the path it leaves: stays
    strings, expect = p.spur(K, 9, 5)
    assert expect.get("outweighed") == 1
    check_piece(strings, expect, K)
    # as strong as the path: a tie cuts
    strings, expect = p.spur(3, 5, 5)
    assert expect["tips"] == 1
    check_piece(strings, expect, K)


@pytest.mark.parametrize("K", KS)
def test_joined_at_both_ends_or_nowhere_stays(K):
    p = tips_cases.Pieces(K)
    for strings, expect in (p.source_bubble(6), p.isolated(4)):
        edges, counts, e2, c2, _ = check_piece(strings, expect, K)
        assert (e2, c2) == (edges, counts)


@pytest.mark.parametrize("K", [k for k in KS if k % 2 == 1])
def test_self_complementary_edges(K):
    p = tips_cases.Pieces(K)
    for strings, expect in (p.lone_palindrome(7), p.hairpin(2, 5)):
        edges, counts, e2, c2, _ = check_piece(strings, expect, K)
        assert any(tm.revcomp(e, K + 1) == e for e in edges)
        assert (e2, c2) == (edges, counts)


@pytest.mark.parametrize("K", KS)
def test_combined_graph_covers_every_class(K):
    strings, expect = tips_cases.combined(K)
    check_piece(strings, expect, K)
    for f in ("joined_at_begin", "joined_at_end", "too_long", "both_joined", "isolated", "outweighed"):
        assert expect[f] > 0
    edges, counts, _ = tips_cases.combined_graph(K)
    steps = tm.prune(edges, counts, K, 3)
    assert steps[0][2]["tips"] == 3 and steps[1][2]["tips"] == 0 and steps[2][0] == steps[1][0]


def test_missing_reverse_complement_is_an_error():
    edges, counts, _ = tips_cases.combined_graph(15)
    beg = next(e for e in edges if tm.revcomp(e, 16) != e)
    i = edges.index(tm.revcomp(beg, 16))
    with pytest.raises(ValueError, match="edge %d has no reverse complement" % edges.index(beg)):
        tm.prune(edges[:i] + edges[i + 1:], counts[:i] + counts[i + 1:], 15, 1)


def test_cli_usage_errors(tmp_path):
    """GossCmdTrimGraph.cc:130-172, GossCmdPruneTips.cc:347-373; the options this build refuses say why."""
    out = str(tmp_path / "x")
    for cmd, extra in (("trim-graph", ["-C", "1"]), ("prune-tips", [])):
        rc, _, err = run_goss(cmd, "-O", out, *extra)
        assert rc == 1 and err == "mandatory option graph-in was not given.\n" + USE % cmd
        rc, _, err = run_goss(cmd, "-G", "a", *extra)
        assert rc == 1 and err == "mandatory option graph-out was not given.\n" + USE % cmd
        rc, _, err = run_goss(cmd, "-G", "a", "-G", "b", "-O", out, *extra)
        assert rc == 1 and err == "mandatory option graph-in must be supplied exactly once.\n" + USE % cmd
        rc, _, err = run_goss(cmd, "-G", "a", "-O", "/nonexistent-dir/x", *extra)
        assert rc == 1 and "\tcannot create filenames with prefix '/nonexistent-dir/x'\n" in err
        rc, _, err = run_goss(cmd, "-h")
        assert rc == 1 and "--graph-in" in err and "--cutoff" in err
    rc, _, err = run_goss("help")
    assert "trim-graph" in err and "prune-tips" in err
    # trim-graph: the reference's two texts (printed without a line end, App.cc:382-389), then what is not built
    rc, _, err = run_goss("trim-graph", "-G", "a", "-O", out, "-C", "2", "--estimate-only")
    assert rc == 1 and err == "cannot estimate cutoff unless it is also being inferred" + USE % "trim-graph"
    rc, _, err = run_goss("trim-graph", "-G", "a", "-O", out, "--scale-cutoff-by-k", "21")
    assert rc == 1 and err == "cannot scale an inferred cutoff" + USE % "trim-graph"
    for extra in ([], ["--estimate-only"], ["-C", "3", "--scale-cutoff-by-k", "21"]):
        rc, _, err = run_goss("trim-graph", "-G", "a", "-O", out, *extra)
        assert rc == 1 and err.startswith("not implemented: give -C") and err.endswith(USE % "trim-graph")
    # prune-tips: neither cutoff is offered
    for extra in (["--cutoff", "3"], ["--relative-cutoff", "0.1"], ["--cutoff", "3", "--relative-cutoff", "0.1"]):
        rc, _, err = run_goss("prune-tips", "-G", "a", "-O", out, *extra)
        assert rc == 1 and err.startswith("not implemented: --cutoff and --relative-cutoff") and err.endswith(USE % "prune-tips")
    rc, _, err = run_goss("prune-tips", "-G", "a", "-O", out, "--iterate", "x")
    assert rc == 1 and "the argument ('x') for option '--iterate' is invalid" in err
    # accepted and ignored: -T; the command then fails on the missing input, not on its options
    rc, _, err = run_goss("prune-tips", "-G", str(tmp_path / "none"), "-O", out, "-T", "8", "--iterate", "2")
    assert rc == 1 and err.startswith("error performing prune-tips:\n") and "none.header" in err


def test_cli_refuses_asymmetric_graphs(tmp_path, oracle):
    edges, counts, _ = tips_cases.combined_graph(15)
    files = oracle.write_graph(edges, counts, 15, out="gr")
    hdr = bytearray(files["gr.header"])
    hdr[16] |= 1                                       # Graph::Header::flags, bit 0 = asymmetric
    files["gr.header"] = bytes(hdr)
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    for cmd, extra in (("trim-graph", ["-C", "1"]), ("prune-tips", [])):
        rc, _, err = run_goss(cmd, "-G", str(tmp_path / "gr"), "-O", str(tmp_path / "out"), *extra)
        assert rc == 1
        assert err == "error performing %s:\n\tunable to open graph '%s'\nAsymmetric graphs not yet handled" % (cmd, tmp_path / "gr")
