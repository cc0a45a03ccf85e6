"""build-subgraph without a GPU: the order-free model of subgraph_model.py pinned to the reference's own loop restated
as it stands, and the command's registration and option errors."""
import os
import random
import subprocess
from bisect import bisect_left

import components_model as cm
import subgraph_model as sm
import tips_cases
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)
RADII = range(6)


def reference_scan(edges, K, marked, radius, linear_paths):
    """GossCmdBuildSubgraph.cc:56-128, 178-191 restated as it stands: the marks of every window and of its reverse
    complement; then `radius` times an ascending scan over `prev` whose every set edge is followed forwards and, as its
    reverse complement, backwards; fringe[k] = !interesting[k] an ASSIGNMENT while the SegmentFollower changes
    `interesting` within the pass; Graph::linearPath (Graph.tcc:19-46) with its `ee == pBegin` break and
    inDegree(n) = outDegree(rc n).  Yields (interesting, logged number) after the marks (None) and after every pass."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1
    rank = {e: i for i, e in enumerate(edges)}

    def begin_end(node):
        return bisect_left(edges, node << 2), bisect_left(edges, (node + 1) << 2)

    def out_degree(node):
        lo, hi = begin_end(node)
        return hi - lo

    def linear_path(begin):
        visited = []
        e, e_rank = begin, rank[begin]
        node = e & node_mask
        lo, hi = begin_end(node)
        while hi - lo == 1 and out_degree(tm.revcomp(node, K)) == 1:
            ee = edges[lo]
            if ee == begin:
                break
            visited.append((e, e_rank))
            e, e_rank = ee, lo
            node = e & node_mask
            lo, hi = begin_end(node)
        visited.append((e, e_rank))
        return e, visited

    def single(interesting, fringe, e):
        lo, hi = begin_end(e & node_mask)
        for k in range(lo, hi):
            fringe[k] = not interesting[k]
            k_rc = rank[tm.revcomp(edges[k], K + 1)]
            fringe[k_rc] = not interesting[k_rc]

    def segment(interesting, fringe, e):
        end, ers = linear_path(e)
        for f, r in ers:
            interesting[r] = True
            interesting[rank[tm.revcomp(f, K + 1)]] = True
        single(interesting, fringe, end)

    follow = segment if linear_paths else single
    interesting = [False] * n
    for i, m in enumerate(marked):
        if m:
            interesting[i] = True
            interesting[rank[tm.revcomp(edges[i], K + 1)]] = True
    yield list(interesting), None
    prev = list(interesting)
    for _ in range(radius):
        before = sum(interesting)
        fringe = [False] * n
        for j in range(n):
            if not prev[j]:
                continue
            e = edges[j]
            follow(interesting, fringe, e)
            follow(interesting, fringe, tm.revcomp(e, K + 1))
        interesting = [a or b for a, b in zip(interesting, fringe)]
        prev = fringe
        yield list(interesting), sum(interesting) - before


def cycle_graph(K, length, seed):
    """a cycle of `length` edges all of whose nodes have one edge in and one out, and its mirror image"""
    rng = random.Random(seed)
    s = "".join(rng.choice("ACGT") for _ in range(length))
    edges, counts = tm.graph_of([(s + s[:K], 2)], K)
    assert len(edges) == 2 * length
    return edges, counts


def sampled(n, seed, k):
    rng = random.Random(seed)
    on = set(rng.sample(range(n), k))
    return [i in on for i in range(n)]


_inputs = {}


def inputs(oracle):
    """[(name, edges, K, marked)]"""
    if not _inputs:
        got = []
        for K in (15, 30, 55):
            edges, _, _ = tips_cases.combined_graph(K)
            n = len(edges)
            got.append(("combined %d, three edges" % K, edges, K, sampled(n, K, 3)))
            got.append(("combined %d, every 29th" % K, edges, K, [i % 29 == 0 for i in range(n)]))
            got.append(("combined %d, the last edge" % K, edges, K, [i == n - 1 for i in range(n)]))
        for K in (15, 28):
            edges, _ = cycle_graph(K, 3 * K + 7, K)
            got.append(("cycle %d" % K, edges, K, [i == 5 for i in range(len(edges))]))
        for K in (15, 27):                                # K + 1 even: a path through a self-complementary edge
            p = tips_cases.Pieces(K, seed=3)
            for name, strings in (("palindrome", p.lone_palindrome(7)[0]), ("hairpin", p.hairpin(2, 5)[0])):
                edges, _ = tm.graph_of(strings, K)
                assert any(tm.revcomp(e, K + 1) == e for e in edges)
                for at in (0, len(edges) // 2):
                    got.append(("%s %d, edge %d" % (name, K, at), edges, K, [i == at for i in range(len(edges))]))
        reads = tips_cases.error_reads(**READS)
        for K in (15, 27, 31):
            edges, _, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
            part = "\n".join(reads.split("\n")[::40])
            marked = cm.marks(edges, K, part)[0]
            assert 0 < sum(marked) < len(edges) // 4
            got.append(("reads %d" % K, edges, K, marked))
        _inputs["all"] = got
    return _inputs["all"]


def test_model_agrees_with_the_reference_loop(oracle):
    grew = {False: 0, True: 0}
    for name, edges, K, marked in inputs(oracle):
        for linear in (False, True):
            steps = list(reference_scan(edges, K, marked, max(RADII), linear))
            model = list(sm.grow_steps(edges, K, marked, max(RADII), linear))
            for radius in RADII:                          # (the model after `radius` passes is sm.grow(..., radius))
                assert model[radius] == steps[radius], (name, linear, radius)
            assert sm.grow(edges, K, marked, 3, linear) == (steps[3][0], [s[1] for s in steps[1:4]]), (name, linear)
            grew[linear] += sum(1 for s in steps[1:] if s[1])
            # radius 0: the marks and their mirror image, no more
            rank = {e: i for i, e in enumerate(edges)}
            assert steps[0][0] == [marked[i] or marked[rank[tm.revcomp(e, K + 1)]] for i, e in enumerate(edges)], name
    assert grew[False] > 20 and grew[True] > 20


def test_modes_differ_and_cycles_are_whole(oracle):
    """What the inputs are there for: a cycle marked in one edge is taken whole, with its mirror image, by the first
    linear-path pass and two edges per strand and pass in node mode; on the read graphs the two modes part."""
    for K in (15, 28):
        edges, _ = cycle_graph(K, 3 * K + 7, K)
        marked = [i == 5 for i in range(len(edges))]
        assert sm.grow(edges, K, marked, 3, True) == ([True] * len(edges), [len(edges) - 2, 0, 0])
        assert sm.grow(edges, K, marked, 3, False)[1] == [4, 4, 4]
    for name, edges, K, marked in inputs(oracle):
        if name.startswith("reads"):
            a, b = sm.grow(edges, K, marked, 2, False), sm.grow(edges, K, marked, 2, True)
            assert sum(a[0]) < sum(b[0]) < len(edges), name


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def test_command_is_registered_and_checks_its_options(tmp_path):
    if not os.path.exists(GOSS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])
    out = str(tmp_path / "sub")
    rc, _, err = run_goss("build-subgraph")
    assert rc == 1 and err.startswith("mandatory option graph-in was not given.\nmandatory option graph-out was not given.\n"
                                      "use\n\tgoss build-subgraph -h\n"), err
    rc, _, err = run_goss("build-subgraph", "-G", "a", "-G", "b", "-O", out)
    assert rc == 1 and err.startswith("mandatory option graph-in must be supplied exactly once.\n"), err
    rc, _, err = run_goss("build-subgraph", "-G", "a")
    assert rc == 1 and err.startswith("mandatory option graph-out was not given.\n"), err
    rc, _, err = run_goss("build-subgraph", "-G", "a", "-O", out, "--bogus")
    assert rc == 1 and err == "unknown option '--bogus'\nuse\n\tgoss build-subgraph -h\nfor more usage information.\n"
    rc, _, err = run_goss("build-subgraph", "-G", "a", "-O", out, "--line-in", str(tmp_path / "missing.txt"))
    assert rc == 1 and "\tcannot open file '%s' for reading\n" % (tmp_path / "missing.txt") in err
    rc, _, err = run_goss("build-subgraph", "-G", "a", "-O", out, "--radius", "two")
    assert rc == 1 and "radius" in err, err
    rc, _, err = run_goss("help")
    assert "build-subgraph   generate a subgraph of an existing graph\n" in err
    rc, _, err = run_goss("build-subgraph", "-h")
    assert rc == 1 and "--radius" in err and "--linear-paths" in err and "--buffer-size" in err and "--line-in" in err
