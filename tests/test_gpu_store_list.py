"""The store list of the narrow first level (kernels_extract.hpp: extract1_part_kernel<.., NARROW>, phases C and D;
role: BackyardHash.cc:115-242 insert).  The thread that owns a bucket lists the bucket's whole granules -- where each
goes in the output and where it lies in LDS -- and the store loop walks that list, not the layout with its carried
granules in between.  The list's positions come out of the same scan as the layout's (a packed word).  Files against
the oracle and against the 8-byte form (GOSS_GPU_NARROW=0), whose store loop is not the list's."""
import os
import random

import pytest

import gossamer_amd as g

pytestmark = pytest.mark.gpu


class env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


STATS = ("fused_chunks", "rem32_chunks", "narrow_chunks", "segment_retries", "fused_overflows")


def build(reads, k, mode, budget=8 << 30):
    with g.Context(k, mode, hbm_budget=budget) as ctx:
        ctx.push_host(reads)
        c = ctx.finish()
        files = ctx.emit()
        st = {n: ctx.stat(n) for n in STATS}
    return c, files, st


_expected = {}


def expected(oracle, name, reads, k, mode):
    """The oracle's files and window count of (reads, k, mode): computed once, shared, never changed."""
    key = (name, k, mode)
    if key not in _expected:
        exp, nwin = (oracle.build_graph if mode else oracle.build_kmer_set)([(oracle.LINE, "reads", reads)], k, out="o")
        _expected[key] = ({n[1:]: d for n, d in exp.items()}, nwin)
    return _expected[key]


def check(oracle, name, reads, k, mode, envs=({},), path=True, tried=True, budget=8 << 30):
    """`reads` built under every environment of `envs` and once in the 8-byte form: the oracle's files every time; with
    `path`, the fused narrow form took the one chunk; without (a region may overflow and the chunk be redone) but with
    `tried`, the narrow first level ran at least: it counted the chunk or overflowed a region."""
    exp, nwin = expected(oracle, name, reads, k, mode)
    for e in envs:
        with env(**e):
            c, got, st = build(reads, k, mode, budget)
        print(name, k, mode, e, st)
        assert c.windows == nwin, (e, st)
        if path:
            assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1 and st["narrow_chunks"] == 1, (e, st)
        elif tried:
            assert st["narrow_chunks"] + st["fused_overflows"] >= 1, (e, st)
        assert got == exp, (e, st)
    with env(**dict(envs[0], GOSS_GPU_NARROW=0)):
        c, got, st = build(reads, k, mode, budget)
    assert c.windows == nwin and st["narrow_chunks"] == 0, st
    if path:
        assert st["fused_chunks"] == 1 and st["rem32_chunks"] == 1, st
    assert got == exp


def reads_45m(k, mode, canon):
    return g.synth_reads_host(300_000, 150, 1_500_000, seed=700 + k + mode + canon)


def test_too_few_keys_for_the_fused_path(oracle):
    """12 reads of 150 random bases are 1 512 windows at k = 25, six keys a bucket, with GOSS_GPU_FUSED_MIN=0.  The
    library does not hand so few keys to the fused path whatever that minimum is (its sample wants 2^20 keys that repeat
    threefold: fused_path.hpp, fused_chunk_once), so here only the result is asserted; the nearest input that does take the
    narrow first level is the next test's."""
    rng = random.Random(52)
    txt = "".join("".join(rng.choice("ACGT") for _ in range(150)) + "\n" for _ in range(12)).encode()
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "tiny", txt, 25, 0, path=False, tried=False, budget=2 << 30)


def test_hardly_a_whole_granule_in_a_tile(oracle):
    """1.2 M reads of 25 bases at k = 25: one window in 26 starts is valid, a tile of 4 096 starts brings 157 keys -- less
    than one a bucket.  A bucket fills a granule of twelve once in twenty tiles: the store list holds a dozen entries
    of its 576, the loop's one round is mostly idle lanes, and most keys of a workgroup's last tiles leave through
    the final flush."""
    rng = random.Random(53)
    genome = "".join(rng.choice("ACGT") for _ in range(100_000))
    txt = "".join(genome[p:p + 25] + "\n" for p in (rng.randrange(len(genome) - 25) for _ in range(1_200_000))).encode()
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "sparse", txt, 25, 0, budget=2 << 30)


@pytest.mark.parametrize("k,mode", [(25, 0), (24, 1)])
def test_many_whole_granules_in_few_buckets(oracle, k, mode):
    """40 000 reads of 150 bp from a genome that is one 64-base motif repeated: 64 distinct windows (and their reverse
    complements), so a tile's ~3 400 keys fall into a handful of buckets -- tens of whole granules a bucket (the entry
    loop's part that is not unrolled) and list positions in the hundreds for the last buckets.  The list itself is no
    longer than any tile's of 150-bp reads, ~285 entries: one round of the store loop (the long reads below make it
    two).  A region may overflow on such keys and the chunk be redone: the result is asserted and that the narrow
    first level ran, not that its result was kept."""
    rng = random.Random(64)
    motif = "".join(rng.choice("ACGT") for _ in range(64))
    genome = motif * 40
    reads = []
    for _ in range(40_000):
        p = rng.randrange(64)
        reads.append(genome[p:p + 150])
    txt = ("\n".join(reads) + "\n").encode()
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "motif", txt, k, mode, path=False, budget=2 << 30)


@pytest.mark.parametrize("k,mode,canon", [(25, 0, 0), (24, 0, 0), (21, 0, 0), (24, 1, 0), (20, 1, 0), (25, 0, 2)])
def test_carried_granules_over_many_tiles(oracle, k, mode, canon):
    """300 000 reads of 150 bp, 45 M window starts: 11 059 tiles of 4 096 starts and more (graphs: 8 to a thread, twice
    the tiles) over at most 768 workgroups -- the persistent grid or a smaller one, so every workgroup runs fourteen
    tiles at least and carries granules from each to the next.  Every instantiation of the narrow form that reads
    bases: the squeeze form (k = 25), even and odd k, graphs, canonical forms computed at the first level; as it is and
    with the layout capped at 576 granules.  A tile of these reads has ~285 whole granules (one round of the store loop)
    and a layout of ~520 to ~540 granules, so hardly any tile passes that cap: the second scan and the second round
    are the long reads' below."""
    reads = reads_45m(k, mode, canon)
    base = {"GOSS_GPU_CANON_L1": 2} if canon else {}
    assert len(reads) // 4096 >= 14 * 768          # (tiles over the largest grid)
    check(oracle, "many%d" % canon, reads, k, mode, envs=(base, dict(base, GOSS_GPU_NARROW_CAPG=576)))


def long_reads(motif):
    """60 reads of 100 000 bases, 6 M window starts of which all but 24 in 100 001 are valid: from a random genome of
    0.5 Mbp (twelvefold coverage), or from one 64-base motif repeated."""
    if not motif:
        return g.synth_reads_host(60, 100_000, 500_000, seed=811)
    rng = random.Random(812)
    unit = "".join(rng.choice("ACGT") for _ in range(64))
    genome = unit * (100_064 // 64 + 1)
    return "".join(genome[p:p + 100_000] + "\n" for p in (rng.randrange(64) for _ in range(60))).encode()


@pytest.mark.parametrize("k,mode", [(25, 0), (24, 1)])
@pytest.mark.parametrize("motif", [0, 1])
def test_every_window_valid_takes_two_rounds(oracle, k, mode, motif):
    """Long reads: every window of a tile is valid, 4 096 keys (a graph: both strands of 2 048 windows) and with them 341
    whole granules on average -- more than the 320 one round of five chunks per lane covers, so the store loop steps on
    to a second round in nearly every tile.  1 465 tiles over the ~90 workgroups such a chunk gets, sixteen tiles each.
    motif: the same from a 64-base motif repeated -- the keys of a tile in a handful of buckets, so that long pieces (the
    entry loop that is not unrolled), large list positions and more than 320 entries occur together; a region may
    overflow on these keys and the chunk be redone, so there the result is asserted and that the narrow first level
    ran.  (The default budget of 8 GB: with as many keys as window starts the bucket regions need the slack that
    process_chunk grants only where the arena has room.)  Not with GOSS_GPU_NARROW_CAPG=576: the layout of such a tile
    is 341 + 256 x 11/12 = 576 granules on average, every other tile would send 256 short granules of eight slots for
    five or six keys, and the host's check of the slots handed out against the keys (fused_path.hpp: "bucket counts do
    not add up") allows a workgroup a few such tiles, not half of them -- the next test has them among short reads."""
    reads = long_reads(motif)
    assert len(reads) // 4096 >= 1024
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "long%d" % motif, reads, k, mode, path=not motif)


@pytest.mark.parametrize("k,mode", [(25, 0), (24, 1)])
def test_second_scan_on_long_reads_among_short_ones(oracle, k, mode):
    """100 000 reads of 150 bp with sixteen reads of 100 000 bases spread among them, as it is and with
    GOSS_GPU_NARROW_CAPG=576.  Each long read fills two dozen tiles with valid windows alone: their layouts are 576
    granules on average, so with the cap about half of them -- some two hundred tiles -- send their carried granules
    off short and are laid out again by the second packed scan, with 341 whole granules, the store loop's second
    round, behind it; the tiles of short reads before and after them (~520 granules) take the first scan's layout and
    pick up what the short granules left.  The slots those two hundred tiles waste stay within what the host's check
    of the slots handed out allows."""
    short = g.synth_reads_host(100_000, 150, 500_000, seed=821)
    longs = long_reads(0).split(b"\n")[:16]
    part = len(short) // 16 // 151 * 151
    txt = b"".join(short[i * part:(i + 1) * part] + longs[i] + b"\n" for i in range(16)) + short[16 * part:]
    assert len(txt) == len(short) + 16 * 100_001
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "mixed", txt, k, mode, envs=({}, {"GOSS_GPU_NARROW_CAPG": 576}))


@pytest.mark.parametrize("k,mode", [(25, 0), (23, 1)])
def test_invalid_windows_stay_out_of_the_list(oracle, k, mode):
    """Ragged reads of 40-150 bp, 5 % of them with an N, half in lower case (tests/test_gpu_rem32.py's small inputs): the
    windows over a non-base and over a read's end rank in the spare counters, which no bucket's thread counts."""
    rng = random.Random(321)
    genome = "".join(rng.choice("ACGT") for _ in range(30000))
    reads = []
    for _ in range(40000):
        L = rng.randint(40, 150)
        p = rng.randint(0, len(genome) - L)
        r = genome[p:p + L]
        if rng.random() < 0.05:
            q = rng.randrange(L)
            r = r[:q] + "N" + r[q + 1:]
        if rng.random() < 0.5:
            r = r.lower()
        reads.append(r)
    txt = ("\n".join(reads) + "\n").encode()
    with env(GOSS_GPU_FUSED_MIN=0):
        check(oracle, "ragged", txt, k, mode, budget=2 << 30)


def test_packed_input(oracle):
    """The 45 M window starts at k = 25 packed on the device and pushed packed: the kernel's PACKED instantiation."""
    import torch
    reads = reads_45m(25, 0, 0)
    exp, nwin = expected(oracle, "many0", reads, 25, 0)
    for e in ({}, {"GOSS_GPU_NARROW": 0}):
        with env(**e):
            with g.Context(25, 0, hbm_budget=8 << 30) as ctx:
                buf = torch.frombuffer(bytearray(reads), dtype=torch.uint8).cuda()
                groups = (len(reads) + 15) // 16
                dc = torch.empty(groups, dtype=torch.int32, device="cuda")
                db = torch.empty(groups, dtype=torch.int16, device="cuda")
                ctx.pack_bases_device(buf.data_ptr(), len(reads), dc.data_ptr(), db.data_ptr())
                del buf
                ctx.push_packed_device(dc.data_ptr(), db.data_ptr(), len(reads))
                c = ctx.finish()
                got = ctx.emit()
                st = {n: ctx.stat(n) for n in STATS + ("packed_fused_chunks",)}
        assert c.windows == nwin
        assert st["fused_chunks"] == 1 and st["packed_fused_chunks"] == 1 and st["rem32_chunks"] == 1, (e, st)
        assert st["narrow_chunks"] == (0 if e else 1), (e, st)
        assert got == exp, e
