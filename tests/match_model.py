"""A model of goss_gpu_object_match_reads and of the two commands on top of it (extract-reads, filter-reads), in plain
Python + numpy: the reads of a byte string, their valid windows, the windows' keys (optionally in canonical form),
membership in a Python set, the per-read answers, and the bytes the commands write.  Nothing here knows the library.

Reads: the stretches between '\\n' bytes; a last stretch without its '\\n' is a read, two adjacent '\\n' enclose an empty
read.  Windows: L consecutive bytes of one read, all of ACGTacgt; the key has the first base in the most significant
used bits (GossRead::Iterator, GossReadBaseString.hh:133-188)."""
import random

import numpy as np

CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
MASK64 = (1 << 64) - 1
FNV_SEED, FNV_PRIME = 14695981039346656037, 1099511628211


# ---- reads and windows ---------------------------------------------------------------------------------------------

def read_spans(data):
    """[(begin, end)] of every read: data[begin:end] are its bytes"""
    spans, at = [], 0
    while True:
        nl = data.find(b"\n", at)
        if nl < 0:
            if at < len(data):
                spans.append((at, len(data)))
            return spans
        spans.append((at, nl))
        at = nl + 1


def read_starts(data):
    """starts[r] = offset of read r; starts[reads] = the offset past the last read's last base"""
    spans = read_spans(data)
    return [b for b, _ in spans] + [spans[-1][1] if spans else 0]


def windows(read, L):
    """[(position in the read, key, key of the reverse complement)] of every valid window"""
    out, fwd, rc, run = [], 0, 0, 0
    mask, top = (1 << (2 * L)) - 1, 2 * (L - 1)
    for i, ch in enumerate(read):
        c = CODE.get(ch)
        if c is None:
            run = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        run += 1
        if run >= L:
            out.append((i - L + 1, fwd, rc))
    return out


def revcomp(x, L):
    r = 0
    for _ in range(L):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def fnv(x):
    """FNV-1a-64 of the 16 little-endian bytes of x (BigInteger.hh:572-582)"""
    h = FNV_SEED
    for i in range(16):
        h = ((h ^ ((x >> (8 * i)) & 0xFF)) * FNV_PRIME) & MASK64
    return h


def canonical(x, L):
    """whichever of x and its reverse complement has the smaller hash, ties to the smaller value (RankSelect.hh:126-140)"""
    r = revcomp(x, L)
    hx, hr = fnv(x), fnv(r)
    return r if (hr < hx or (hr == hx and r < x)) else x


def _fnv_np(vals):
    lo = np.array([v & MASK64 for v in vals], dtype=np.uint64)
    hi = np.array([v >> 64 for v in vals], dtype=np.uint64)
    h = np.full(len(vals), FNV_SEED, dtype=np.uint64)
    prime = np.uint64(FNV_PRIME)
    with np.errstate(over="ignore"):
        for w in (lo, hi):
            for i in range(8):
                h = (h ^ ((w >> np.uint64(8 * i)) & np.uint64(0xFF))) * prime
    return h


def canonical_many(pairs):
    """canonical form of every (key, reverse complement) pair, the hashes through numpy"""
    if not pairs:
        return []
    hx, hr = _fnv_np([p[0] for p in pairs]), _fnv_np([p[1] for p in pairs])
    return [r if (b < a or (a == b and r < x)) else x for (x, r), a, b in zip(pairs, hx.tolist(), hr.tolist())]


def object_keys(data, K, graph):
    """what build-graph (both strands of every (K + 1)-mer) or build-kmer-set (the canonical K-mers) makes of the reads"""
    L = K + 1 if graph else K
    keys = set()
    for b, e in read_spans(data):
        ws = windows(data[b:e], L)
        if graph:
            for _, x, r in ws:
                keys.add(x)
                keys.add(r)
        else:
            keys.update(canonical_many([(x, r) for _, x, r in ws]))
    return keys


# ---- the entry point ---------------------------------------------------------------------------------------------------

def match(data, L, keys, normalize=False, any=False):
    """(windows[], hits[], starts[], info) as goss_gpu_object_match_reads answers"""
    spans = read_spans(data)
    nwin, nhit = [], []
    for b, e in spans:
        ws = windows(data[b:e], L)
        ks = canonical_many([(x, r) for _, x, r in ws]) if normalize else [x for _, x, _ in ws]
        h = sum(1 for x in ks if x in keys)
        nwin.append(len(ws))
        nhit.append((1 if h else 0) if any else h)
    info = {"reads": len(spans), "windows": sum(nwin), "hits": sum(nhit), "matched_reads": sum(1 for h in nhit if h)}
    return nwin, nhit, read_starts(data), info


def first_failing_window(data, L, fails, normalize=False):
    """byte offset of the first window (in input order) whose looked-up key satisfies fails(key), or None"""
    for b, e in read_spans(data):
        ws = windows(data[b:e], L)
        ks = canonical_many([(x, r) for _, x, r in ws]) if normalize else [x for _, x, _ in ws]
        for (p, _, _), x in zip(ws, ks):
            if fails(x):
                return b + p
    return None


# ---- the parsers' framing (what reaches the device: the bases of each read) --------------------------------------------

def parse_lines(text):
    """LineParser: every line is a read; a last line without '\\n' counts when it is not empty"""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return parts


def parse_fasta(text):
    reads, cur = [], None
    for ln in parse_lines(text):
        if ln[:1] == b">":
            if cur is not None:
                reads.append(cur)
            cur = b""
        else:
            cur += ln
    if cur is not None:
        reads.append(cur)
    return reads


def parse_fastq(text):
    lines = parse_lines(text)
    return [lines[i + 1] for i in range(0, len(lines) - 3, 4)]


PARSERS = {"line": parse_lines, "fasta": parse_fasta, "fastq": parse_fastq}


def item_order(items):
    """items: [(format, bytes)] in command-line order -> the reference's order: line files, then FASTA, then FASTQ"""
    return [it for fmt in ("line", "fasta", "fastq") for it in items if it[0] == fmt]


def _matches(read, L, keys, normalize):
    ws = windows(read, L)
    ks = canonical_many([(x, r) for _, x, r in ws]) if normalize else [x for _, x, _ in ws]
    return any(x in keys for x in ks)


def extract_reads(items, K, edges):
    """(stdout bytes, matching reads, reads) of goss extract-reads: L = K + 1, no normalisation"""
    out, m, n = [], 0, 0
    for fmt, text in item_order(items):
        for r in PARSERS[fmt](text):
            n += 1
            if _matches(r, K + 1, edges, False):
                m += 1
                out.append(r + b"\n")
    return b"".join(out), m, n


def pair_files(name):
    """pairFiles (GossCmdFilterReads.cc:164-172)"""
    dot = name.rfind(".")
    pre, suf = (name[:dot], name[dot:]) if dot >= 0 else (name, "")
    return pre + "_1" + suf, pre + "_2" + suf


def filter_reads(items, K, kmers, pairs=False, match_name="m.txt", non_match_name="n.txt"):
    """{file name: bytes} of goss filter-reads: either strand of a K-mer; with pairs, files 2i and 2i + 1 in lockstep"""
    ordered = item_order(items)
    if not pairs:
        out = {match_name: [], non_match_name: []}
        for fmt, text in ordered:
            for r in PARSERS[fmt](text):
                out[match_name if _matches(r, K, kmers, True) else non_match_name].append(r + b"\n")
        return {n: b"".join(v) for n, v in out.items()}
    if len(ordered) % 2:
        raise ValueError("an even number of input files is required")
    m1, m2 = pair_files(match_name)
    n1, n2 = pair_files(non_match_name)
    out = {m1: [], m2: [], n1: [], n2: []}
    for i in range(0, len(ordered), 2):
        a, b = PARSERS[ordered[i][0]](ordered[i][1]), PARSERS[ordered[i + 1][0]](ordered[i + 1][1])
        if len(a) != len(b):
            raise ValueError("unequal read counts")
        for x, y in zip(a, b):
            hit = _matches(x, K, kmers, True) or _matches(y, K, kmers, True)
            out[m1 if hit else n1].append(x + b"\n")
            out[m2 if hit else n2].append(y + b"\n")
    return {n: b"".join(v) for n, v in out.items()}


# ---- inputs ------------------------------------------------------------------------------------------------------------

def genome(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc_text(s):
    return "".join(COMP[c] for c in reversed(s))


def build_reads(seed, genome_len=6000, nreads=700, read_len=100):
    """(genome, the '\\n'-terminated reads an object is built from): error-free reads of both strands"""
    rng = random.Random(seed)
    gen = genome(rng, genome_len)
    reads = []
    for _ in range(nreads):
        p = rng.randrange(genome_len - read_len)
        r = gen[p:p + read_len]
        reads.append(r if rng.random() < 0.5 else rc_text(r))
    return gen, ("\n".join(reads) + "\n").encode()


def query_reads(seed, gen, L, nreads=400, read_len=100, long_read=200000, trailing_newline=True):
    """The bytes to match: half the reads drawn from `gen` with substitution errors, half from an unrelated genome; lower
    case, Ns, empty reads, reads of L - 1, L and L + 1 bases sprinkled in, and one read of `long_read` bases (pieces of
    `gen` between foreign stretches).  trailing_newline=False leaves the last read without its '\\n'."""
    rng = random.Random(seed * 7919 + 1)
    other = genome(rng, len(gen))
    reads = []
    for i in range(nreads):
        src = gen if i % 2 == 0 else other
        p = rng.randrange(len(src) - read_len)
        r = list(src[p:p + read_len])
        if rng.random() < 0.5:
            r = list(rc_text("".join(r)))
        if src is gen:
            for _ in range(rng.choice((0, 1, 2, 4, 8))):          # substitution errors
                j = rng.randrange(read_len)
                r[j] = rng.choice([c for c in "ACGT" if c != r[j]])
        if i % 11 == 3:
            r[rng.randrange(read_len)] = "N"
        if i % 13 == 5:
            a = rng.randrange(read_len - 10)
            r[a:a + 10] = [c.lower() for c in r[a:a + 10]]
        reads.append("".join(r))
        if i % 37 == 7:
            reads.append("")
        if i % 41 == 9:
            p = rng.randrange(len(gen) - L - 1)
            reads += [gen[p:p + L - 1], gen[p:p + L], gen[p:p + L + 1]]
    if long_read:
        pieces, n = [], 0
        while n < long_read:
            if len(pieces) % 2 == 0:
                piece = genome(rng, rng.randrange(500, 3000))
            else:
                p = rng.randrange(len(gen) - 400)
                piece = gen[p:p + rng.randrange(L, 400)]
            pieces.append(piece)
            n += len(piece)
        reads.insert(len(reads) // 2, "".join(pieces))
    reads.append("")                                              # two adjacent '\n' at the end, too
    reads.append(gen[5:5 + read_len])
    text = "\n".join(reads)
    return (text + "\n" if trailing_newline else text).encode()


def as_fasta(reads, width=60):
    out = []
    for i, r in enumerate(reads):
        out.append(b">r%d some text" % i)
        out += [r[j:j + width] for j in range(0, len(r), width)]
    return b"\n".join(out) + b"\n"


def as_fastq(reads):
    out = []
    for i, r in enumerate(reads):
        out += [b"@q%d" % i, r, b"+", b"I" * len(r)]
    return b"\n".join(out) + b"\n"
