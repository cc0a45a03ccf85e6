"""A model of goss_gpu_object_classify_reads and of `goss group-reads` on top of it (GossCmdGroupReads.cc), in plain
Python over match_model.py (reads, windows, canonical forms) and near_model.pack_bits (the bitmap files).  Nothing here
knows the library.

A k-mer set of sorted keys carries two bits per rank, lhs and rhs.  Every valid K-window of a read is looked up in its
canonical form; a window present at rank r has the class c = 2 * lhs[r] + rhs[r], and the read's mask is the OR of
1 << c over its windows: bit 0 "M" neither side, bit 1 "H" right only, bit 2 "G" left only, bit 3 "B" both."""
import match_model as mm
import near_model as nm

# the file a mask goes to (GossCmdGroupReads.cc:605-620), written out
FILES = ("neither", "both", "rhs", "rhs", "lhs", "lhs", "ambiguous", "ambiguous",
         "both", "both", "rhs", "rhs", "lhs", "lhs", "ambiguous", "ambiguous")
SUFFIX = {"line": "txt", "fasta": "fasta", "fastq": "fastq"}


def file_of(mask):
    """one of neither, both, rhs, lhs, ambiguous"""
    return FILES[mask]


def class_str(lhs_name, rhs_name, mask):
    """classStr (GossCmdGroupReads.cc:488-526)"""
    return ("neither", "both", "definitely " + rhs_name, "probably " + rhs_name, "definitely " + lhs_name, "probably " + lhs_name,
            "ambiguous", "ambiguous", "both", "probably both", "definitely " + rhs_name, "probably " + rhs_name,
            "definitely " + lhs_name, "probably " + lhs_name, "ambiguous", "ambiguous")[mask]


def read_mask(read, K, rank_of, lhs, rhs):
    """(mask, windows) of one read; rank_of: {key: rank}"""
    ws = mm.windows(read, K)
    mask = 0
    for x in mm.canonical_many([(x, r) for _, x, r in ws]):
        r = rank_of.get(x)
        if r is not None:
            mask |= 1 << ((lhs[r] << 1) | rhs[r])
    return mask, len(ws)


def classify(data, K, keys_sorted, lhs, rhs):
    """(classes[], windows[], counts[16]) as goss_gpu_object_classify_reads answers; lhs, rhs: one bit per rank"""
    assert list(keys_sorted) == sorted(set(keys_sorted)) and len(lhs) == len(rhs) == len(keys_sorted)
    rank_of = {x: i for i, x in enumerate(keys_sorted)}
    classes, nwin, counts = [], [], [0] * 16
    for b, e in mm.read_spans(data):
        m, w = read_mask(data[b:e], K, rank_of, lhs, rhs)
        classes.append(m)
        nwin.append(w)
        counts[m] += 1
    return classes, nwin, counts


def info_of(data, K, keys_sorted, lhs, rhs):
    """the info dict of Object.classify_reads, without its time"""
    classes, nwin, counts = classify(data, K, keys_sorted, lhs, rhs)
    return {"reads": len(classes), "windows": sum(nwin), "counts": counts}


def bitmap_files(base, lhs, rhs):
    """{<base>.lhs-bits, <base>.rhs-bits}: WordyBitVector files"""
    return {base + ".lhs-bits": nm.words_to_bytes(nm.pack_bits(lhs)), base + ".rhs-bits": nm.words_to_bytes(nm.pack_bits(rhs))}


def num(x):
    """a double as a C++ stream prints it by default"""
    return "%g" % x


def stats_text(counts, lhs_name="lhs", rhs_name="rhs", dont_write=False):
    """printStats (GossCmdGroupReads.cc:809-854); total > 0"""
    total = sum(counts)
    sums = {n: 0 for n in ("lhs", "rhs", "both", "neither", "ambiguous")}
    for m, c in enumerate(counts):
        sums[file_of(m)] += c
    order = ("lhs", "rhs", "both", "neither", "ambiguous")
    if dont_write:
        return ("\t".join(num(100.0 * sums[n] / total) for n in order) + "\n").encode()
    out = ["Statistics\n", "B\tG\tH\tM\tcount\tpercent\tclass\n"]
    for i in range(16):
        out.append("%d\t%d\t%d\t%d\t%d\t%s\t\"%s\"\n" % ((i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1, counts[i],
                                                     num(100.0 * counts[i] / total), class_str(lhs_name, rhs_name, i)))
    out += ["\nSummary\n", "count\tpercent\tclass\n"]
    shown = {"lhs": lhs_name, "rhs": rhs_name}
    for n in order:
        out.append("%d\t%s\t%s\n" % (sums[n], num(100.0 * sums[n] / total), shown.get(n, n)))
    return "".join(out).encode()


def file_name(cls, fmt, prefix="", lhs_name="lhs", rhs_name="rhs", half=None):
    """filename() (GossCmdGroupReads.cc:529-577): [prefix_]class[_half].suffix; an empty name falls back to graft / host"""
    cls = {"lhs": lhs_name or "graft", "rhs": rhs_name or "host"}.get(cls, cls)
    return (prefix + "_" if prefix else "") + cls + ("_%d" % half if half else "") + "." + SUFFIX[fmt]


def group_reads(items, K, keys, lhs, rhs, pairs=False, prefix="", lhs_name="lhs", rhs_name="rhs", dont_write=False):
    """({file name: bytes}, stdout bytes) of goss group-reads.  items: [(format, bytes)] in command-line order; only one
    format is processed: the line files if there are any, else the FASTA files, else the FASTQ files."""
    keys = sorted(keys)
    rank_of = {x: i for i, x in enumerate(keys)}
    fmt = next((f for f in ("line", "fasta", "fastq") if any(it[0] == f for it in items)), "line")
    texts = [mm.PARSERS[fmt](t) for f, t in items if f == fmt]
    if pairs and len(texts) % 2:
        raise ValueError("an even number of input files is required")
    files = {}
    if not dont_write:
        for cls in ("neither", "both", "lhs", "rhs", "ambiguous"):
            for half in ((1, 2) if pairs else (None,)):
                files[file_name(cls, fmt, prefix, lhs_name, rhs_name, half)] = []
    counts = [0] * 16

    def put(cls, read, half=None):
        if not dont_write:
            files[file_name(cls, fmt, prefix, lhs_name, rhs_name, half)].append(read + b"\n")
    if not pairs:
        for reads in texts:
            for r in reads:
                m = read_mask(r, K, rank_of, lhs, rhs)[0]
                counts[m] += 1
                put(file_of(m), r)
    else:
        for i in range(0, len(texts), 2):
            if len(texts[i]) != len(texts[i + 1]):
                raise ValueError("unequal read counts")
            ms = [read_mask(a, K, rank_of, lhs, rhs)[0] | read_mask(b, K, rank_of, lhs, rhs)[0] for a, b in zip(texts[i], texts[i + 1])]
            for m in ms:
                counts[m] += 1
            for half in (1, 2):                                   # (one file of the pair after the other)
                for m, r in zip(ms, texts[i + half - 1]):
                    put(file_of(m), r, half)
    return {n: b"".join(v) for n, v in files.items()}, stats_text(counts, lhs_name, rhs_name, dont_write)
