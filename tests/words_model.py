"""Python mirror of gossamer_amd/csrc/goss_words.hpp: the words of the 32-bit-remainder form (tests/test_words_cpu.py
checks it against vectors the C++ functions print).  Used to construct k-mers whose STORED word is a chosen one."""
M32 = 0xFFFFFFFF
R32_MUL, R32_MUL_INV = 0x9E3779B1, 0x0E8B2F51


def r32_mix(k):
    return ((k ^ (k >> 15)) * R32_MUL) & M32


def r32_unmix(f):
    y = (f * R32_MUL_INV) & M32
    return y ^ (y >> 15) ^ (y >> 30)


def r32_image(k):
    f = r32_mix(k)
    return ((f >> 16) | (f << 16)) & M32


def r32_unimage(w):
    return r32_unmix(((w >> 16) | (w << 16)) & M32)


def r32_image_home(w, nb):
    return (w >> 4) & (nb - 1)


def r32_image_second(w, home, nb):
    return home ^ (((w >> 20) & (nb - 1)) | 1)


def r32_image_marker(bkt):
    return ((bkt ^ 1) << 4) | (3 << 20)


def rem32_unpack_sq(r, sqbit):
    return ((r >> sqbit) << (sqbit + 1)) | (r & ((1 << sqbit) - 1))


def kmer25_with_word(word, prefix):
    """The 25-mer (forward = its strand representative: bit 24, the low bit of its central base, is clear) that the squeeze
    form stores as `word` in the sub-region of the 17-bit prefix `prefix`."""
    key = (prefix << 33) | rem32_unpack_sq(r32_unimage(word), 24)
    assert key < (1 << 50) and not (key >> 24) & 1
    return "".join("ACGT"[(key >> (2 * (24 - i))) & 3] for i in range(25))
