// The 32-bit words that travel between the first level, the second level and the counting kernel of the
// 32-bit-remainder form, as plain functions: a host compiler can include this header by itself (tests/words_check.cpp
// does), the kernels include it through kernels_partition.hpp and kernels_count.hpp.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GOSS_HD __host__ __device__ __forceinline__
#else
#define GOSS_HD inline
#endif

namespace goss {

// ---- the remainder of a key ---------------------------------------------------------------------
// low `rbits` bits of a key, bit `sqbit` (always clear) taken out when SQ
template <bool SQ>
GOSS_HD uint32_t rem32_pack(uint64_t key, uint32_t rbits, uint32_t sqbit)
{
    const uint64_t x = key & ((1ULL << rbits) - 1ULL);
    if (!SQ) return (uint32_t)x;
    return (uint32_t)(((x >> (sqbit + 1)) << sqbit) | (x & ((1ULL << sqbit) - 1ULL)));
}
template <bool SQ>
GOSS_HD uint64_t rem32_unpack(uint32_t r, uint32_t sqbit)
{
    if (!SQ) return r;
    return (((uint64_t)r >> sqbit) << (sqbit + 1)) | ((uint64_t)r & ((1ULL << sqbit) - 1ULL));
}

// the low word of (hi:lo) >> s, 0 <= s < 32: one v_alignbit_b32 on the device
GOSS_HD uint32_t funnel_shr(uint32_t hi, uint32_t lo, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
#endif
}

// ---- the squeeze form between the first and the second level ---------------------------------------
// The squeeze form is that of 33-bit remainders (k = 25: nine second-level bits, the digit at key bits 33 .. 41), so the
// remainder's top bit is bit 0 of the key's high word and the digit the nine bits above it.  The first level stores
// the key's low word as it is and the low TEN bits of the high word as the chunk's 10-bit field: one instruction,
// in the kernel that is bound by what it issues.  The second level, which waits for memory, takes the digit from
// field >> 1 and squeezes the remainder itself.
constexpr uint32_t kNarrowSqRbits = 33, kNarrowSqDigitBits = 9;
GOSS_HD uint32_t narrow_sq_field(uint32_t key_hi) { return key_hi & 0x3FFu; }
GOSS_HD uint32_t narrow_sq_digit(uint32_t field) { return (field >> 1) & ((1u << kNarrowSqDigitBits) - 1u); }
// (what leaves the funnel's word at the top in the shift are the digit's bits: only bit 0 of `field` stays)
GOSS_HD uint32_t narrow_sq_rem(uint32_t key_lo, uint32_t field, uint32_t sqbit)
{
    return (key_lo & ((1u << sqbit) - 1u)) | (funnel_shr(field, key_lo, sqbit + 1u) << sqbit);
}

// ---- the counting table's words -----------------------------------------------------------------------
constexpr uint32_t kR32Mul = 0x9E3779B1u, kR32MulInv = 0x0E8B2F51u;          // kR32Mul * kR32MulInv = 1 mod 2^32
GOSS_HD uint32_t r32_mix(uint32_t k) { return (k ^ (k >> 15)) * kR32Mul; }
GOSS_HD uint32_t r32_unmix(uint32_t f) { const uint32_t y = f * kR32MulInv; return y ^ (y >> 15) ^ (y >> 30); }

// The IMAGE of a remainder: its mix turned by 16 bits, so that the mix's top bits -- the home bucket -- lie at bits 4 and
// up of the word, where they ARE the byte offset of a 16-byte bucket.  A table of NB buckets (512 .. 4 096) takes the low
// log2(NB) bits of the twelve-bit field at bit 4 (mix bits 20 and up) as the home bucket and those of the twelve-bit field
// at bit 20 (mix bits 4 .. 15), made odd, as the distance to the second: two fields of a bijection's value that share no
// bit, whatever the table's size -- the word does not depend on it.  The trade-off: one turn cannot put both the home
// at bit 4 and the bits just below the mix's top (the plain form's distance field) next to it, so the distance comes
// from the lower half of the product: bits 4 .. 15 of it are a function of bits 0 .. 15 of k ^ (k >> 15) alone, the weaker
// bits of a multiplicative hash.  Home buckets are spread as before; keys that share a home share their second more
// often when those bits agree.  A per-mille of the keys looks at a second bucket at all, and no count depends on
// where a key lives.
GOSS_HD uint32_t r32_image(uint32_t k) { const uint32_t f = r32_mix(k); return (f >> 16) | (f << 16); }
GOSS_HD uint32_t r32_unimage(uint32_t w) { return r32_unmix((w >> 16) | (w << 16)); }
GOSS_HD uint32_t r32_image_home_bytes(uint32_t w, uint32_t nb) { return w & ((nb - 1u) << 4); }          // 16 * home bucket
GOSS_HD uint32_t r32_image_home(uint32_t w, uint32_t nb) { return (w >> 4) & (nb - 1u); }
GOSS_HD uint32_t r32_image_second(uint32_t w, uint32_t home, uint32_t nb) { return home ^ (((w >> 20) & (nb - 1u)) | 1u); }
// the word an empty slot of bucket `bkt` holds: home bkt ^ 1, odd field 3 -> second bucket bkt ^ 2
GOSS_HD uint32_t r32_image_marker(uint32_t bkt) { return ((bkt ^ 1u) << 4) | (3u << 20); }

// the same three on plain remainders (the forms with a third level, whose segments are split on the remainder's top bits):
// the mix is computed per key by the counting kernel, home = its top bb bits, odd field = the bb bits below
GOSS_HD uint32_t r32_plain_home(uint32_t f, uint32_t bb) { return f >> (32u - bb); }
GOSS_HD uint32_t r32_plain_second(uint32_t f, uint32_t home, uint32_t bb) { return home ^ (((f >> (32u - 2u * bb)) & ((1u << bb) - 1u)) | 1u); }
GOSS_HD uint32_t r32_plain_marker(uint32_t bkt, uint32_t bb) { return r32_unmix(((bkt ^ 1u) << (32u - bb)) | (3u << (32u - 2u * bb))); }

}  // namespace goss
