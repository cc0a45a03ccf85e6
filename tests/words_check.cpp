// Stand-alone check of gossamer_amd/csrc/goss_words.hpp with the system's C++ compiler (tests/test_words_cpu.py builds and
// runs it): the words between the first level, the second level and the counting kernel of the 32-bit-remainder form.
// Prints "ok <what>" per property, "vec ..." lines that tests/words_model.py's Python mirror is compared with, and
// exits non-zero at the first property that does not hold.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "goss_words.hpp"

using namespace goss;

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd()
{
    // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static void fail(const char* what, uint64_t a, uint64_t b)
{
    std::printf("FAILED %s: %#" PRIx64 " %#" PRIx64 "\n", what, a, b);
    std::exit(1);
}

int main()
{
    // 1. the image is a bijection with the stated inverse: all 2^32 words (some seconds on one core; the mix and its
    //    inverse are inside the image and its inverse)
    {
        uint64_t bad = 0, first = 0;
        for (uint64_t x = 0; x < (1ULL << 32); ++x)
        {
            const uint32_t w = r32_image((uint32_t)x);
            if (r32_unimage(w) != (uint32_t)x) { if (!bad) first = x; ++bad; }
        }
        if (bad) fail("unimage(image(x)) == x", first, bad);
        if (r32_image(r32_unimage(0u)) != 0u || r32_image(r32_unimage(~0u)) != ~0u) fail("image(unimage(w)) == w", 0, 0);
        std::printf("ok unimage(image(x)) == x for all 2^32 words\n");
    }
    // 2. every table size: home != second for every word of a sample and all words of few bits; the marker of bucket b
    //    has home b ^ 1 and second b ^ 2; and the plain form's marker likewise
    for (uint32_t slots = 2048; slots <= 16384; slots *= 2)
    {
        const uint32_t nb = slots / 4;
        uint32_t bb = 0;
        while ((1u << bb) < nb) ++bb;
        for (uint32_t b = 0; b < nb; ++b)
        {
            const uint32_t m = r32_image_marker(b);
            const uint32_t h = r32_image_home(m, nb);
            if (h != (b ^ 1u) || r32_image_second(m, h, nb) != (b ^ 2u) || r32_image_home_bytes(m, nb) != 16u * h) fail("image marker", slots, b);
            const uint32_t f = r32_mix(r32_plain_marker(b, bb));
            const uint32_t hp = r32_plain_home(f, bb);
            if (hp != (b ^ 1u) || r32_plain_second(f, hp, bb) != (b ^ 2u)) fail("plain marker", slots, b);
        }
        auto one = [&](uint32_t w) {
            const uint32_t h = r32_image_home(w, nb), s = r32_image_second(w, h, nb);
            if (h >= nb || s >= nb || h == s || r32_image_home_bytes(w, nb) != 16u * h) fail("home != second", slots, w);
        };
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) { one((1u << i) | (1u << j)); one(~((1u << i) | (1u << j))); }
        one(0u); one(~0u);
        for (uint32_t i = 0; i < (1u << 20); ++i) one((uint32_t)rnd());
        std::printf("ok table of %u slots: home != second, marker of b at home b ^ 1 with second b ^ 2\n", slots);
    }
    // 3. squeeze pack / unpack: 33-bit values with bit 24 clear
    {
        const uint32_t sqbit = 24;
        for (uint32_t i = 0; i < (1u << 24); ++i)
        {
            const uint64_t x = rnd() & ((1ULL << 33) - 1ULL) & ~(1ULL << sqbit);
            const uint32_t r = rem32_pack<true>(x, 33, sqbit);
            if (rem32_unpack<true>(r, sqbit) != x) fail("squeeze round trip", x, r);
        }
        // (and every packed word comes from such a value)
        for (uint32_t i = 0; i < (1u << 24); ++i)
        {
            const uint32_t r = (uint32_t)rnd();
            const uint64_t x = rem32_unpack<true>(r, sqbit);
            if ((x >> 33) || ((x >> sqbit) & 1ULL) || rem32_pack<true>(x, 33, sqbit) != r) fail("squeeze round trip (words)", x, r);
        }
        std::printf("ok squeeze pack / unpack on 33-bit values with bit 24 clear\n");
    }
    // 4. the first level's (low word, 10-bit field) and the second level's rebuild = rem32_pack<true> and the digit, on
    //    10^6 random 50-bit keys with bit 24 clear -- with and without junk above the key's bits in the high word
    {
        const uint32_t sqbit = 24;
        for (uint32_t i = 0; i < 1000000u; ++i)
        {
            const uint64_t key = rnd() & ((1ULL << 50) - 1ULL) & ~(1ULL << sqbit);
            const uint32_t junk = (i & 1u) ? (uint32_t)rnd() << 18 : 0u;
            const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32) | junk;
            const uint32_t field = narrow_sq_field(hi);
            // (the second level sees the field with its neighbours above it: dw >> 10 m)
            const uint32_t seen = field | ((uint32_t)rnd() << 10);
            if (narrow_sq_rem(lo, seen, sqbit) != rem32_pack<true>(key, kNarrowSqRbits, sqbit)) fail("rebuilt remainder", key, seen);
            if (narrow_sq_digit(seen) != (uint32_t)(key >> kNarrowSqRbits) % (1u << kNarrowSqDigitBits)) fail("digit of the field", key, seen);
        }
        std::printf("ok (low word, field) -> remainder and digit on 10^6 keys\n");
    }
    // vectors for the Python mirror: x, mix, image, unimage(x), unpack<true>(x, 24), marker(x mod 4096)
    for (uint32_t i = 0; i < 64; ++i)
    {
        const uint32_t x = i < 4 ? (i == 0 ? 0u : i == 1 ? ~0u : i == 2 ? 1u : 0x80000000u) : (uint32_t)rnd();
        std::printf("vec %u %u %u %u %" PRIu64 " %u\n", x, r32_mix(x), r32_image(x), r32_unimage(x), rem32_unpack<true>(x, 24), r32_image_marker(x % 4096u));
    }
    return 0;
}
