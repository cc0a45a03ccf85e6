// gossamer_amd/csrc/goss_read_src.hpp by itself, under the host compiler and its sanitizers (tests/test_read_src_cpu.py
// builds and runs this): ReadSrc::advance, launch and to_next16 against the arithmetic they replace -- byte addresses
// split by hand into aligned + mis, a packed string passed as the address 2^44 + position that the launch sites turned
// back into its group's two pointers, records advanced by (slots / 16) * record bytes.  What launch() returns is read
// through, so that a pointer outside the arrays is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "goss_read_src.hpp"

using goss::ReadSrc;

static int failures = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) { if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// ---- the arithmetic of before ---------------------------------------------------------------------
constexpr uintptr_t kFake = (uintptr_t)1 << 44;          // "address" of position 0 of a packed string
struct Old { const uint8_t* base; uint32_t mis; const uint16_t* bad; };
static Old old_bytes(const uint8_t* d, uint64_t done)
{
    const uintptr_t addr = (uintptr_t)(d + done);
    const uint32_t mis = (uint32_t)(addr & 15u);
    return {(const uint8_t*)(addr - mis), mis, nullptr};
}
static Old old_packed(const uint32_t* codes, const uint16_t* bad, uint64_t pos, uint64_t done)
{
    const uintptr_t addr = kFake + pos + done;
    const uint32_t mis = (uint32_t)(addr & 15u);
    const uint64_t g = ((addr - mis) - kFake) >> 4;
    return {(const uint8_t*)(codes + g), mis, bad + g};
}
static const uint8_t* old_records(const uint8_t* d, uint64_t done, uint64_t rec_bytes) { return d + (done / 16) * rec_bytes; }
static uint64_t old_skip(uintptr_t addr) { return (uint64_t)(((addr + 15) & ~(uintptr_t)15) - addr); }

static bool same(const ReadSrc::Launch& a, const Old& b) { return a.base == b.base && a.mis == b.mis && a.bad == b.bad; }

int main()
{
    const uint64_t dones[] = {0, 4096, 8192, 3 * 4096, 17 * 4096, 1, 15, 16, 17, 4095, 12345};

    // bytes at every misalignment, chunk after chunk
    {
        std::vector<uint8_t> store(20 * 4096 + 64, (uint8_t)'A');
        const uint8_t* al = (const uint8_t*)(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
        unsigned sum = 0;
        for (uint32_t mis = 0; mis < 16; ++mis)
        {
            const uint8_t* d = al + mis;
            const ReadSrc s = ReadSrc::of_bytes(d);
            CHECK(s.launch().kind == ReadSrc::Bytes && s.launch().mis == mis && s.launch().base == al);
            CHECK(s.to_next16() == old_skip((uintptr_t)d));
            CHECK(s.advance(s.to_next16()).launch().mis == 0 && s.advance(s.to_next16()).launch().base == d + old_skip((uintptr_t)d));
            for (uint64_t done : dones)
            {
                const ReadSrc::Launch in = s.advance(done).launch();
                CHECK(same(in, old_bytes(d, done)));
                CHECK(same(s.advance(4096).advance(done).launch(), old_bytes(d, 4096 + done)));
                sum += in.base[in.mis];
            }
        }
        CHECK(sum == 16 * (sizeof(dones) / sizeof(dones[0])) * 'A');
        std::printf("ok bytes\n");
    }

    // packed strings: first positions on, before and behind group boundaries (a staged push begins where the last ended)
    {
        const uint64_t npos = 24 * 4096;
        std::vector<uint32_t> codes(npos / 16 + 4, 7u);
        std::vector<uint16_t> bad(npos / 16 + 4, 3u);
        const uint64_t poss[] = {0, 1, 7, 15, 16, 17, 31, 32, 33, 255, 256, 4095, 4096, 4096 + 5, 5 * 4096 + 15, 5 * 4096 + 16};
        uint64_t sum = 0, n = 0;
        for (uint64_t pos : poss)
        {
            const ReadSrc s = ReadSrc::of_packed(codes.data(), bad.data(), pos);
            CHECK(s.to_next16() == old_skip(kFake + pos));
            CHECK(same(s.advance(s.to_next16()).launch(), old_packed(codes.data(), bad.data(), pos + old_skip(kFake + pos), 0)));
            for (uint64_t done : dones)
            {
                const ReadSrc::Launch in = s.advance(done).launch();
                CHECK(in.kind == ReadSrc::Packed);
                CHECK(same(in, old_packed(codes.data(), bad.data(), pos, done)));
                CHECK(same(s.advance(4096).advance(done).launch(), old_packed(codes.data(), bad.data(), pos, 4096 + done)));
                CHECK(in.mis == ((pos + done) & 15u) && (const uint32_t*)in.base - codes.data() == (int64_t)((pos + done) >> 4));
                sum += *(const uint32_t*)in.base + *in.bad;
                ++n;
            }
        }
        CHECK(sum == 10 * n);
        std::printf("ok packed\n");
    }

    // records of 12 and 20 bytes: chunks of whole multiples of 4096 slots, laid end to end as the chunk loop cuts them
    for (uint32_t rb : {12u, 20u})
    {
        const uint64_t nrecs = 3 * 4096 + 777;
        std::vector<uint8_t> store(nrecs * rb + 3, (uint8_t)1);
        for (uint32_t off = 0; off < 3; ++off)          // (records lie where the caller put them: any address)
        {
            const uint8_t* d = store.data() + off;
            const ReadSrc s = ReadSrc::of_records(d, rb);
            CHECK(s.launch().kind == ReadSrc::Records && s.launch().mis == 0 && s.launch().base == d && s.launch().bad == nullptr);
            for (uint64_t m : {0u, 1u, 2u, 5u, 12u})
            {
                const uint64_t done = m * 4096;
                if (done / 16 >= nrecs) continue;
                CHECK(s.advance(done).launch().base == old_records(d, done, rb) && s.advance(done).launch().mis == 0);
                CHECK(s.advance(4096).advance(done).bytes == old_records(d, 4096 + done, rb));
            }
            for (uint64_t capn : {(uint64_t)4096, (uint64_t)2 * 4096, (uint64_t)7 * 4096})
            {
                const uint64_t total = nrecs * 16;
                uint64_t done = 0, seen = 0;
                const uint8_t* expect = d;
                while (done < total)
                {
                    const uint64_t ns = capn < total - done ? capn : total - done;
                    const ReadSrc::Launch in = s.advance(done).launch();
                    CHECK(in.base == expect && in.base == old_records(d, done, rb));
                    for (uint64_t r = 0; r < ns / 16; ++r) seen += in.base[r * rb + rb - 1];
                    expect += ns / 16 * rb;
                    done += ns;
                }
                CHECK(expect == d + nrecs * rb && seen == nrecs);
            }
        }
        std::printf("ok records %u\n", rb);
    }
    if (failures) { std::printf("FAILED: %d checks\n", failures); return 1; }
    return 0;
}
