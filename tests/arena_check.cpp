// gossamer_amd/csrc/goss_arena.hpp by itself, under the host compiler and its sanitizers (tests/test_arena_cpu.py
// builds and runs this): an Arena over 4 KB of host memory.  Every offset below is a literal, worked out by hand from
// the rule -- permanent blocks start at the next multiple of 256 from the bottom, temporary blocks at the last multiple
// of 256 that leaves them room below the temporary end -- and every block handed out is written over its whole length,
// so a block that overlapped another or left the buffer would be seen by the address sanitizer or by the bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "goss_arena.hpp"

using namespace goss;

static int failures = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) { if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

constexpr uint64_t kSize = 4096;

struct Fixture {
    std::vector<uint8_t> buf = std::vector<uint8_t>(kSize, 0);
    Arena a;
    Fixture() { a.base = buf.data(); a.size = kSize; a.lo = 0; a.hi = kSize; }
    // the block's offset, after writing `tag` over all of it
    uint64_t perm(uint64_t bytes, uint8_t tag) { uint8_t* p = (uint8_t*)a.perm(bytes); std::memset(p, tag, bytes); return (uint64_t)(p - a.base); }
    uint64_t temp(uint64_t bytes, uint8_t tag) { uint8_t* p = (uint8_t*)a.temp(bytes); std::memset(p, tag, bytes); return (uint64_t)(p - a.base); }
    bool all(uint64_t at, uint64_t bytes, uint8_t tag) const { for (uint64_t i = 0; i < bytes; ++i) if (buf[at + i] != tag) return false; return true; }
};

// what `f` throws: the status and the text of a StatusError, or {0, ""} when it returns
template <class F>
static StatusError thrown_by(F&& f)
{
    try { f(); }
    catch (const StatusError& e) { return e; }
    return StatusError{0, ""};
}

int main()
{
    // 1. both ends align to 256 bytes
    {
        Fixture x;
        CHECK(x.a.avail() == 4096);
        CHECK(x.perm(10, 1) == 0 && x.a.lo == 10);
        CHECK(x.perm(1, 2) == 256 && x.a.lo == 257);
        CHECK(x.perm(256, 3) == 512 && x.a.lo == 768);
        CHECK(x.a.hi == 4096);
        CHECK(x.temp(10, 4) == 3840 && x.a.hi == 3840);
        CHECK(x.temp(256, 5) == 3584 && x.a.hi == 3584);
        CHECK(x.temp(1, 6) == 3328 && x.a.hi == 3328);
        CHECK(x.a.lo == 768 && x.a.avail() == 2560);
        CHECK(x.temp(0, 7) == 3328 && x.a.hi == 3328);          // nothing asked for at an aligned end: nothing taken
        CHECK(x.all(0, 10, 1) && x.all(256, 1, 2) && x.all(512, 256, 3) && x.all(3840, 10, 4) && x.all(3584, 256, 5) && x.all(3328, 1, 6));
        std::printf("ok align\n");
    }

    // 2. the two ends never cross: GOSS_ERR_OOM with the side's text, and nothing moved
    {
        Fixture x;
        x.perm(768, 1);                     // lo 768
        x.temp(768, 2);                     // hi 3328
        CHECK(x.a.lo == 768 && x.a.hi == 3328);
        StatusError e = thrown_by([&]() { x.a.perm(2561); });
        CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (permanent)");
        CHECK(x.a.lo == 768 && x.a.hi == 3328);
        e = thrown_by([&]() { x.a.temp(2561); });          // would start at 512, inside the permanent part
        CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (temporary)");
        CHECK(x.a.lo == 768 && x.a.hi == 3328);
        // exactly what is left fits, from either side
        {
            ArenaScope s(x.a);
            CHECK(x.temp(2560, 3) == 768 && x.a.hi == 768 && x.a.avail() == 0);
            e = thrown_by([&]() { x.a.perm(1); });
            CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (permanent)");
        }
        CHECK(x.perm(2560, 4) == 768 && x.a.lo == 3328 && x.a.avail() == 0);
        e = thrown_by([&]() { x.a.temp(1); });
        CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (temporary)");
        // the guard `bytes + 256 > hi`: refused although the block itself would still lie above the permanent end
        Fixture y;
        y.temp(3584, 5);                    // hi 512, lo 0
        CHECK(y.a.hi == 512 && y.a.lo == 0);
        e = thrown_by([&]() { y.a.temp(300); });          // (512 - 300) & ~255 = 0 >= lo, but 300 + 256 > 512
        CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (temporary)");
        CHECK(y.a.hi == 512 && y.a.lo == 0);
        CHECK(y.temp(256, 6) == 256 && y.a.hi == 256);    // 256 + 256 > 512 does not hold: taken
        e = thrown_by([&]() { y.a.temp(1); });
        CHECK(e.status == GOSS_ERR_OOM && e.msg == "HBM budget exceeded (temporary)" && y.a.hi == 256);
        std::printf("ok oom\n");
    }

    // 3. a scope puts the temporary end back: on normal exit, when the body throws, nested in order; never the permanent end
    {
        static_assert(!std::is_copy_constructible<ArenaScope>::value && !std::is_copy_assignable<ArenaScope>::value, "ArenaScope is not copyable");
        Fixture x;
        x.temp(100, 1);                     // hi 3840: what is found is put back, not the arena's size
        {
            ArenaScope s(x.a);
            CHECK(x.temp(1000, 2) == 2816 && x.a.hi == 2816);
            CHECK(x.perm(100, 3) == 0 && x.a.lo == 100);
        }
        CHECK(x.a.hi == 3840 && x.a.lo == 100);
        try
        {
            ArenaScope s(x.a);
            x.temp(512, 4);
            CHECK(x.a.hi == 3328);
            x.perm(200, 5);                 // lo 456
            x.a.temp(4000);                 // throws
            CHECK(false);
        }
        catch (const StatusError& e) { CHECK(e.status == GOSS_ERR_OOM && x.a.hi == 3840 && x.a.lo == 456); }
        try
        {
            ArenaScope s(x.a);
            x.temp(256, 6);
            throw std::runtime_error("anything else");
        }
        catch (const std::runtime_error&) { CHECK(x.a.hi == 3840 && x.a.lo == 456); }
        {
            ArenaScope outer(x.a);
            x.temp(256, 7);                 // 3584
            {
                ArenaScope inner(x.a);
                x.temp(256, 8);             // 3328
                try { ArenaScope third(x.a); x.temp(256, 9); CHECK(x.a.hi == 3072); throw 1; } catch (int) { CHECK(x.a.hi == 3328); }
                CHECK(x.temp(256, 10) == 3072);
            }
            CHECK(x.a.hi == 3584);
            CHECK(x.temp(256, 11) == 3328);
        }
        CHECK(x.a.hi == 3840 && x.a.lo == 456);
        std::printf("ok scope\n");
    }

    // 4. rewind: what was taken goes back early, the scope lives on and ends at the same place
    {
        Fixture x;
        x.temp(256, 1);                     // hi 3840
        x.perm(300, 2);                     // lo 300
        {
            ArenaScope s(x.a);
            CHECK(x.temp(1024, 3) == 2816);
            s.rewind();
            CHECK(x.a.hi == 3840 && x.a.lo == 300);
            CHECK(x.temp(2048, 4) == 1792);          // the second attempt has the room of the first
            x.perm(100, 5);                 // 512 .. 612
            s.rewind();
            s.rewind();                     // (twice is once)
            CHECK(x.a.hi == 3840 && x.a.lo == 612);
            {
                ArenaScope inner(x.a);
                x.temp(512, 6);
                inner.rewind();
                CHECK(x.a.hi == 3840);
                x.temp(256, 7);
            }
            CHECK(x.a.hi == 3840);
            x.temp(512, 8);
            CHECK(x.a.hi == 3328);
        }
        CHECK(x.a.hi == 3840 && x.a.lo == 612);
        CHECK(x.all(3840, 256, 1) && x.all(0, 300, 2) && x.all(512, 100, 5));          // what lay outside the scope was never written over
        std::printf("ok rewind\n");
    }

    if (failures) std::printf("FAILED: %d check(s)\n", failures);
    return failures ? 1 : 0;
}
