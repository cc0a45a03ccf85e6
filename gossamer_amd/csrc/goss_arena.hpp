// goss_arena.hpp -- the two-ended bump arena of a context, the scope through which its temporary end is lent to a call,
// and the error that both throw.  Host-only (no HIP include): tests/arena_check.cpp compiles it by itself under the host
// compiler's sanitizers.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/goss_gpu.h"

namespace goss {

struct StatusError { int status; std::string msg; };

// Two-ended bump arena over one hipMalloc: permanent blocks grow from the bottom, temporary
// blocks from the top (given back by ArenaScope, and by nothing else).
struct Arena {
    uint8_t* base = nullptr;
    uint64_t size = 0;
    uint64_t lo = 0;        // permanent top
    uint64_t hi = 0;        // temporary bottom (offset from base)

    void* perm(uint64_t bytes)
    {
        uint64_t a = (lo + 255) & ~255ULL;
        if (a + bytes > hi) throw StatusError{GOSS_ERR_OOM, "HBM budget exceeded (permanent)"};
        lo = a + bytes;
        return base + a;
    }
    void* temp(uint64_t bytes)
    {
        if (bytes + 256 > hi) throw StatusError{GOSS_ERR_OOM, "HBM budget exceeded (temporary)"};
        uint64_t a = (hi - bytes) & ~255ULL;
        if (a < lo) throw StatusError{GOSS_ERR_OOM, "HBM budget exceeded (temporary)"};
        hi = a;
        return base + a;
    }
    uint64_t avail() const { return hi > lo ? hi - lo : 0; }
};

// Temporaries of one call or one stretch of it, given back on every way out (an exception included).  The permanent
// end is not the scope's business.
struct ArenaScope {
    Arena& a;
    const uint64_t mark;
    explicit ArenaScope(Arena& arena) : a(arena), mark(arena.hi) {}
    ~ArenaScope() { a.hi = mark; }
    // give back what was taken so far; the scope goes on (a second attempt, the next round of a loop)
    void rewind() { a.hi = mark; }
    ArenaScope(const ArenaScope&) = delete;
    ArenaScope& operator=(const ArenaScope&) = delete;
};

}  // namespace goss
