// goss_knobs.hpp -- the three records of a context that are not state of a build: the knobs read from the environment
// once, the diagnostic counters behind goss_gpu_stat, and the guard through which a flag is lent to a call.  Host-only
// (no HIP include): tests/knobs_check.cpp compiles it by itself under the host compiler's sanitizers.
#pragma once

#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace goss {

// ---- knobs -------------------------------------------------------------------------------------------
// What goss_gpu_create takes from GOSS_GPU_* (knobs_from_env; the table below says which variable and by what rule).
// Not const: a build that finds a form unusable demotes it for the rest of the context's life (count_rem32, count_sub8
// and count_dense in fused_path.hpp, radix_sort in count_path.hpp), and goss_gpu_reset leaves the knobs -- the
// demotions included -- alone.  Anything else that changes one lends it through Scoped (below).
struct Knobs {
    bool lookback = true;               // single-pass radix scatter (GOSS_GPU_NO_LOOKBACK=1 disables)
    bool ordered_tiles = false;         // take tile numbers from a ticket instead of blockIdx
    double est_scale = 1.0;             // GOSS_GPU_EST_SCALE: factor on the distinct-key estimate of the fused path (tests)
    uint32_t order_bits = 0;            // group bits of the canonical re-ordering (GOSS_GPU_ORDER_BITS=16|20; 0 = by size)
    bool fused = true;                  // GOSS_GPU_NO_FUSED=1: never fuse the first partition pass into the extraction
    bool fused_msd = true;              // GOSS_GPU_NO_MSD=1: never use the two-level (sub-region) form
    bool graph_rep = true;              // GOSS_GPU_NO_GRAPH_REP=1: the fused path of a graph build counts both strands of every window (round 3's form)
    int canon_l1 = 1;                   // GOSS_GPU_CANON_L1=0|1|2: the fused first level computes gossamer's canonical form itself never / from kCanonL1At distinct keys per window on / always
    bool rem32 = true;                  // GOSS_GPU_NO_REM32=1: never take the 32-bit-remainder form of the second level and the counting
    uint32_t rem32_bits_min = 0;        // GOSS_GPU_REM32_BITS=<9..12>: at least that many second-level bits (tests)
    uint32_t rem32_split_min = 0;       // GOSS_GPU_REM32_SPLIT=<0..4>: at least that many third-level bits (tests; raised when tables overflow)
    int rem32_slots = 0;                // GOSS_GPU_REM32_SLOTS=2048|4096|8192|16384: counting table of that form (0 = by the distinct-key estimate)
    bool narrow = true;                 // GOSS_GPU_NARROW=0: 8-byte keys between the two levels of the 32-bit-remainder form (rounds 3-4)
    bool overflow_by_sort = true;       // GOSS_GPU_OVERFLOW_BY_SORT=0: a table that overflows sends the whole chunk up the ladder of forms (rounds 1-5)
    uint32_t narrow_capg = 0xFFFFFFFFu; // GOSS_GPU_NARROW_CAPG (tests): granules a tile of the narrow form may lay out before it sends its carried granules off short (576 at least; by default and at most what the kernel's LDS layout holds)
    uint32_t r32_small_max = 0;         // distinct keys per segment up to which the 2048-slot table is taken (GOSS_GPU_R32_SMALL_MAX; 0 = the form's default)
    bool big_table = true;              // GOSS_GPU_NO_BIG_TABLE=1: never count 16-bit segments in the 8192-slot table
    uint64_t hash_merge_min = 1u << 20; // GOSS_GPU_HASH_MERGE_MIN=<entries>: smallest merge that goes through the counting table (65 536 workgroups)
    uint32_t blk_log2_max = 0;          // GOSS_GPU_BLK_LOG2=<b>: blocks of the fused extraction of at most 2^b slots (experiments)
    bool no_fast32 = false;             // GOSS_GPU_NO_FAST32=1: the fused extraction of one-word keys in its 64-bit form (tests of both forms)
    bool table96 = true;                // GOSS_GPU_NO_TABLE96=1: never count two-word keys as 96-bit remainders in 16-byte slots
    bool wide_table = true;             // GOSS_GPU_NO_WIDE_TABLE=1: never count two-word keys in the 6144-slot table
    int big_rounds_min = 0;             // GOSS_GPU_BIG_ROUNDS_MIN=<r>: at least 2^r (tests)
    bool size_by_valid = true;          // GOSS_GPU_NO_VALID_SIZING=1: key buffers always hold one key per window start
    uint64_t fused_min = 32u << 20;     // GOSS_GPU_FUSED_MIN=<window starts>: smallest chunk the fused path takes
    double fused_capscale = 1.0;        // GOSS_GPU_FUSED_CAPSCALE: multiplies the bucket regions (tests force overflows)
    bool debug = false;                 // GOSS_GPU_DEBUG=1: say on stderr why a fast path was not taken
};

// When a variable's text is taken and what number it stands for.  `lo`, `hi` are the row's.
enum class Rule {
    IsOne,        // begins with '1' -> 1
    Truthy,       // not empty and does not begin with '0' -> 1
    Digit,        // begins with a digit lo..hi -> that digit
    IntIn,        // atoi in lo..hi -> it
    Pow2In,       // atoi a power of two in lo..hi -> it
    IntAny,       // set at all, the empty string too -> atoi
    IntSet,       // not empty -> atoi
    IntClamp,     // not empty -> atoi, clamped to lo..hi
    U64Set,       // not empty -> strtoull
    FloatPos,     // atof > 0 -> it
    FloatSet,     // not empty -> atof
};

// A Knobs field of one of the five types there are.
struct KnobField {
    enum Type { Bool, Int, U32, U64, Double } type;
    union { bool Knobs::*b; int Knobs::*i; uint32_t Knobs::*u; uint64_t Knobs::*q; double Knobs::*d; };
    constexpr KnobField(bool Knobs::*p) : type(Bool), b(p) {}
    constexpr KnobField(int Knobs::*p) : type(Int), i(p) {}
    constexpr KnobField(uint32_t Knobs::*p) : type(U32), u(p) {}
    constexpr KnobField(uint64_t Knobs::*p) : type(U64), q(p) {}
    constexpr KnobField(double Knobs::*p) : type(Double), d(p) {}
};

struct KnobRow {
    const char* name;
    KnobField field;
    Rule rule;
    int lo, hi;
    bool negate;          // a NO_ variable: the field is what the rule yields, negated
};

inline const KnobRow* knob_table(size_t* n)
{
    static const KnobRow rows[] = {
        {"GOSS_GPU_NO_LOOKBACK", &Knobs::lookback, Rule::IsOne, 0, 0, true},
        {"GOSS_GPU_ORDERED_TILES", &Knobs::ordered_tiles, Rule::IsOne, 0, 0, false},
        {"GOSS_GPU_EST_SCALE", &Knobs::est_scale, Rule::FloatPos, 0, 0, false},
        {"GOSS_GPU_ORDER_BITS", &Knobs::order_bits, Rule::IntIn, 16, 24, false},
        {"GOSS_GPU_NO_FUSED", &Knobs::fused, Rule::IsOne, 0, 0, true},
        {"GOSS_GPU_NO_MSD", &Knobs::fused_msd, Rule::IsOne, 0, 0, true},
        {"GOSS_GPU_NO_GRAPH_REP", &Knobs::graph_rep, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_CANON_L1", &Knobs::canon_l1, Rule::Digit, 0, 2, false},
        {"GOSS_GPU_NO_REM32", &Knobs::rem32, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_REM32_BITS", &Knobs::rem32_bits_min, Rule::IntIn, 9, 10, false},
        {"GOSS_GPU_REM32_SPLIT", &Knobs::rem32_split_min, Rule::IntIn, 0, 4, false},
        {"GOSS_GPU_REM32_SLOTS", &Knobs::rem32_slots, Rule::Pow2In, 2048, 16384, false},
        {"GOSS_GPU_NARROW", &Knobs::narrow, Rule::IntAny, 0, 0, false},
        {"GOSS_GPU_OVERFLOW_BY_SORT", &Knobs::overflow_by_sort, Rule::IntAny, 0, 0, false},
        {"GOSS_GPU_NARROW_CAPG", &Knobs::narrow_capg, Rule::IntIn, 1, INT_MAX, false},
        {"GOSS_GPU_R32_SMALL_MAX", &Knobs::r32_small_max, Rule::IntAny, 0, 0, false},
        {"GOSS_GPU_NO_BIG_TABLE", &Knobs::big_table, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_HASH_MERGE_MIN", &Knobs::hash_merge_min, Rule::U64Set, 0, 0, false},
        {"GOSS_GPU_BLK_LOG2", &Knobs::blk_log2_max, Rule::IntSet, 0, 0, false},
        {"GOSS_GPU_NO_FAST32", &Knobs::no_fast32, Rule::IsOne, 0, 0, false},
        {"GOSS_GPU_NO_TABLE96", &Knobs::table96, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_NO_WIDE_TABLE", &Knobs::wide_table, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_BIG_ROUNDS_MIN", &Knobs::big_rounds_min, Rule::IntClamp, 0, 3, false},
        {"GOSS_GPU_NO_VALID_SIZING", &Knobs::size_by_valid, Rule::Truthy, 0, 0, true},
        {"GOSS_GPU_FUSED_MIN", &Knobs::fused_min, Rule::U64Set, 0, 0, false},
        {"GOSS_GPU_FUSED_CAPSCALE", &Knobs::fused_capscale, Rule::FloatSet, 0, 0, false},
        {"GOSS_GPU_DEBUG", &Knobs::debug, Rule::IsOne, 0, 0, false},
    };
    *n = sizeof rows / sizeof rows[0];
    return rows;
}

// The rule applied to a variable's text (never null): false = the text is ignored.  An integer comes back in *u (two's
// complement of what atoi said), a fraction in *d.
inline bool knob_parse(const KnobRow& r, const char* e, unsigned long long* u, double* d)
{
    const int v = std::atoi(e);
    *u = (unsigned long long)(long long)v;
    *d = 0;
    switch (r.rule)
    {
        case Rule::IsOne: *u = 1; return *e == '1';
        case Rule::Truthy: *u = 1; return *e && *e != '0';
        case Rule::Digit: *u = (unsigned long long)(*e - '0'); return *e >= '0' + r.lo && *e <= '0' + r.hi;
        case Rule::IntIn: return v >= r.lo && v <= r.hi;
        case Rule::Pow2In: return v >= r.lo && v <= r.hi && (v & (v - 1)) == 0;
        case Rule::IntAny: return true;
        case Rule::IntSet: return *e != 0;
        case Rule::IntClamp: *u = (unsigned long long)(v < r.lo ? r.lo : v > r.hi ? r.hi : v); return *e != 0;
        case Rule::U64Set: *u = std::strtoull(e, nullptr, 10); return *e != 0;
        case Rule::FloatPos: *d = std::atof(e); return *d > 0;
        case Rule::FloatSet: *d = std::atof(e); return *e != 0;
    }
    return false;
}

inline Knobs knobs_from_env()
{
    Knobs k;
    size_t n = 0;
    const KnobRow* rows = knob_table(&n);
    for (size_t j = 0; j < n; ++j)
    {
        const KnobRow& r = rows[j];
        const char* e = std::getenv(r.name);
        unsigned long long u = 0;
        double d = 0;
        if (!e || !knob_parse(r, e, &u, &d)) continue;
        switch (r.field.type)
        {
            case KnobField::Bool: k.*r.field.b = (u != 0) != r.negate; break;
            case KnobField::Int: k.*r.field.i = (int)(long long)u; break;
            case KnobField::U32: k.*r.field.u = (uint32_t)u; break;
            case KnobField::U64: k.*r.field.q = u; break;
            case KnobField::Double: k.*r.field.d = d; break;
        }
    }
    return k;
}

// ---- counters ----------------------------------------------------------------------------------------
// What goss_gpu_stat serves by name (stat_table).  They only ever grow or are overwritten by the next build's figure:
// goss_gpu_reset leaves them as they are, so a context that serves several builds in a row reports their sum.
struct Stats {
    uint64_t fused_chunks = 0;          // chunks counted by the fused path
    uint64_t rep_chunks = 0;            // chunks counted in strand-representative space and mapped to canonical order afterwards
    uint64_t canon_chunks = 0;          // chunks whose first level computed the canonical form itself
    uint64_t rec_chunks = 0;            // chunks counted from records by the fused path
    uint64_t flush_wait_us = 0, flush_count_us = 0, flushes = 0;   // staging buffer counted: waiting for queued copies / counting (host wall)
    uint64_t fused_overflows = 0;       // fused chunks redone because a bucket region was too small
    uint64_t fused_msd_chunks = 0;      // chunks counted by the two-level form
    uint64_t rem32_chunks = 0;          // chunks counted in the 32-bit-remainder form
    uint64_t narrow_chunks = 0;         // ... of them with remainder + digit (5.33 bytes a key) between the two levels
    uint64_t overflow_units = 0;        // segments counted by sort because their table overflowed
    uint64_t pk_fused_chunks = 0;       // chunks of a packed string the fused kernels read as they were
    uint64_t pk_unpacked_chunks = 0;    // ... and chunks (or samples) unpacked to bytes for the plain kernels
    uint64_t assemble_us = 0;           // host clock of the last goss_gpu_emit_assemble
    uint64_t ds_blocks_ranges = 0, ds_blocks_own = 0;      // DenseSelect blocks of the last assembly: taken from the ranges' records / built here from the bitmap
    uint64_t rem32_bits_last = 0;       // second-level bits of the last chunk counted in the 32-bit-remainder form
    uint64_t rem32_split_last = 0;      // third-level bits of the last chunk counted in that form
    uint64_t big_table_chunks = 0;      // chunks of 16-bit segments counted in the 8192-slot table
    uint64_t wide_table_chunks = 0;     // ... of them, two-word keys in the 6144-slot table
    uint64_t table96_chunks = 0;        // chunks of two-word keys counted as 96-bit remainders
    uint64_t valid_sized_chunks = 0;    // chunks counted in key buffers sized from the estimated share of valid windows
    uint64_t valid_resizes = 0;         // chunks whose estimate was too low: redone in full-size buffers
    uint64_t seg_merges = 0;            // merges done by segments
    uint64_t hash_merges = 0;           // ... of them through the counting table (seg_hash_merge96_kernel)
    uint64_t segment_retries = 0;       // segment path attempts that overflowed an LDS table
    uint64_t lookback_failures = 0;
    uint64_t arena_ms = 0;              // time hipMalloc took to map the arena
    uint64_t arena_grows = 0;
};

struct StatRow { const char* name; uint64_t Stats::*field; };

// Every name goss_gpu_stat knows but "runs" and "arena_bytes", which are no counters.  Four names are not their
// field's: they are the public spelling and stay.
inline const StatRow* stat_table(size_t* n)
{
    static const StatRow rows[] = {
        {"fused_chunks", &Stats::fused_chunks},
        {"rep_chunks", &Stats::rep_chunks},
        {"canon_chunks", &Stats::canon_chunks},
        {"rec_chunks", &Stats::rec_chunks},
        {"flush_wait_us", &Stats::flush_wait_us},
        {"flush_count_us", &Stats::flush_count_us},
        {"flushes", &Stats::flushes},
        {"fused_overflows", &Stats::fused_overflows},
        {"fused_msd_chunks", &Stats::fused_msd_chunks},
        {"rem32_chunks", &Stats::rem32_chunks},
        {"narrow_chunks", &Stats::narrow_chunks},
        {"overflow_units", &Stats::overflow_units},
        {"packed_fused_chunks", &Stats::pk_fused_chunks},
        {"packed_unpacked_chunks", &Stats::pk_unpacked_chunks},
        {"assemble_us", &Stats::assemble_us},
        {"ds_blocks_from_ranges", &Stats::ds_blocks_ranges},
        {"ds_blocks_assembled", &Stats::ds_blocks_own},
        {"rem32_bits", &Stats::rem32_bits_last},
        {"rem32_split", &Stats::rem32_split_last},
        {"big_table_chunks", &Stats::big_table_chunks},
        {"wide_table_chunks", &Stats::wide_table_chunks},
        {"table96_chunks", &Stats::table96_chunks},
        {"valid_sized_chunks", &Stats::valid_sized_chunks},
        {"valid_resizes", &Stats::valid_resizes},
        {"seg_merges", &Stats::seg_merges},
        {"hash_merges", &Stats::hash_merges},
        {"segment_retries", &Stats::segment_retries},
        {"lookback_failures", &Stats::lookback_failures},
        {"arena_ms", &Stats::arena_ms},
        {"arena_grows", &Stats::arena_grows},
    };
    *n = sizeof rows / sizeof rows[0];
    return rows;
}

inline bool stat_lookup(const Stats& s, const char* name, uint64_t* value)
{
    size_t n = 0;
    const StatRow* rows = stat_table(&n);
    for (size_t j = 0; j < n; ++j)
        if (std::strcmp(rows[j].name, name) == 0) { *value = s.*rows[j].field; return true; }
    return false;
}

// ---- a flag lent to a call ---------------------------------------------------------------------------
// *p holds `v` while the guard lives and what it held before afterwards, however the scope is left: the way a field
// of the context is made an argument of the calls below a point (mute_timing, more_follows, more_starts, valid_frac,
// a lookback switched off for an auxiliary sort).
template <class T>
struct Scoped {
    T* p;
    T was;
    Scoped(T* ptr, T v) : p(ptr), was(*ptr) { *p = v; }
    ~Scoped() { *p = was; }
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
};

}  // namespace goss
