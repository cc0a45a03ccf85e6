// gossamer_amd/csrc/goss_knobs.hpp by itself, under the host compiler and its sanitizers (tests/test_knobs_cpu.py
// builds and runs this).  The cases below are the acceptance rules of the getenv lines that goss_gpu_create had before
// the table existed, written down as literals: one text per variable that is taken, and the texts just outside its rule,
// which must leave every field at its default.  The counters' public names are those of goss_gpu_stat's former chain.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "goss_knobs.hpp"

using namespace goss;

static int failures = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) { if (++failures <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// every field of Knobs, by hand (not from the table under test)
#define KNOB_FIELDS(X)                                                                                                  \
    X(lookback) X(ordered_tiles) X(est_scale) X(order_bits) X(fused) X(fused_msd) X(graph_rep) X(canon_l1) X(rem32)     \
    X(rem32_bits_min) X(rem32_split_min) X(rem32_slots) X(narrow) X(overflow_by_sort) X(narrow_capg) X(r32_small_max)   \
    X(big_table) X(hash_merge_min) X(blk_log2_max) X(no_fast32) X(table96) X(wide_table) X(big_rounds_min)              \
    X(size_by_valid) X(fused_min) X(fused_capscale) X(debug)

static const char* const kKnobNames[] = {
#define X(f) #f,
    KNOB_FIELDS(X)
#undef X
};
constexpr size_t kKnobs = sizeof kKnobNames / sizeof kKnobNames[0];

static std::vector<double> snap(const Knobs& k)
{
    return {
#define X(f) (double)k.f,
        KNOB_FIELDS(X)
#undef X
    };
}

// the defaults, as the context's initialisers had them
static void check_defaults(const Knobs& k)
{
    CHECK(k.lookback && !k.ordered_tiles && k.est_scale == 1.0 && k.order_bits == 0 && k.fused && k.fused_msd && k.graph_rep);
    CHECK(k.canon_l1 == 1 && k.rem32 && k.rem32_bits_min == 0 && k.rem32_split_min == 0 && k.rem32_slots == 0 && k.narrow);
    CHECK(k.overflow_by_sort && k.narrow_capg == 0xFFFFFFFFu && k.r32_small_max == 0 && k.big_table && k.hash_merge_min == (1u << 20));
    CHECK(k.blk_log2_max == 0 && !k.no_fast32 && k.table96 && k.wide_table && k.big_rounds_min == 0 && k.size_by_valid);
    CHECK(k.fused_min == (32u << 20) && k.fused_capscale == 1.0 && !k.debug);
}

// var = text -> `field` reads `value` and every other field its default; taken == false: `field` too
struct Case { const char* var; const char* text; bool taken; const char* field; double value; };
static const Case kCases[] = {
    // *e == '1'
    {"GOSS_GPU_NO_LOOKBACK", "1", true, "lookback", 0}, {"GOSS_GPU_NO_LOOKBACK", "2", false, "lookback", 1},
    {"GOSS_GPU_NO_LOOKBACK", "0", false, "lookback", 1}, {"GOSS_GPU_NO_LOOKBACK", "", false, "lookback", 1},
    {"GOSS_GPU_NO_LOOKBACK", "true", false, "lookback", 1},
    {"GOSS_GPU_ORDERED_TILES", "1", true, "ordered_tiles", 1}, {"GOSS_GPU_ORDERED_TILES", "2", false, "ordered_tiles", 0},
    {"GOSS_GPU_ORDERED_TILES", "", false, "ordered_tiles", 0},
    {"GOSS_GPU_NO_FUSED", "1", true, "fused", 0}, {"GOSS_GPU_NO_FUSED", "2", false, "fused", 1}, {"GOSS_GPU_NO_FUSED", "0", false, "fused", 1},
    {"GOSS_GPU_NO_MSD", "1", true, "fused_msd", 0}, {"GOSS_GPU_NO_MSD", "2", false, "fused_msd", 1}, {"GOSS_GPU_NO_MSD", "", false, "fused_msd", 1},
    {"GOSS_GPU_NO_FAST32", "1", true, "no_fast32", 1}, {"GOSS_GPU_NO_FAST32", "2", false, "no_fast32", 0}, {"GOSS_GPU_NO_FAST32", "0", false, "no_fast32", 0},
    {"GOSS_GPU_DEBUG", "1", true, "debug", 1}, {"GOSS_GPU_DEBUG", "2", false, "debug", 0}, {"GOSS_GPU_DEBUG", "yes", false, "debug", 0},
    // not empty and not '0'
    {"GOSS_GPU_NO_GRAPH_REP", "1", true, "graph_rep", 0}, {"GOSS_GPU_NO_GRAPH_REP", "yes", true, "graph_rep", 0},
    {"GOSS_GPU_NO_GRAPH_REP", "0", false, "graph_rep", 1}, {"GOSS_GPU_NO_GRAPH_REP", "", false, "graph_rep", 1},
    {"GOSS_GPU_NO_REM32", "2", true, "rem32", 0}, {"GOSS_GPU_NO_REM32", "1", true, "rem32", 0},
    {"GOSS_GPU_NO_REM32", "0", false, "rem32", 1}, {"GOSS_GPU_NO_REM32", "", false, "rem32", 1},
    {"GOSS_GPU_NO_BIG_TABLE", "1", true, "big_table", 0}, {"GOSS_GPU_NO_BIG_TABLE", "0", false, "big_table", 1}, {"GOSS_GPU_NO_BIG_TABLE", "", false, "big_table", 1},
    {"GOSS_GPU_NO_TABLE96", "1", true, "table96", 0}, {"GOSS_GPU_NO_TABLE96", "0", false, "table96", 1}, {"GOSS_GPU_NO_TABLE96", "", false, "table96", 1},
    {"GOSS_GPU_NO_WIDE_TABLE", "7", true, "wide_table", 0}, {"GOSS_GPU_NO_WIDE_TABLE", "0", false, "wide_table", 1}, {"GOSS_GPU_NO_WIDE_TABLE", "", false, "wide_table", 1},
    {"GOSS_GPU_NO_VALID_SIZING", "1", true, "size_by_valid", 0}, {"GOSS_GPU_NO_VALID_SIZING", "0", false, "size_by_valid", 1},
    {"GOSS_GPU_NO_VALID_SIZING", "", false, "size_by_valid", 1},
    // a leading digit 0..2
    {"GOSS_GPU_CANON_L1", "0", true, "canon_l1", 0}, {"GOSS_GPU_CANON_L1", "2", true, "canon_l1", 2}, {"GOSS_GPU_CANON_L1", "3", false, "canon_l1", 1},
    {"GOSS_GPU_CANON_L1", "", false, "canon_l1", 1}, {"GOSS_GPU_CANON_L1", "-1", false, "canon_l1", 1}, {"GOSS_GPU_CANON_L1", "/", false, "canon_l1", 1},
    // atoi within a range
    {"GOSS_GPU_ORDER_BITS", "16", true, "order_bits", 16}, {"GOSS_GPU_ORDER_BITS", "24", true, "order_bits", 24},
    {"GOSS_GPU_ORDER_BITS", "15", false, "order_bits", 0}, {"GOSS_GPU_ORDER_BITS", "25", false, "order_bits", 0}, {"GOSS_GPU_ORDER_BITS", "", false, "order_bits", 0},
    {"GOSS_GPU_REM32_BITS", "9", true, "rem32_bits_min", 9}, {"GOSS_GPU_REM32_BITS", "10", true, "rem32_bits_min", 10},
    {"GOSS_GPU_REM32_BITS", "8", false, "rem32_bits_min", 0}, {"GOSS_GPU_REM32_BITS", "11", false, "rem32_bits_min", 0}, {"GOSS_GPU_REM32_BITS", "", false, "rem32_bits_min", 0},
    {"GOSS_GPU_REM32_SPLIT", "4", true, "rem32_split_min", 4}, {"GOSS_GPU_REM32_SPLIT", "1", true, "rem32_split_min", 1},
    {"GOSS_GPU_REM32_SPLIT", "5", false, "rem32_split_min", 0}, {"GOSS_GPU_REM32_SPLIT", "-1", false, "rem32_split_min", 0},
    {"GOSS_GPU_NARROW_CAPG", "576", true, "narrow_capg", 576}, {"GOSS_GPU_NARROW_CAPG", "1", true, "narrow_capg", 1},
    {"GOSS_GPU_NARROW_CAPG", "0", false, "narrow_capg", 4294967295.0}, {"GOSS_GPU_NARROW_CAPG", "-5", false, "narrow_capg", 4294967295.0},
    {"GOSS_GPU_NARROW_CAPG", "", false, "narrow_capg", 4294967295.0},
    // one of four values
    {"GOSS_GPU_REM32_SLOTS", "2048", true, "rem32_slots", 2048}, {"GOSS_GPU_REM32_SLOTS", "4096", true, "rem32_slots", 4096},
    {"GOSS_GPU_REM32_SLOTS", "8192", true, "rem32_slots", 8192}, {"GOSS_GPU_REM32_SLOTS", "16384", true, "rem32_slots", 16384},
    {"GOSS_GPU_REM32_SLOTS", "1024", false, "rem32_slots", 0}, {"GOSS_GPU_REM32_SLOTS", "32768", false, "rem32_slots", 0},
    {"GOSS_GPU_REM32_SLOTS", "2049", false, "rem32_slots", 0}, {"GOSS_GPU_REM32_SLOTS", "6144", false, "rem32_slots", 0},
    {"GOSS_GPU_REM32_SLOTS", "", false, "rem32_slots", 0},
    // atoi whatever the text, the empty string too
    {"GOSS_GPU_NARROW", "0", true, "narrow", 0}, {"GOSS_GPU_NARROW", "", true, "narrow", 0}, {"GOSS_GPU_NARROW", "x", true, "narrow", 0}, {"GOSS_GPU_NARROW", "1", true, "narrow", 1},
    {"GOSS_GPU_OVERFLOW_BY_SORT", "0", true, "overflow_by_sort", 0}, {"GOSS_GPU_OVERFLOW_BY_SORT", "", true, "overflow_by_sort", 0},
    {"GOSS_GPU_OVERFLOW_BY_SORT", "-1", true, "overflow_by_sort", 1},
    {"GOSS_GPU_R32_SMALL_MAX", "100", true, "r32_small_max", 100}, {"GOSS_GPU_R32_SMALL_MAX", "", true, "r32_small_max", 0},
    {"GOSS_GPU_R32_SMALL_MAX", "-1", true, "r32_small_max", 4294967295.0},
    // not empty -> a number
    {"GOSS_GPU_BLK_LOG2", "12", true, "blk_log2_max", 12}, {"GOSS_GPU_BLK_LOG2", "", false, "blk_log2_max", 0},
    {"GOSS_GPU_HASH_MERGE_MIN", "12345678901234", true, "hash_merge_min", 12345678901234.0}, {"GOSS_GPU_HASH_MERGE_MIN", "0", true, "hash_merge_min", 0},
    {"GOSS_GPU_HASH_MERGE_MIN", "", false, "hash_merge_min", 1048576},
    {"GOSS_GPU_FUSED_MIN", "4096", true, "fused_min", 4096}, {"GOSS_GPU_FUSED_MIN", "0", true, "fused_min", 0}, {"GOSS_GPU_FUSED_MIN", "", false, "fused_min", 33554432},
    {"GOSS_GPU_FUSED_CAPSCALE", "0.25", true, "fused_capscale", 0.25}, {"GOSS_GPU_FUSED_CAPSCALE", "0", true, "fused_capscale", 0},
    {"GOSS_GPU_FUSED_CAPSCALE", "-1", true, "fused_capscale", -1}, {"GOSS_GPU_FUSED_CAPSCALE", "", false, "fused_capscale", 1},
    // clamped to 0..3
    {"GOSS_GPU_BIG_ROUNDS_MIN", "9", true, "big_rounds_min", 3}, {"GOSS_GPU_BIG_ROUNDS_MIN", "2", true, "big_rounds_min", 2},
    {"GOSS_GPU_BIG_ROUNDS_MIN", "-4", true, "big_rounds_min", 0}, {"GOSS_GPU_BIG_ROUNDS_MIN", "", false, "big_rounds_min", 0},
    // atof > 0
    {"GOSS_GPU_EST_SCALE", "2.5", true, "est_scale", 2.5}, {"GOSS_GPU_EST_SCALE", "0", false, "est_scale", 1}, {"GOSS_GPU_EST_SCALE", "-1", false, "est_scale", 1},
    {"GOSS_GPU_EST_SCALE", "", false, "est_scale", 1}, {"GOSS_GPU_EST_SCALE", "x", false, "est_scale", 1},
};

// goss_gpu_stat's names and the fields they read, by hand
#define STAT_FIELDS(X)                                                                                                   \
    X("fused_chunks", fused_chunks) X("rep_chunks", rep_chunks) X("canon_chunks", canon_chunks) X("rec_chunks", rec_chunks) \
    X("flush_wait_us", flush_wait_us) X("flush_count_us", flush_count_us) X("flushes", flushes)                          \
    X("fused_overflows", fused_overflows) X("fused_msd_chunks", fused_msd_chunks) X("rem32_chunks", rem32_chunks)        \
    X("narrow_chunks", narrow_chunks) X("overflow_units", overflow_units) X("packed_fused_chunks", pk_fused_chunks)      \
    X("ds_blocks_from_ranges", ds_blocks_ranges) X("assemble_us", assemble_us) X("ds_blocks_assembled", ds_blocks_own)   \
    X("packed_unpacked_chunks", pk_unpacked_chunks) X("rem32_bits", rem32_bits_last) X("rem32_split", rem32_split_last)  \
    X("big_table_chunks", big_table_chunks) X("wide_table_chunks", wide_table_chunks) X("table96_chunks", table96_chunks) \
    X("valid_sized_chunks", valid_sized_chunks) X("valid_resizes", valid_resizes) X("seg_merges", seg_merges)            \
    X("hash_merges", hash_merges) X("segment_retries", segment_retries) X("lookback_failures", lookback_failures)        \
    X("arena_ms", arena_ms) X("arena_grows", arena_grows)

static void clean_env()
{
    size_t n = 0;
    const KnobRow* rows = knob_table(&n);
    for (size_t j = 0; j < n; ++j) unsetenv(rows[j].name);
}

int main()
{
    // 1. a clean environment gives the defaults
    {
        clean_env();
        check_defaults(Knobs());
        check_defaults(knobs_from_env());
        CHECK(snap(knobs_from_env()) == snap(Knobs()));
        std::printf("ok defaults\n");
    }

    // 2. every variable: what is taken lands in its field and nowhere else, what is outside the rule changes nothing
    {
        const std::vector<double> def = snap(Knobs());
        size_t nrows = 0;
        const KnobRow* rows = knob_table(&nrows);
        CHECK(nrows == kKnobs);                     // one variable per field
        std::vector<int> taken(nrows, 0), refused(nrows, 0);
        for (const Case& cs : kCases)
        {
            size_t row = nrows, field = kKnobs;
            for (size_t j = 0; j < nrows; ++j) if (std::strcmp(rows[j].name, cs.var) == 0) row = j;
            for (size_t j = 0; j < kKnobs; ++j) if (std::strcmp(kKnobNames[j], cs.field) == 0) field = j;
            CHECK(row < nrows && field < kKnobs);
            if (row == nrows || field == kKnobs) { std::printf("  (no row or field for %s / %s)\n", cs.var, cs.field); continue; }
            clean_env();
            setenv(cs.var, cs.text, 1);
            const std::vector<double> got = snap(knobs_from_env());
            std::vector<double> want = def;
            want[field] = cs.value;
            if (!cs.taken) CHECK(cs.value == def[field]);          // (a case that is written wrongly)
            if (got != want) std::printf("  %s='%s': field %s reads %.17g, expected %.17g\n", cs.var, cs.text, cs.field, got[field], want[field]);
            CHECK(got == want);
            (cs.taken ? taken : refused)[row]++;
        }
        clean_env();
        for (size_t j = 0; j < nrows; ++j)
        {
            if (!taken[j]) std::printf("  no accepted case for %s\n", rows[j].name);
            CHECK(taken[j] > 0);
            // (three variables are taken whatever their text: NARROW, OVERFLOW_BY_SORT, R32_SMALL_MAX)
            const std::string name = rows[j].name;
            const bool always = name == "GOSS_GPU_NARROW" || name == "GOSS_GPU_OVERFLOW_BY_SORT" || name == "GOSS_GPU_R32_SMALL_MAX";
            CHECK(always || refused[j] > 0);
        }
        // two variables at once do not disturb each other
        setenv("GOSS_GPU_NO_FUSED", "2", 1);
        setenv("GOSS_GPU_NO_REM32", "2", 1);
        setenv("GOSS_GPU_BIG_ROUNDS_MIN", "9", 1);
        const Knobs k = knobs_from_env();
        CHECK(k.fused && !k.rem32 && k.big_rounds_min == 3);
        clean_env();
        std::printf("ok knobs\n");
    }

    // 3. the counters by name
    {
        size_t nrows = 0;
        stat_table(&nrows);
        Stats s;
        uint64_t next = 1000;
        std::vector<std::pair<const char*, uint64_t>> want;
#define X(name, f) s.f = next; want.push_back({name, next}); next += 7;
        STAT_FIELDS(X)
#undef X
        CHECK(want.size() == 30 && nrows == want.size());
        CHECK(sizeof(Stats) == want.size() * sizeof(uint64_t));          // no field without a name
        for (auto& w : want)
        {
            uint64_t v = ~0ULL;
            CHECK(stat_lookup(s, w.first, &v));
            if (v != w.second) std::printf("  %s reads %llu, expected %llu\n", w.first, (unsigned long long)v, (unsigned long long)w.second);
            CHECK(v == w.second);
        }
        uint64_t v = 42;
        for (const char* no : {"runs", "arena_bytes", "", "fused_chunk", "fused_chunks ", "pk_fused_chunks", "ds_blocks_own", "rem32_bits_last"})
            CHECK(!stat_lookup(s, no, &v) && v == 42);
        std::printf("ok stats\n");
    }

    // 4. Scoped
    {
        static_assert(!std::is_copy_constructible<Scoped<bool>>::value && !std::is_copy_assignable<Scoped<bool>>::value, "Scoped is not copyable");
        bool flag = false;
        { Scoped<bool> a(&flag, true); CHECK(flag); }
        CHECK(!flag);
        flag = true;                                // what was found is put back, not a constant
        { Scoped<bool> a(&flag, true); CHECK(flag); }
        CHECK(flag);
        uint64_t n = 5;
        try
        {
            Scoped<uint64_t> a(&n, n + 10);
            CHECK(n == 15);
            throw std::runtime_error("out of memory");
        }
        catch (const std::runtime_error&) { CHECK(n == 5); }
        double f = 1.0;
        {
            Scoped<double> a(&f, 0.5);
            f = 0.25;                               // (assigned inside the stretch: still the outer value afterwards)
            {
                Scoped<double> b(&f, 0.125);
                CHECK(f == 0.125);
                try { Scoped<double> c(&f, 2.0); CHECK(f == 2.0); throw 1; } catch (int) { CHECK(f == 0.125); }
            }
            CHECK(f == 0.25);
        }
        CHECK(f == 1.0);
        bool lb = true, mute = false;
        { Scoped<bool> p(&lb, false), m(&mute, true); CHECK(!lb && mute); }
        CHECK(lb && !mute);
        std::printf("ok scoped\n");
    }

    if (failures) std::printf("FAILED: %d check(s)\n", failures);
    return failures ? 1 : 0;
}
