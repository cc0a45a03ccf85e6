// goss_ctx.hpp -- the context behind the C ABI (goss_gpu_ctx) and what every path needs of it: the HIP error type, the
// arena's mapping and growth, the phase timer and guarded(), the frame of every entry point.  Included by goss_gpu.hip
// ahead of the *_path.hpp files; the knobs, the counters and Scoped are goss_knobs.hpp's, the arena itself, its scope
// and StatusError goss_arena.hpp's.
#pragma once

namespace {

struct HipError { hipError_t e; const char* what; };

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) throw HipError{_e, #expr};                      \
    } while (0)

struct OutFile {
    std::string suffix;
    uint64_t size = 0;
    const uint8_t* dev = nullptr;      // device-resident image, or
    std::vector<uint8_t> host;         // host-built bytes
};

// version words of the two objects' headers (KmerSet.hh, Graph.hh): written by emit_path.hpp, named in the text dump's
// heading, checked by object_path.hpp
constexpr uint64_t kKmerSetVersion = 2011101701ULL, kGraphVersion = 2011101014ULL;

typedef std::map<std::pair<uint64_t, uint64_t>, uint64_t> BigMap;     // key (hi, lo) -> count that does not fit 32 bits
struct Run { void* keys; uint32_t* counts; uint64_t m; int big = -1; bool rep = false; };
// big: index into ctx.big_maps, or -1.  rep: the keys are strand representatives (extract1_part_kernel), not yet
// gossamer's canonical forms -- runs of ONE space are merged as they are, and the result is canonicalised once

struct PhaseEvents { hipEvent_t a, b; int phase; uint64_t units; };

// What a build entry point left on top of the permanent room for later calls to read (graph_passes.hpp): the segment
// table and text of goss_gpu_segments_build, the images of goss_gpu_entries_build, or the marks, labels and table of the
// components entry points.  One record: at most one is held.
enum class Held : uint8_t { None, Segments, Entries, Components, Pool, Links };
struct HeldResult { Held kind = Held::None; uint64_t lo = 0; };          // lo: the permanent top before the build

// Distinct keys per window from which the fused first level of a one-word k-mer set computes gossamer's canonical form
// itself (Knobs::canon_l1 == 1).
// (0.05: re-ordering M distinct pairs into the canonical order costs 53 ms per 10^9 of them, two FNV hashes per window
// 34 ms per 12.6 G windows -- even at M = 0.051 x windows, and the counting of canonical keys is the faster above that
// (C2 with 0.3 % / 0.5 % errors: 160 -> 148 / 216 -> 170 ms); 0.10 until the end of round 5)
constexpr double kCanonL1At = 0.05;
// At most 2^kBigRoundsMax workgroups share a 16-bit segment counted in the big table.
constexpr int kBigRoundsMax = 2;

// One build's state: what goss_gpu_reset clears, by assigning a new one.  A field belongs here if and only if a second
// build on the same context must not see what the first left in it.
struct Build {
    std::vector<Run> runs;
    std::vector<BigMap> big_maps;       // per run that has them: the counts >= 2^32 - 1 (graph mode; marker 0xFFFFFFFF in the run)
    BigMap res_big;                     // ... of the result (its u32 counts hold the value modulo 2^32, as the reference stores it)
    bool pushed_counts = false;         // a run came in with its counts (goss_gpu_push_run_*): an entry 0xFFFFFFFF of it is that number
    std::vector<OutFile> files;
    uint64_t windows = 0, keys_total = 0;
    int space_choice = -1;              // the key space the build's fused chunks count in once one has chosen: 0 representatives, 1 canonical forms (-1: none yet)
    uint64_t expect_bases = 0;          // goss_gpu_expect_bases: bases the caller means to push in all (0: not said)
    bool finished = false, emitted = false;
    // a group's route-and-exchange round failed half way: what this context had staged may be in records that were
    // lost with the round -- every later push, exchange and finish is refused (GOSS_ERR_STATE) until goss_gpu_reset
    bool broken = false;
    void* res_keys = nullptr;
    uint32_t* res_counts = nullptr;
    uint64_t M = 0;
    void* tips_keys = nullptr;            // result arrays that goss_gpu_prune_tips allocated: the next iteration compacts
    uint32_t* tips_counts = nullptr;      // back into them instead of taking new permanent room
    bool dump_live = false;               // a dump piece's text lies above dump_lo
};

}  // namespace

struct goss_gpu_ctx {
    // ---- identity: fixed by goss_gpu_create ------------------------------------------------------
    int device = 0;
    uint32_t k = 0, len = 0;
    int mode = 0;
    int words = 1;
    Knobs knobs;                        // from the environment, once; a build may demote a form; reset leaves them alone
    Stats stats;                        // behind goss_gpu_stat; cumulative over resets

    // ---- resources: live as long as the context ---------------------------------------------------
    uint64_t budget = 0;
    uint64_t budget_limit = 0;          // the arena may grow up to this many bytes (goss_gpu_set_budget_limit; 0 = fixed)
    Arena arena;
    std::thread arena_thread;           // goss_gpu_prepare: the arena is being mapped in the background
    int arena_status = GOSS_OK;         // ... and how that went
    std::string arena_error;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    ExtractCounters* d_ctr = nullptr;     // device counters
    uint32_t* d_flags = nullptr;          // device error flags [0]=count overflow [1]=ef overflow
    void* d_route = nullptr;              // RouteCounters + the parts' first slots and capacities (goss_gpu_route_records_device)
    void* h_pinned = nullptr;             // pinned scratch (>= 64 bytes)
    uint8_t* grp_send = nullptr;        // goss_gpu_group_route_exchange: this member's routed records (device memory of its own) ...
    uint64_t grp_send_cap = 0;          // ... record slots
    uint8_t* grp_inbox = nullptr;       // ... and what the other members sent it
    uint64_t grp_inbox_cap = 0;
    hipStream_t xstream = nullptr;      // stream of the transfers into this member's inbox
    double grp_count_ms = 0;            // how long the background thread of the last exchange round took to count this member's records
    std::vector<PhaseEvents> events;
    std::vector<hipEvent_t> event_pool;
    goss_gpu_timing timing{};
    float paths_ms[5] = {};               // link, flag, gather, walk, compact of the last trim-paths / clip-links pass
    float relative_ms[3] = {};            // judge, mirror, compact of the last trim-relative pass; lookup, -, compact of the last recount
    std::string last_error;

    // ---- staging: host pushes on their way to a count ---------------------------------------------
    struct Pending { hipEvent_t ev; void (*fn)(void*); void* user; };
    std::vector<Pending> pending;       // asynchronous host pushes whose buffers the caller has not got back yet
    std::vector<hipEvent_t> pend_pool;  // events of `pending` (the counting thread has event_pool to itself)
    // Host pushes are staged in one of TWO buffers (device memory of their own, beside the arena) by copies on a stream of
    // their own; a full buffer is counted by a thread of the library while the caller goes on filling the other
    // A packed staging buffer (round 5): what goss_gpu_push_packed_host* hands over stays 2-bit codes + flags in HBM --
    // u32 of codes per sixteen positions from the buffer's start, u16 of flags per sixteen positions behind them -- and the
    // kernels that read bases take it as it is (load_group16, kernels_common.hpp).  A buffer holds bytes OR packed
    // groups (stage_pk[i]); staged_src makes the ReadSrc (goss_read_src.hpp) of what one holds, and that value -- the
    // two arrays and a position for a packed string -- is what travels from the entry points to the launch sites.
    bool stage_pk[2] = {false, false};
    uint8_t* stage_buf[2] = {nullptr, nullptr};
    int stage_cur = 0;
    uint8_t* stage = nullptr;           // the staging buffer being filled (= stage_buf[stage_cur])
    uint64_t stage_cap = 0, stage_fill = 0;
    hipStream_t copy_stream = nullptr;
    std::thread bg;                     // counts a full staging buffer (one at a time)
    int bg_status = GOSS_OK;
    std::string bg_error;
    bool deferred = false;              // goss_gpu_set_deferred: host pushes only stage; a full staging buffer is reported, not counted
                                        // (the caller then runs goss_gpu_group_route_exchange: the exchange before counting)

    // ---- the build --------------------------------------------------------------------------------
    Build build;                        // what goss_gpu_reset clears
    // ... and what it leaves: the caller's choice for every build of the context, and notes that only the call in
    // progress reads
    int path = 0;                       // 0 auto, 1 LSD sort only
    uint32_t extract_hist_shift = 0xFFFFFFFFu;   // digits histogrammed by the last extraction (or none)
    uint64_t dump_lo = 0;               // permanent top before the current dump piece
    // Arguments that travel through the context: each holds its default between calls, and a Scoped (goss_knobs.hpp)
    // opens every stretch in which one differs (push_source assigns valid_frac inside the stretch it opened)
    bool mute_timing = false;           // set around auxiliary launches (the distinct-count estimate)
    // more of the same input is known to follow the push being counted (a staging buffer that filled up while the caller
    // keeps pushing): its runs will be merged with the runs of the others
    // in representative space and the re-ordering into canonical order paid ONCE, on the merged run -- the chunk's own
    // share of distinct keys then says little about what that costs (C2 from FASTQ: thirteen chunks of 0.8 G windows
    // that each see all 10^8 k-mers of the genome, 12 %, took the canonical form per window -- 67 ms of first level
    // where the representatives take 31, ten second-level bits, and a re-ordering per run)
    bool more_follows = false;
    uint64_t more_starts = 0;           // ... and how many window starts of the push being counted lie behind this chunk (a device push knows)
    double valid_frac = 1.0;            // estimated valid windows per window start of the current push (sizes the key buffers)

    // ---- the held result ---------------------------------------------------------------------------
    // permanent room above everything else from held.lo on, held until its release entry point or the next call that
    // may allocate (guarded() gives it back first; guarded_reading() leaves it).  goss_gpu_segments_build: the segment
    // table and the text (seg_*); goss_gpu_entries_build: the images of the EntryEdgeSet, which are the file list
    HeldResult held;
    void* seg_recs = nullptr;
    uint8_t* seg_text = nullptr;
    uint64_t seg_count = 0, seg_text_bytes = 0;
    // Held::Components, bottom to top: the marks (goss_gpu_components_mark_*; null = none), then from cmp_built_lo on
    // what goss_gpu_components_build left: a component index per edge and the table
    uint32_t* cmp_marks = nullptr;
    uint64_t cmp_mark_words = 0, cmp_built_lo = 0, cmp_marked = 0;      // cmp_marked: bits set in the marks
    uint32_t* cmp_labels = nullptr;
    void* cmp_recs = nullptr;
    uint64_t cmp_count = 0;
    bool cmp_built = false;
    // Held::Pool (pool_path.hpp), bottom to top: the bit rows, the samples' sizes, then from pool_top on the positions
    // and file images of goss_gpu_pool_emit_index
    unsigned long long* pool_rows = nullptr;
    unsigned long long* pool_sizes = nullptr;
    uint64_t pool_z = 0, pool_top = 0;
    uint32_t pool_sets = 0;
    std::vector<bool> pool_added;         // per sample: its row has been written
    // Held::Links (read_links_*, graph_passes.hpp), bottom to top: the segment of every edge, the flag "only edge out
    // of its node", the bucket table of the window lookup, the uniqueness bitmap; then the records batch by batch;
    // then, from lnk_rows_lo on, the table of goss_gpu_read_links_finish (dropped when another batch is added)
    struct LinkChunk { unsigned long long* keys; uint32_t* gaps; uint64_t n; };
    uint32_t* lnk_seg_of = nullptr;
    uint8_t* lnk_single = nullptr;
    uint32_t* lnk_table = nullptr;
    uint32_t* lnk_unique = nullptr;
    uint32_t lnk_bits = 0, lnk_flags = 0;
    uint64_t lnk_entries = 0, lnk_records = 0, lnk_rows_lo = 0, lnk_row_count = 0;
    std::vector<LinkChunk> lnk_chunks;
    void* lnk_rows = nullptr;
    bool lnk_reduced = false;
};

namespace {

// HIP-event timer around the launches of one kernel class (GOSS_T_*).
struct PhaseTimer {
    goss_gpu_ctx* c;
    PhaseEvents pe;
    PhaseTimer(goss_gpu_ctx* ctx, int phase, uint64_t units = 0) : c(ctx)
    {
        muted = c->mute_timing;
        if (muted) return;
        pe.units = units;
        auto get = [&]() {
            hipEvent_t e;
            if (!c->event_pool.empty()) { e = c->event_pool.back(); c->event_pool.pop_back(); }
            else HIP_TRY(hipEventCreate(&e));
            return e;
        };
        pe.a = get(); pe.b = get(); pe.phase = phase;
        HIP_TRY(hipEventRecord(pe.a, c->stream));
    }
    void stop()
    {
        if (muted) return;
        HIP_TRY(hipEventRecord(pe.b, c->stream));
        c->events.push_back(pe);
    }
    bool muted = false;
};

void resolve_timing(goss_gpu_ctx* c)
{
    for (auto& pe : c->events)
    {
        HIP_TRY(hipEventSynchronize(pe.b));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, pe.a, pe.b));
        c->timing.ms[pe.phase] += ms;
        c->timing.launches[pe.phase] += 1;
        c->timing.units[pe.phase] += pe.units;
        c->event_pool.push_back(pe.a);
        c->event_pool.push_back(pe.b);
    }
    c->events.clear();
}

inline uint32_t grid_for(uint64_t n, uint32_t per_block)
{
    uint64_t g = (n + per_block - 1) / per_block;
    if (g == 0) g = 1;
    if (g > 0x7FFFFFFFULL) throw StatusError{GOSS_ERR_INVALID_ARG, "launch grid too large"};
    return (uint32_t)g;
}

void map_arena(goss_gpu_ctx* c)
{
    uint64_t budget = c->budget;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (budget == 0) budget = (uint64_t)((double)free_b * 0.8);
    if (budget > (uint64_t)((double)free_b * 0.92)) budget = (uint64_t)((double)free_b * 0.92);   // a request, not a demand
    void* p = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&p, budget);
    if (e != hipSuccess) throw StatusError{GOSS_ERR_OOM, std::string("hipMalloc(budget) failed: ") + hipGetErrorString(e)};
    c->stats.arena_ms = (uint64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->arena.base = (uint8_t*)p;
    c->arena.size = budget;
    c->arena.lo = 0;
    c->arena.hi = budget;
    c->budget = budget;
}

void ensure_arena(goss_gpu_ctx* c)
{
    if (c->arena_thread.joinable())
    {
        c->arena_thread.join();
        if (c->arena_status != GOSS_OK) throw StatusError{c->arena_status, c->arena_error};
    }
    if (c->arena.base) return;
    map_arena(c);
}

// Grow the arena so that at least `want_avail` bytes are free (or double it when want_avail is 0),
// up to budget_limit (0 = the budget is fixed): a new mapping, the permanent part copied over, every
// pointer into the arena rebased.  Only legal where no temporary is live (start of a chunk, start of a
// merge; the staging buffers of host pushes are memory of their own).  False = not possible.
bool grow_arena(goss_gpu_ctx* c, uint64_t want_avail)
{
    Arena& a = c->arena;
    if (!a.base || c->budget_limit <= a.size) return false;
    const uint64_t top = a.size - a.hi;                    // live temporaries at the top: none where growing is legal
    if (top != 0) return false;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    uint64_t target = std::max<uint64_t>(a.size * 2, a.lo + top + want_avail + (1ULL << 30));
    target = std::min<uint64_t>(target, c->budget_limit);
    target = std::min<uint64_t>(target, (uint64_t)((double)free_b * 0.95));        // the old mapping is still there
    if (target < a.size + (1ULL << 30) || (want_avail && target < a.lo + top + want_avail)) return false;
    void* p = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipMalloc(&p, target) != hipSuccess) { (void)hipGetLastError(); return false; }
    c->stats.arena_ms += (uint64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint8_t* nb = (uint8_t*)p;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (a.lo) HIP_TRY(hipMemcpyAsync(nb, a.base, a.lo, hipMemcpyDeviceToDevice, c->stream));
    if (top) HIP_TRY(hipMemcpyAsync(nb + target - top, a.base + a.hi, top, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    auto rebase = [&](auto*& ptr) {
        if (!ptr) return;
        uint8_t* q = (uint8_t*)ptr;
        if (q >= a.base && q < a.base + a.size) ptr = (std::remove_reference_t<decltype(ptr)>)(nb + (q - a.base));
    };
    for (auto& r : c->build.runs) { rebase(r.keys); rebase(r.counts); }
    rebase(c->build.res_keys); rebase(c->build.res_counts);
    rebase(c->build.tips_keys); rebase(c->build.tips_counts);
    rebase(c->seg_recs); rebase(c->seg_text);
    rebase(c->cmp_marks); rebase(c->cmp_labels); rebase(c->cmp_recs);
    rebase(c->pool_rows); rebase(c->pool_sizes);
    rebase(c->lnk_seg_of); rebase(c->lnk_single); rebase(c->lnk_table); rebase(c->lnk_unique); rebase(c->lnk_rows);
    for (auto& k : c->lnk_chunks) { rebase(k.keys); rebase(k.gaps); }
    for (auto& f : c->build.files) rebase(f.dev);          // file images already emitted (stand-alone SparseArray builds)
    (void)hipFree(a.base);
    a.base = nb; a.hi = target - top; a.size = target;
    c->budget = target;
    c->stats.arena_grows++;
    if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: arena grown to %llu GB\n", (unsigned long long)(target >> 30));
    return true;
}

void wait_background_thread(goss_gpu_ctx* c);
inline void check_launch(const char* what);          // count_path.hpp

// Give back what the context holds (segments, an entry edge set or components), if anything: the permanent room from held.lo on.
void release_held(goss_gpu_ctx* c)
{
    if (c->held.kind != Held::None) c->arena.lo = c->held.lo;
    if (c->held.kind == Held::Entries || c->held.kind == Held::Pool) c->build.files.clear();
    c->held = HeldResult();
    c->pool_rows = nullptr; c->pool_sizes = nullptr; c->pool_z = c->pool_top = 0; c->pool_sets = 0; c->pool_added.clear();
    c->seg_recs = nullptr; c->seg_text = nullptr; c->seg_count = c->seg_text_bytes = 0;
    c->cmp_marks = nullptr; c->cmp_labels = nullptr; c->cmp_recs = nullptr;
    c->cmp_mark_words = c->cmp_built_lo = c->cmp_count = c->cmp_marked = 0;
    c->cmp_built = false;
    c->lnk_seg_of = nullptr; c->lnk_single = nullptr; c->lnk_table = nullptr; c->lnk_unique = nullptr; c->lnk_rows = nullptr;
    c->lnk_bits = c->lnk_flags = 0;
    c->lnk_entries = c->lnk_records = c->lnk_rows_lo = c->lnk_row_count = 0;
    c->lnk_chunks.clear();
    c->lnk_reduced = false;
}

// wait_bg: the call works on the arena or the runs -- the thread that counts a full staging buffer must have ended
// (its failure becomes this call's).  Only the host pushes, which touch nothing but the other staging buffer, go on
// beside it.
// The frame of an entry point that only reads what the context holds, or adds to it: the held result stays.
template <class F>
int guarded_reading(goss_gpu_ctx* c, F&& f, bool wait_bg = true)
{
    try
    {
        if (c) HIP_TRY(hipSetDevice(c->device));
        // forget what the calling thread left behind (e.g. hipErrorNotReady from an event or stream
        // poll of the host process): from here on an error is ours
        (void)hipGetLastError();
        if (c && wait_bg) wait_background_thread(c);
        f();
        // a refused kernel launch raises no exception by itself and leaves its outputs untouched:
        // no entry point returns success over one
        check_launch("a kernel launch was refused");
        return GOSS_OK;
    }
    catch (const HipError& e)
    {
        if (c) c->last_error = std::string(e.what) + ": " + hipGetErrorString(e.e);
        return GOSS_ERR_HIP;
    }
    catch (const StatusError& e)
    {
        if (c) c->last_error = e.msg;
        return e.status;
    }
    catch (const std::bad_alloc&)
    {
        if (c) c->last_error = "host allocation failed";
        return GOSS_ERR_OOM;
    }
    catch (const std::system_error& e)
    {
        // (a thread that could not be started: nothing may cross the C boundary)
        if (c) c->last_error = std::string("a host resource is exhausted: ") + e.what();
        return GOSS_ERR_OOM;
    }
    catch (const std::exception& e)
    {
        if (c) c->last_error = std::string("unexpected failure: ") + e.what();
        return GOSS_ERR_STATE;
    }
}

// The frame of every other entry point.  A held result lies on top of the permanent room: whatever may allocate there,
// or change the result it was read from, gives it back first.
template <class F>
int guarded(goss_gpu_ctx* c, F&& f, bool wait_bg = true)
{
    return guarded_reading(c, [&]() { if (c) release_held(c); f(); }, wait_bg);
}

}  // namespace
