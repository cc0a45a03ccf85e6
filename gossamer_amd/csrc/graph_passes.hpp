// graph_passes.hpp -- the passes over the decoded, sorted edge list of a finished graph: prune-tips, the linear segments
// of print-contigs, the EntryEdgeSet of build-entry-edge-set, count-components, build-subgraph, read links.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, once guarded() and the emit helpers it calls are
// defined).  Two steps are shared and live here once each:
//
//   link_graph   rcr / nxt / info of every edge (kernels_tips.hpp); refuses a graph that lacks a reverse complement
//   rank_lists   starts and predecessors (contigs_mark_kernel), then the position of every edge on its path by a
//                bounded walk and pointer doubling (kernels_contigs.hpp), with or without the multiplicities
//
// prune_tips_once is link_graph and the tip walk; segments_build and entries_build are link_graph, rank_lists and
// their own records; components_build and components_keep are link_graph and a union-find over the links;
// components_grow is link_graph and the passes of build-subgraph over the marks; read_links_begin is link_graph,
// rank_lists and the segment of every edge, read_links_batch and read_links_finish the scans and the sort over it.  What a build leaves behind for
// later calls is the context's one held result (build_held).  trim_relative and recount_from (kernels_relative.hpp)
// need no links: a judge or lookup pass over the edges, the bucket table alone where mirror images are looked up,
// and the compaction of prune-tips.
#pragma once

struct EventPair {
    hipEvent_t e[5] = {};
    EventPair() { for (auto& x : e) HIP_TRY(hipEventCreate(&x)); }
    ~EventPair() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
};

// The pinned scratch of the context as the passes use it: a report at its start, two words behind it.
static_assert(sizeof(TipsReport) <= 128 && sizeof(ContigsReport) <= 128 && sizeof(CompReport) <= 128, "pinned scratch");
template <class R> R* pinned_report(goss_gpu_ctx* c) { return (R*)c->h_pinned; }
inline uint64_t* pinned_words(goss_gpu_ctx* c) { return (uint64_t*)((uint8_t*)c->h_pinned + 128); }

inline void sync_checked(goss_gpu_ctx* c)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    check_launch("a kernel launch was refused");
}

struct NothingQueued { template <class... A> void operator()(A&&...) const {} };

// ---- the state the passes ask for, and the one held result ---------------------------------------------------------

// A graph, between finish and emit, every multiplicity below 2^32 - 1: GOSS_OK, or the status to refuse with
// (last_error is set; the first two texts are the caller's own, `who` heads the third).
int graph_pass_state(goss_gpu_ctx* c, const char* who, const char* not_a_graph, const char* out_of_place)
{
    if (c->mode != GOSS_MODE_GRAPH) { c->last_error = not_a_graph; return GOSS_ERR_STATE; }
    if (!c->build.finished || c->build.emitted) { c->last_error = out_of_place; return GOSS_ERR_STATE; }
    if (!c->build.res_big.empty())
    {
        c->last_error = std::string(who) + ": the graph has multiplicities of 2^32 - 1 or more";
        return GOSS_ERR_INVALID_ARG;
    }
    return GOSS_OK;
}

// The skeleton of goss_gpu_segments_build, goss_gpu_entries_build and the components entry points: guarded() gives
// back what an earlier build holds, `body` builds on top of the permanent room as it is then, and the context holds
// the outcome as `kind`.
// After a failure nothing is held and *out is zero; the result was only read.
// `extend`: what is held is of this kind already and stays (the marks of count-components): body goes on from it.
template <class Info, class F>
int build_held(goss_gpu_ctx* c, Held kind, Info* out, F&& body, bool extend = false)
{
    bool began = false;
    auto build = [&]() {
        if (!extend) c->held = {kind, c->arena.lo};
        began = true;
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        body();
        t.stop();
    };
    const int rc = extend ? guarded_reading(c, build) : guarded(c, build);
    if (rc != GOSS_OK)
    {
        if (began) release_held(c);
        std::memset(out, 0, sizeof *out);
    }
    return rc;
}

// ---- the link pass --------------------------------------------------------------------------------------------------

// Bits of the link pass's bucket table for n edges of len bases: about one edge per bucket, at most 2^26 entries
// (256 MB).  GOSS_GPU_TIPS_BUCKET_BITS overrides it (0 = plain binary search; the probe's A/B).
uint32_t tips_bucket_bits(uint64_t n, uint32_t len)
{
    uint32_t bits = 0;
    while (bits < 26u && (2ULL << bits) <= n) ++bits;
    if (const char* e = std::getenv("GOSS_GPU_TIPS_BUCKET_BITS")) bits = (uint32_t)std::min<long>(26, std::max<long>(0, std::atol(e)));
    return std::min(bits, 2u * len);
}

// The edges of the result as the 32-bit number the link arrays rank them by, or the refusal.
uint32_t link_edges(const goss_gpu_ctx* c, const char* who)
{
    if (c->build.M >= 0xFFFFFFFFULL)
        throw StatusError{GOSS_ERR_INVALID_ARG, std::string(who) + ": the link arrays hold 32-bit ranks; this graph has 2^32 - 1 edges or more"};
    return (uint32_t)c->build.M;
}

inline uint64_t link_table_bytes(uint32_t bits) { return bits ? ((1ULL << bits) + 1) * 4 : 0; }

// What link_graph takes from the arena: rcr, nxt (4 + 4), info (1) and the bucket table.
uint64_t link_bytes(const goss_gpu_ctx* c, const char* who)
{
    const uint64_t n = link_edges(c, who);
    return n * (4 + 4 + 1) + link_table_bytes(n ? tips_bucket_bits(n, c->len) : 0);
}

template <class K>
struct GraphLinks {
    const K* keys;
    const uint32_t* counts;
    uint32_t *rcr, *nxt;              // rank of the reverse complement; of the first edge that leaves to(E[i])
    uint8_t* info;                    // out-degree of to(E[i]) and the size of the group E[i] lies in (kernels_tips.hpp)
    uint32_t n, bits;
    const uint32_t* table;            // the bucket table of the lookups (null when bits == 0): a temporary like the arrays
    dim3 grid, block;                 // one thread per edge
};

// The link pass over the result's n >= 1 edges, complete when this returns: an edge whose reverse complement is
// missing refuses the call.  `who` heads the messages.  `report` is the caller's device report where the kernels
// that follow add to it (it is cleared here), or null for a private one; `before_wait(links)` queues what the caller
// wants on the stream ahead of the wait.
template <class K, class F = NothingQueued>
GraphLinks<K> link_graph(goss_gpu_ctx* c, const char* who, TipsReport* report = nullptr, F&& before_wait = F())
{
    GraphLinks<K> l{};
    l.keys = (const K*)c->build.res_keys;
    l.counts = c->build.res_counts;
    l.n = link_edges(c, who);
    l.bits = tips_bucket_bits(l.n, c->len);
    const uint64_t n64 = l.n;
    l.rcr = (uint32_t*)c->arena.temp(n64 * 4);
    l.nxt = (uint32_t*)c->arena.temp(n64 * 4);
    l.info = (uint8_t*)c->arena.temp(n64);
    uint32_t* table = l.bits ? (uint32_t*)c->arena.temp(link_table_bytes(l.bits)) : nullptr;
    l.table = table;
    if (!report) report = (TipsReport*)c->arena.temp(sizeof(TipsReport));
    l.grid = dim3(grid_for(n64, kTB));
    l.block = dim3(kTB);

    HIP_TRY(hipMemsetAsync(report, 0, sizeof(TipsReport), c->stream));
    HIP_TRY(hipMemsetAsync(&report->missing_rc, 0xFF, 8, c->stream));
    if (l.bits)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tips_table_kernel<K>), l.grid, l.block, 0, c->stream, l.keys, l.n, c->len, l.bits, table);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tips_link_kernel<K>), l.grid, l.block, 0, c->stream, l.keys, l.n, c->len, l.bits,
                       (const uint32_t*)table, l.rcr, l.nxt, l.info, report);
    uint64_t* missing = pinned_words(c);
    HIP_TRY(hipMemcpyAsync(missing, &report->missing_rc, 8, hipMemcpyDeviceToHost, c->stream));
    before_wait(l);
    sync_checked(c);
    if (*missing != ~0ULL)
        throw StatusError{GOSS_ERR_INVALID_ARG, std::string(who) + ": edge " + std::to_string(*missing) +
                                                    " has no reverse complement in the graph (lint-graph reports such edges)"};
    return l;
}

// ---- list ranking ---------------------------------------------------------------------------------------------------

// Pointers the first ranking launch follows per lane before doubling takes over: kContigsWalkSteps, or
// GOSS_GPU_CONTIGS_WALK=<steps> (1 = doubling alone; the probe's A/B).
uint32_t contigs_walk_steps()
{
    long v = kContigsWalkSteps;
    if (const char* e = std::getenv("GOSS_GPU_CONTIGS_WALK")) v = std::atol(e);
    return (uint32_t)std::min<long>(4096, std::max<long>(1, v));
}

// What rank_lists takes from the arena per edge: flag, st (1 + 1), pred (4), two arrays of pairs (8 + 8) and, with the
// multiplicities, two of weights (8 + 8).
constexpr uint64_t rank_bytes_per_edge(bool weighted) { return 1 + 1 + 4 + 8 + 8 + (weighted ? 8 + 8 : 0); }

struct ListRanks {
    uint8_t *flag, *st;               // kCtgStart / kCtgSucc per edge; what is resolved (kCtgOpen = on a cycle without a start)
    uint32_t* pred;
    uint2 *cur, *oth;                 // (start, distance) of every resolved edge; the pairs of the round before the last
    uint64_t *wcur, *woth;            // the weights beside them, or null
    ContigsReport* report;            // on the device: open and resolved so far; the callers' kernels add their figures
    uint32_t steps, rounds;
    dim3 few;                         // the grid of the kernels that stride over the edges
};

// Starts, predecessors and list ranking over the links.  `counts` makes the ranking carry the multiplicities
// (kernels_contigs.hpp, WEIGHTED); null ranks positions alone.  `after_mark(flag)` queues what the caller wants
// between the start flags and the first ranking launch.  Complete when this returns.
template <class K, class F = NothingQueued>
ListRanks rank_lists(goss_gpu_ctx* c, const GraphLinks<K>& l, const uint32_t* counts, F&& after_mark = F())
{
    const uint64_t n64 = l.n;
    const uint32_t n = l.n;
    ListRanks r{};
    r.flag = (uint8_t*)c->arena.temp(n64);
    r.st = (uint8_t*)c->arena.temp(n64);
    r.pred = (uint32_t*)c->arena.temp(n64 * 4);
    r.cur = (uint2*)c->arena.temp(n64 * 8);
    r.oth = (uint2*)c->arena.temp(n64 * 8);
    if (counts)
    {
        r.wcur = (uint64_t*)c->arena.temp(n64 * 8);
        r.woth = (uint64_t*)c->arena.temp(n64 * 8);
    }
    r.report = (ContigsReport*)c->arena.temp(sizeof(ContigsReport));
    r.steps = contigs_walk_steps();
    r.few = dim3((uint32_t)std::min<uint64_t>(grid_for(n64, kTB), kContigsGridBlocks));
    const auto walk = counts ? contigs_walk_kernel<true> : contigs_walk_kernel<false>;
    const auto twice = counts ? contigs_double_kernel<true> : contigs_double_kernel<false>;
    ContigsReport* h = pinned_report<ContigsReport>(c);
    auto fetch_report = [&]() {
        HIP_TRY(hipMemcpyAsync(h, r.report, sizeof(ContigsReport), hipMemcpyDeviceToHost, c->stream));
        sync_checked(c);
    };

    HIP_TRY(hipMemsetAsync(r.report, 0, sizeof(ContigsReport), c->stream));
    HIP_TRY(hipMemsetAsync(r.pred, 0, n64 * 4, c->stream));
    hipLaunchKernelGGL(contigs_mark_kernel, l.grid, l.block, 0, c->stream, (const uint32_t*)l.rcr, (const uint32_t*)l.nxt,
                       (const uint8_t*)l.info, n, r.flag, r.pred);
    after_mark((const uint8_t*)r.flag);
    hipLaunchKernelGGL(walk, r.few, l.block, 0, c->stream, (const uint32_t*)r.pred, (const uint8_t*)r.flag, counts, n, r.steps,
                       r.cur, r.oth, r.wcur, r.woth, r.st, r.report);
    r.rounds = 1;
    fetch_report();
    uint64_t open = h->open, resolved = 0;
    while (open && r.rounds < 64)
    {
        hipLaunchKernelGGL(twice, r.few, l.block, 0, c->stream, (const uint2*)r.cur, r.oth, (const uint8_t*)r.flag, r.st, n, r.report,
                           (const uint64_t*)r.wcur, r.woth);
        std::swap(r.cur, r.oth);
        std::swap(r.wcur, r.woth);
        ++r.rounds;
        fetch_report();
        const uint64_t fresh = h->resolved - resolved;
        resolved = h->resolved;
        if (fresh == 0) break;                          // what is open now lies on cycles without a start
        open -= fresh;
    }
    return r;
}

// ---- prune-tips -----------------------------------------------------------------------------------------------------

// The result becomes its m edges whose bit in the removal bitmap `zap` is clear (tile_offsets: the scanned counts of
// tips_keep_count_kernel).  A result that prune-tips or keep-component allocated is compacted beside itself and
// copied back (five iterations take the permanent room of one); anybody else's arrays (a run, select_counts) are
// left alone and the survivors take new permanent room.  Complete when this returns.
template <class K>
void replace_result(goss_gpu_ctx* c, const K* keys, const uint32_t* counts, uint64_t n64, const uint32_t* zap, const uint64_t* tile_offsets,
                    uint64_t ntiles, uint64_t m)
{
    const uint64_t kb = std::max<uint64_t>(m * sizeof(K), 16), cb = std::max<uint64_t>(m * 4, 16);
    const bool own = c->build.tips_keys && c->build.res_keys == c->build.tips_keys && c->build.res_counts == c->build.tips_counts;
    K* okeys = (K*)(own ? c->arena.temp(kb) : c->arena.perm(kb));
    uint32_t* ocounts = (uint32_t*)(own ? c->arena.temp(cb) : c->arena.perm(cb));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tips_keep_write_kernel<K>), dim3((uint32_t)ntiles), dim3(kTB), 0, c->stream, keys, counts, n64, zap,
                       tile_offsets, okeys, ocounts);
    if (own)
    {
        if (m) HIP_TRY(hipMemcpyAsync(c->build.tips_keys, okeys, m * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        if (m) HIP_TRY(hipMemcpyAsync(c->build.tips_counts, ocounts, m * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    sync_checked(c);
    if (!own) { c->build.tips_keys = okeys; c->build.tips_counts = ocounts; c->build.res_keys = okeys; c->build.res_counts = ocounts; }
    c->build.M = m;
}

// One iteration of prune-tips over the result (GossCmdPruneTips.cc:279-319).  Nothing of the context changes
// before the survivors are complete: a failure leaves the result as it was.
template <class K>
void prune_tips_once(goss_gpu_ctx* c, goss_gpu_tips_report* out)
{
    static_assert(sizeof(goss_gpu_tips_report) == 11 * 8 && sizeof(TipsReport) == 13 * 8, "tips report layout");
    goss_gpu_tips_report rep{};
    const uint64_t n64 = c->build.M;
    rep.edges_before = rep.edges_after = n64;
    if (out) *out = rep;
    if (n64 == 0) return;
    const uint64_t ntiles = (n64 + kRedTile - 1) / kRedTile;
    const uint64_t zap_words = ntiles * (kRedTile / 32), cand_words = (n64 + 63) / 64;
    {
        // the links + the two bitmaps, and the survivors once more while they are compacted
        const uint64_t need = link_bytes(c, "prune_tips") + zap_words * 4 + cand_words * 8 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);       // (no temporary is live between two entry points)
    }
    ArenaScope scope(c->arena);
    uint32_t* zap = (uint32_t*)c->arena.temp(zap_words * 4);
    uint64_t* cand = (uint64_t*)c->arena.temp(cand_words * 8);
    TipsReport* d_rep = (TipsReport*)c->arena.temp(sizeof(TipsReport));
    TipsReport* h = pinned_report<TipsReport>(c);

    HIP_TRY(hipMemsetAsync(zap, 0, zap_words * 4, c->stream));
    const GraphLinks<K> l = link_graph<K>(c, "prune_tips", d_rep, [&](const GraphLinks<K>& q) {
        const dim3 few((uint32_t)std::min<uint64_t>(q.grid.x, kTipsGridBlocks));
        hipLaunchKernelGGL(tips_flag_kernel, few, q.block, 0, c->stream, (const uint32_t*)q.rcr, (const uint8_t*)q.info, q.n, cand, d_rep);
        HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(TipsReport), hipMemcpyDeviceToHost, c->stream));
    });
    const uint32_t n = l.n;
    const dim3 block = l.block;
    const uint64_t ncand = h->candidates;
    rep.candidates = ncand;
    if (ncand == 0) { if (out) *out = rep; return; }

    uint32_t* list = (uint32_t*)c->arena.temp(ncand * 4);
    HIP_TRY(hipMemsetAsync(list, 0xFF, ncand * 4, c->stream));
    const uint64_t words_per_block = (cand_words + kTipsGridBlocks - 1) / kTipsGridBlocks;
    hipLaunchKernelGGL(tips_gather_kernel, dim3(grid_for(cand_words, (uint32_t)std::max<uint64_t>(words_per_block, 1))), block, 0, c->stream,
                       (const uint64_t*)cand, cand_words, words_per_block, list, ncand, d_rep);
    hipLaunchKernelGGL(tips_walk_kernel, dim3(grid_for(ncand, kTB)), block, 0, c->stream, (const uint32_t*)list, ncand, n, c->k,
                       (const uint32_t*)l.rcr, (const uint32_t*)l.nxt, (const uint8_t*)l.info, l.counts, zap, d_rep);
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(tips_keep_count_kernel, dim3((uint32_t)ntiles), block, 0, c->stream, (const uint32_t*)zap, n64, tile_counts);
    uint64_t* hm = pinned_words(c);
    scan_with_total(c, tile_counts, ntiles, hm);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(TipsReport), hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    rep.tips = h->tips; rep.zapped = h->zapped;
    rep.too_long = h->too_long; rep.both_joined = h->both_joined; rep.isolated = h->isolated; rep.outweighed = h->outweighed;
    rep.joined_at_begin = h->joined_at_begin; rep.joined_at_end = h->joined_at_end;
    const uint64_t m = hm[0];
    rep.edges_after = m;
    if (m != n64) replace_result<K>(c, l.keys, l.counts, n64, zap, tile_counts, ntiles, m);
    if (out) *out = rep;
}

void prune_tips(goss_gpu_ctx* c, uint32_t iterations, goss_gpu_tips_report* reports)
{
    for (uint32_t it = 0; it < iterations; ++it)
    {
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        goss_gpu_tips_report* r = reports ? reports + it : nullptr;
        if (c->words == 1) prune_tips_once<Key1>(c, r); else prune_tips_once<Key2>(c, r);
        t.stop();
    }
}

// ---- trim-paths, clip-links -----------------------------------------------------------------------------------------

// What one pass of either command found, as the device report has it (kernels_paths.hpp).
struct PathsOutcome { uint64_t before, after, candidates, hits, edges, too_long, why0, why1; };
constexpr uint64_t kPathsNoEdge = ~0ULL;               // goss_gpu_paths_report::missing_rc of a graph that has them all

// The pass both commands share, in the steps of prune_tips_once: link, flag (`forks`: the starts of clip-links, else
// those of trim-paths and prune-tips), gather, walk under `rule`, compact.  Nothing of the context changes before the
// survivors are complete: a failure leaves the result as it was.  *missing: the edge the link pass refused the graph
// for, where it did.
template <class K, class Rule>
PathsOutcome paths_pass(goss_gpu_ctx* c, const char* who, bool forks, Rule rule, uint64_t* missing)
{
    PathsOutcome o{};
    const uint64_t n64 = c->build.M;
    o.before = o.after = n64;
    if (n64 == 0) return o;
    const uint64_t ntiles = (n64 + kRedTile - 1) / kRedTile;
    const uint64_t zap_words = ntiles * (kRedTile / 32), cand_words = (n64 + 63) / 64;
    {
        // the links, the two bitmaps, the list of starts (every edge can be one), and the survivors once more
        const uint64_t need = link_bytes(c, who) + zap_words * 4 + cand_words * 8 + n64 * 4 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    uint32_t* zap = (uint32_t*)c->arena.temp(zap_words * 4);
    uint64_t* cand = (uint64_t*)c->arena.temp(cand_words * 8);
    PathsReport* d_rep = (PathsReport*)c->arena.temp(sizeof(PathsReport));
    PathsReport* h = pinned_report<PathsReport>(c);

    // the phases of this pass for goss_gpu_paths_timing: link, flag, gather, walk, compact
    EventPair ev, ev_end;
    auto mark = [&](int i) { HIP_TRY(hipEventRecord(i < 5 ? ev.e[i] : ev_end.e[0], c->stream)); };
    auto phases = [&](int done) {
        for (int i = 0; i < 5; ++i)
        {
            c->paths_ms[i] = 0.f;
            if (i < done) HIP_TRY(hipEventElapsedTime(&c->paths_ms[i], ev.e[i], i < 4 ? ev.e[i + 1] : ev_end.e[0]));
        }
    };
    for (float& x : c->paths_ms) x = 0.f;
    mark(0);
    HIP_TRY(hipMemsetAsync(zap, 0, zap_words * 4, c->stream));
    *pinned_words(c) = kPathsNoEdge;
    auto flag_starts = [&](const GraphLinks<K>& q) {
        const dim3 few((uint32_t)std::min<uint64_t>(q.grid.x, kTipsGridBlocks));
        mark(1);
        if (forks) hipLaunchKernelGGL(paths_flag_kernel, few, q.block, 0, c->stream, (const uint8_t*)q.info, q.n, cand, d_rep);
        else hipLaunchKernelGGL(tips_flag_kernel, few, q.block, 0, c->stream, (const uint32_t*)q.rcr, (const uint8_t*)q.info, q.n, cand, (TipsReport*)d_rep);
        mark(2);
        HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(PathsReport), hipMemcpyDeviceToHost, c->stream));
    };
    GraphLinks<K> l{};
    try { l = link_graph<K>(c, who, (TipsReport*)d_rep, flag_starts); }
    catch (...) { *missing = *pinned_words(c); throw; }     // (the edge link_graph refuses the graph for, where that is why)
    const uint32_t n = l.n;
    const dim3 block = l.block;
    const uint64_t ncand = h->candidates;
    o.candidates = ncand;
    if (ncand == 0) { phases(2); return o; }

    uint32_t* list = (uint32_t*)c->arena.temp(ncand * 4);
    HIP_TRY(hipMemsetAsync(list, 0xFF, ncand * 4, c->stream));
    const uint64_t words_per_block = (cand_words + kTipsGridBlocks - 1) / kTipsGridBlocks;
    hipLaunchKernelGGL(tips_gather_kernel, dim3(grid_for(cand_words, (uint32_t)std::max<uint64_t>(words_per_block, 1))), block, 0, c->stream,
                       (const uint64_t*)cand, cand_words, words_per_block, list, ncand, (TipsReport*)d_rep);
    mark(3);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(paths_walk_kernel<Rule>), dim3(grid_for(ncand, kTB)), block, 0, c->stream, (const uint32_t*)list, ncand, n,
                       c->k, (const uint32_t*)l.rcr, (const uint32_t*)l.nxt, (const uint8_t*)l.info, l.counts, zap, d_rep, rule);
    mark(4);
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(tips_keep_count_kernel, dim3((uint32_t)ntiles), block, 0, c->stream, (const uint32_t*)zap, n64, tile_counts);
    uint64_t* hm = pinned_words(c);
    scan_with_total(c, tile_counts, ntiles, hm);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(PathsReport), hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    o.hits = h->hits; o.edges = h->edges; o.too_long = h->too_long; o.why0 = h->why[0]; o.why1 = h->why[1];
    const uint64_t m = hm[0];
    o.after = m;
    if (m != n64) replace_result<K>(c, l.keys, l.counts, n64, zap, tile_counts, ntiles, m);
    mark(5);
    sync_checked(c);
    phases(5);
    return o;
}

// trim-paths over the result (GossCmdTrimPaths.cc:78-248): a path of at most 2K edges from a node without incoming
// edges goes, with the reverse complement of each of its edges.  GOSS_PATHS_CUTOFF spares a path that holds an edge
// of multiplicity >= cutoff (what the reference's visitor was evidently meant to do and never does).
template <class K>
void trim_paths(goss_gpu_ctx* c, uint32_t flags, uint32_t cutoff, goss_gpu_paths_report* out)
{
    static_assert(sizeof(goss_gpu_paths_report) == 8 * 8 && sizeof(PathsReport) == 13 * 8, "paths report layout");
    out->missing_rc = kPathsNoEdge;
    const PathsOutcome o = paths_pass<K>(c, "trim_paths", false, TrimPaths{cutoff, (flags & GOSS_PATHS_CUTOFF) ? 1u : 0u}, &out->missing_rc);
    goss_gpu_paths_report rep{};
    rep.edges_before = o.before; rep.edges_after = o.after; rep.candidates = o.candidates;
    rep.paths = o.hits; rep.zapped = o.edges; rep.too_long = o.too_long; rep.spared_by_cutoff = o.why0;
    rep.missing_rc = kPathsNoEdge;                      // (an edge without its reverse complement refuses the call)
    *out = rep;
}

// clip-links over the result (GossCmdClipLinks.cc:50-174): a path of at most 2K edges that leaves a fork as a minor
// branch and enters a join as a minor branch goes, with the reverse complement of each of its edges.
template <class K>
void clip_links(goss_gpu_ctx* c, goss_gpu_links_report* out)
{
    static_assert(sizeof(goss_gpu_links_report) == 9 * 8, "links report layout");
    out->missing_rc = kPathsNoEdge;
    const PathsOutcome o = paths_pass<K>(c, "clip_links", true, ClipLinks{}, &out->missing_rc);
    goss_gpu_links_report rep{};
    rep.edges_before = o.before; rep.edges_after = o.after; rep.candidates = o.candidates;
    rep.links = o.hits; rep.edges = o.edges; rep.too_long = o.too_long; rep.major_out = o.why0; rep.major_in = o.why1;
    rep.missing_rc = kPathsNoEdge;
    *out = rep;
}

// goss_gpu_trim_paths and goss_gpu_clip_links: the state checks of goss_gpu_prune_tips, one pass, and after a failure
// a report that holds nothing but the edge the graph was refused for.
template <class R, class F>
int paths_entry(goss_gpu_ctx* c, R* out, const char* who, const char* not_a_graph, const char* out_of_place, F&& pass)
{
    std::memset(out, 0, sizeof *out);
    out->missing_rc = GOSS_PATHS_NO_EDGE;
    if (const int st = graph_pass_state(c, who, not_a_graph, out_of_place)) return st;
    const int rc = guarded(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        pass();
        t.stop();
    });
    if (rc != GOSS_OK)
    {
        const uint64_t missing = out->missing_rc;
        std::memset(out, 0, sizeof *out);
        out->missing_rc = missing;
    }
    return rc;
}

// ---- print-contigs --------------------------------------------------------------------------------------------------

// Linear segments of the result (GossCmdPrintContigs.cc:49-193).  Temporaries under an ArenaScope; the table and the
// text are permanent room on top of everything else: the held result.
template <class K>
void segments_build(goss_gpu_ctx* c, uint64_t min_length, uint64_t min_coverage, uint32_t flags, goss_gpu_segments_info* out)
{
    static_assert(sizeof(goss_gpu_segment) == sizeof(SegRec) && sizeof(SegRec) == 64, "segment layout");
    goss_gpu_segments_info inf{};
    const uint64_t n64 = c->build.M;
    if (n64 == 0) { *out = inf; return; }
    const uint32_t Kn = c->k;
    const uint32_t line = (flags & GOSS_SEGMENTS_NO_LINE_BREAKS) ? 0u : 60u;
    {
        // the links, the ranking, the scan (8); then a record per taken path and about half a byte of text per edge
        const uint64_t need = link_bytes(c, "segments") + n64 * (rank_bytes_per_edge(false) + 8) + n64 + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    ContigsReport* h = pinned_report<ContigsReport>(c);
    uint64_t* hx = pinned_words(c);

    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    const GraphLinks<K> l = link_graph<K>(c, "segments", nullptr, [&](const GraphLinks<K>&) { HIP_TRY(hipEventRecord(ev.e[1], c->stream)); });
    const ListRanks r = rank_lists(c, l, nullptr);
    inf.walk_steps = r.steps;
    inf.rounds = r.rounds;
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    const uint32_t n = l.n;
    const dim3 grid = l.grid, block = l.block, few = r.few;

    // ---- ends, the rule per path, the layout of the taken paths
    uint64_t* sc = (uint64_t*)c->arena.temp((n64 + 1) * 8);
    uint32_t* end_of = r.pred;                          // (the predecessors are no longer needed)
    uint32_t* len_of = (uint32_t*)r.oth;                // (nor the pairs of the round before the last)
    uint32_t* ord = len_of + n64;
    hipLaunchKernelGGL(contigs_ends_kernel, few, block, 0, c->stream, (const uint2*)r.cur, (const uint8_t*)r.flag, (const uint8_t*)r.st, n,
                       end_of, len_of, r.report);
    hipLaunchKernelGGL(contigs_decide_kernel, few, block, 0, c->stream, r.flag, (const uint32_t*)l.rcr, (const uint32_t*)end_of,
                       (const uint32_t*)len_of, n, sc, r.report);
    scan_with_total(c, sc, n64, hx);
    HIP_TRY(hipMemcpyAsync(h, r.report, sizeof(ContigsReport), hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    inf.paths = h->paths; inf.taken_paths = h->taken; inf.cycle_edges = h->cycle_edges; inf.longest_path = h->longest;
    const uint64_t npaths = hx[0] >> 32, nslots = hx[0] & 0xFFFFFFFFULL;
    uint64_t nsegs = 0, total = 0;
    SegRec* segs = nullptr;
    uint8_t* text = nullptr;
    if (npaths)
    {
        SegRec* recs = (SegRec*)c->arena.temp(npaths * sizeof(SegRec));
        uint64_t* pass = (uint64_t*)c->arena.temp((npaths + 1) * 8);
        uint64_t* bytes = (uint64_t*)c->arena.temp((npaths + 1) * 8);
        hipLaunchKernelGGL(contigs_paths_kernel, grid, block, 0, c->stream, (const uint8_t*)r.flag, (const uint64_t*)sc,
                           (const uint32_t*)end_of, (const uint32_t*)len_of, n, recs);
        hipLaunchKernelGGL(contigs_order_kernel, grid, block, 0, c->stream, (const uint2*)r.cur, (const uint8_t*)r.flag, (const uint8_t*)r.st,
                           (const uint64_t*)sc, n, ord);
        hipLaunchKernelGGL(contigs_figures_kernel, dim3(grid_for(nslots, kTB * kContigsFigSteps)), block, 0, c->stream,
                           (const uint32_t*)ord, (uint32_t)nslots, l.counts, (const uint2*)r.cur, (const uint64_t*)sc, recs);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(contigs_select_kernel<K>), dim3(grid_for(npaths, kTB)), block, 0, c->stream, l.keys,
                           (const uint32_t*)l.rcr, (const uint8_t*)l.info, recs, npaths, Kn, min_length, min_coverage, line, pass, bytes);
        scan_with_total(c, pass, npaths, hx);
        scan_with_total(c, bytes, npaths, hx + 1);
        HIP_TRY(hipEventRecord(ev.e[3], c->stream));
        sync_checked(c);
        nsegs = hx[0]; total = hx[1];
        if (nsegs)
        {
            segs = (SegRec*)c->arena.perm(nsegs * sizeof(SegRec));
            text = (uint8_t*)c->arena.perm(((total + 15) & ~15ULL) + 16);
            uint32_t* base = (uint32_t*)c->arena.temp(nsegs * 4);
            hipLaunchKernelGGL(contigs_compact_kernel, dim3(grid_for(npaths, kTB)), block, 0, c->stream, (const SegRec*)recs, npaths,
                               (const uint64_t*)pass, (const uint64_t*)bytes, segs, base);
            if (total)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(contigs_text_kernel<K>), dim3(grid_for(total, kTB * kContigsTextRun)), block, 0,
                                   c->stream, l.keys, (const uint32_t*)ord, (const SegRec*)segs, (const uint32_t*)base, nsegs, total, Kn,
                                   line, text);
        }
    }
    else HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    HIP_TRY(hipEventRecord(ev.e[4], c->stream));
    sync_checked(c);
    float* ms[4] = {&inf.ms_link, &inf.ms_rank, &inf.ms_figures, &inf.ms_text};
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    inf.segments = nsegs; inf.text_bytes = total;
    c->seg_recs = segs; c->seg_text = text; c->seg_count = nsegs; c->seg_text_bytes = total;
    *out = inf;
}

void segments_build(goss_gpu_ctx* c, uint64_t min_length, uint64_t min_coverage, uint32_t flags, goss_gpu_segments_info* out)
{
    if (c->words == 1) segments_build<Key1>(c, min_length, min_coverage, flags, out);
    else segments_build<Key2>(c, min_length, min_coverage, flags, out);
}

// ---- build-entry-edge-set -------------------------------------------------------------------------------------------

// The EntryEdgeSet of the result (EntryEdgeSet::build, EntryEdgeSet.cc:154-287).  Working arrays under an ArenaScope;
// the compacted columns and the file images are permanent room on top of everything else (the held result), and the
// images are the context's file list under names that begin with "-entries".
template <class K>
void entries_build(goss_gpu_ctx* c, goss_gpu_entries_info* out)
{
    goss_gpu_entries_info inf{};
    const uint64_t n64 = c->build.M;
    inf.walk_steps = contigs_walk_steps();
    {
        // the links, the ranking with its weights, the scan (8): 55 bytes per edge and the table; then per entry the
        // key, two columns, the images and what the emit kernels sort
        const uint64_t need = link_bytes(c, "entries") + n64 * (rank_bytes_per_edge(true) + 8) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    uint64_t nent = 0;
    K* ekeys = nullptr;
    uint32_t *elen = nullptr, *ecnt = nullptr, *lwr = nullptr;
    uint8_t* upr = nullptr;
    auto columns = [&]() {
        ekeys = (K*)c->arena.perm(std::max<uint64_t>(nent * sizeof(K), 16));
        elen = (uint32_t*)c->arena.perm(std::max<uint64_t>(nent * 4, 16));
        ecnt = (uint32_t*)c->arena.perm(std::max<uint64_t>(nent * 4, 16));
        upr = (uint8_t*)c->arena.perm(std::max<uint64_t>(nent, 16));
        lwr = (uint32_t*)c->arena.perm(std::max<uint64_t>(nent * 4, 16));
    };
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    if (n64 == 0)
    {
        columns();
        for (int i = 1; i < 4; ++i) HIP_TRY(hipEventRecord(ev.e[i], c->stream));
    }
    else
    {
        ContigsReport* h = pinned_report<ContigsReport>(c);
        uint64_t* hx = pinned_words(c);
        const GraphLinks<K> l = link_graph<K>(c, "entries", nullptr, [&](const GraphLinks<K>&) { HIP_TRY(hipEventRecord(ev.e[1], c->stream)); });
        const uint32_t n = l.n;
        // ---- list ranking with the weights; on its way, the numbering of the starts
        uint64_t* sc = (uint64_t*)c->arena.temp((n64 + 1) * 8);
        const ListRanks r = rank_lists(c, l, l.counts, [&](const uint8_t* flag) {
            hipLaunchKernelGGL(entries_flags_kernel, l.grid, l.block, 0, c->stream, flag, n, sc);
            scan_with_total(c, sc, n64, hx);
        });
        nent = hx[0];
        inf.rounds = r.rounds;
        HIP_TRY(hipEventRecord(ev.e[2], c->stream));

        // ---- the records, compacted: every path's last edge writes where the path's start goes
        columns();
        if (nent)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(entries_keys_kernel<K>), l.grid, l.block, 0, c->stream, l.keys, (const uint8_t*)r.flag,
                               (const uint64_t*)sc, n, ekeys);
        hipLaunchKernelGGL(entries_paths_kernel, r.few, l.block, 0, c->stream, (const uint2*)r.cur, (const uint64_t*)r.wcur,
                           (const uint8_t*)r.flag, (const uint8_t*)r.st, (const uint32_t*)l.rcr, l.counts, (const uint64_t*)sc, n, elen, ecnt,
                           upr, lwr, r.report);
        HIP_TRY(hipMemcpyAsync(h, r.report, sizeof(ContigsReport), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(ev.e[3], c->stream));
        sync_checked(c);
        inf.cycle_edges = h->cycle_edges; inf.longest_path = h->longest;
    }
    inf.entries = nent;

    // ---- the images (EntryEdgeSet.cc:203-286): SparseArray::Builder(.edges, z, n) ... end(z) with z = 4^(K+1), two
    // VariableByteArrays of n items, the histogram of the counts, the 40-bit IntegerArray, the header
    const std::string base = "-entries";
    const uint32_t ubits = 2 * c->k + 2;
    const uint64_t zlo = ubits < 64 ? (1ULL << ubits) : 0, zhi = ubits >= 64 ? (1ULL << (ubits - 64)) : 0;
    emit_sparse_array<K>(c, ekeys, nent, zlo, zhi, nent, zlo, zhi, base + ".edges");
    uint64_t lines = 0;
    emit_counts(c, ecnt, nent, nent, base + ".counts", base + ".counts-hist.txt", &lines);
    emit_counts(c, elen, nent, nent, base + ".lengths", std::string());
    inf.hist_size = lines;
    {
        std::vector<IaCol> cols;                          // RankBits = 40 (EntryEdgeSet.hh:41): ".upr" u8, ".lwr" u32
        ia_layout(40, base + ".ends", 0, cols);
        const uint8_t* img[2] = {upr, (const uint8_t*)lwr};
        for (size_t i = 0; i < cols.size() && i < 2; ++i) add_dev_file(c, cols[i].suffix, img[i], nent * cols[i].bytes);
    }
    const uint64_t hdr[2] = {2011041901ULL, c->k};
    add_host_file(c, base + ".header", hdr, sizeof hdr);
    HIP_TRY(hipEventRecord(ev.e[4], c->stream));
    sync_checked(c);
    float* ms[4] = {&inf.ms_link, &inf.ms_rank, &inf.ms_paths, &inf.ms_emit};
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    *out = inf;
}

void entries_build(goss_gpu_ctx* c, goss_gpu_entries_info* out)
{
    c->build.files.clear();
    if (c->words == 1) entries_build<Key1>(c, out); else entries_build<Key2>(c, out);
}

// ---- count-components ---------------------------------------------------------------------------------------------

// The held result of count-components, bottom to top: the marks (a bit per edge, goss_gpu_components_mark_*), then
// what goss_gpu_components_build left -- a label per edge and the table.  The marks outlive the builds that use
// them; a new mark call or build drops the labels and the table above them.
inline void components_drop_built(goss_gpu_ctx* c)
{
    c->arena.lo = c->cmp_built_lo;
    c->cmp_labels = nullptr; c->cmp_recs = nullptr; c->cmp_count = 0; c->cmp_built = false;
}

// Every forward (K+1)-window of the byte-form reads is looked up among the edges and the bits of those found are
// OR-ed into the marks (GossCmdCountComponents.cc:229-241).  The first call takes the zeroed bitmap.
template <class K>
void components_mark(goss_gpu_ctx* c, const void* bases, uint64_t nbytes, bool on_host, goss_gpu_mark_info* out)
{
    goss_gpu_mark_info inf{};
    const uint32_t n = link_edges(c, "components");
    const uint32_t bits = n ? tips_bucket_bits(n, c->len) : 0;
    const uint64_t words = ((uint64_t)n + 63) / 64 * 2;
    {
        // the marks; the reads' copy, the bucket table
        const uint64_t need = (c->cmp_marks ? 0 : words * 4) + (on_host ? nbytes : 0) + link_table_bytes(bits) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    if (c->cmp_marks) components_drop_built(c);
    else
    {
        c->cmp_marks = (uint32_t*)c->arena.perm(std::max<uint64_t>(words * 4, 16));
        c->cmp_mark_words = words;
        c->cmp_built_lo = c->arena.lo;
        HIP_TRY(hipMemsetAsync(c->cmp_marks, 0, std::max<uint64_t>(words * 4, 16), c->stream));
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    const uint8_t* d_bases = (const uint8_t*)bases;
    if (on_host && nbytes)
    {
        uint8_t* d = (uint8_t*)c->arena.temp(nbytes);
        HIP_TRY(hipMemcpyAsync(d, bases, nbytes, hipMemcpyHostToDevice, c->stream));
        d_bases = d;
    }
    uint32_t* table = bits ? (uint32_t*)c->arena.temp(link_table_bytes(bits)) : nullptr;
    CompReport* d_rep = (CompReport*)c->arena.temp(sizeof(CompReport));
    CompReport* h = pinned_report<CompReport>(c);
    const K* keys = (const K*)c->build.res_keys;
    const uint64_t ntiles = (nbytes + kMatchTile - 1) / kMatchTile;
    HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(CompReport), c->stream));
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    if (n && ntiles)
    {
        if (bits)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(tips_table_kernel<K>), dim3(grid_for(n, kTB)), dim3(kTB), 0, c->stream, keys, n, c->len, bits, table);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(components_mark_kernel<K>), unit_grid(ntiles), dim3(kTB), 0, c->stream, keys, n, c->len, bits,
                           (const uint32_t*)table, d_bases, nbytes, ntiles, (uint32_t)(((uintptr_t)d_bases & 7u) == 0), c->cmp_marks, d_rep);
    }
    if (words)
        hipLaunchKernelGGL(components_popcount_kernel, dim3((uint32_t)std::min<uint64_t>(grid_for(words, kTB), kTipsGridBlocks)), dim3(kTB), 0,
                           c->stream, (const uint32_t*)c->cmp_marks, words, d_rep);
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(CompReport), hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    inf.windows = h->windows; inf.hits = h->hits; inf.marked_total = h->marked;
    c->cmp_marked = h->marked;
    HIP_TRY(hipEventElapsedTime(&inf.ms, ev.e[0], ev.e[1]));
    *out = inf;
}

void components_mark(goss_gpu_ctx* c, const void* bases, uint64_t nbytes, bool on_host, goss_gpu_mark_info* out)
{
    if (c->words == 1) components_mark<Key1>(c, bases, nbytes, on_host, out); else components_mark<Key2>(c, bases, nbytes, on_host, out);
}

// parent[i] = the smallest rank of the component of edge i among the marked edges (every edge when marks is null),
// kCompNone where unmarked: three launches over the edges (kernels_components.hpp).  sc as components_flatten_kernel
// takes it.  Queued, not waited for.
template <class K>
uint32_t* components_label(goss_gpu_ctx* c, const GraphLinks<K>& l, const uint32_t* marks, uint64_t* sc, uint32_t* launches)
{
    uint32_t* parent = (uint32_t*)c->arena.temp((uint64_t)l.n * 4);
    hipLaunchKernelGGL(components_init_kernel, l.grid, l.block, 0, c->stream, marks, l.n, parent);
    hipLaunchKernelGGL(components_hook_kernel, l.grid, l.block, 0, c->stream, (const uint32_t*)l.rcr, (const uint32_t*)l.nxt,
                       (const uint8_t*)l.info, marks, l.n, parent);
    hipLaunchKernelGGL(components_flatten_kernel, l.grid, l.block, 0, c->stream, parent, l.n, sc);
    if (launches) *launches = 3;
    return parent;
}

// The components of the marked edges (GossCmdCountComponents.cc:244-258), numbered by ascending smallest rank, with
// their true figures.  Working arrays under an ArenaScope; the labels and the table are permanent room above the marks.
template <class K>
void components_build(goss_gpu_ctx* c, uint32_t flags, goss_gpu_components_info* out)
{
    static_assert(sizeof(goss_gpu_component) == sizeof(CompRec), "component layout");
    goss_gpu_components_info inf{};
    const uint64_t n64 = c->build.M;
    const uint32_t* marks = (flags & GOSS_COMPONENTS_MARKED) ? c->cmp_marks : nullptr;
    c->cmp_built = true;
    if (n64 == 0) { *out = inf; return; }
    {
        // the links, parent (4), the scan (8); the labels (4) and 40 bytes per component stay.  The table is taken
        // once the components are counted, when the arena can no longer grow: its room is asked for here by the
        // only bound there is before the labelling, a component per marked edge
        const uint64_t most = marks ? std::min<uint64_t>(n64, c->cmp_marked) : n64;
        const uint64_t need = link_bytes(c, "components") + n64 * (4 + 8 + 4) + most * sizeof(CompRec) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    uint32_t* labels = (uint32_t*)c->arena.perm(n64 * 4);
    ArenaScope scope(c->arena);
    EventPair ev;
    CompReport* h = pinned_report<CompReport>(c);
    uint64_t* hx = pinned_words(c);

    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    const GraphLinks<K> l = link_graph<K>(c, "components", nullptr, [&](const GraphLinks<K>&) { HIP_TRY(hipEventRecord(ev.e[1], c->stream)); });
    const uint32_t n = l.n;
    uint64_t* sc = (uint64_t*)c->arena.temp((n64 + 1) * 8);
    CompReport* d_rep = (CompReport*)c->arena.temp(sizeof(CompReport));
    HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(CompReport), c->stream));
    const uint32_t* parent = components_label<K>(c, l, marks, sc, &inf.launches);
    scan_with_total(c, sc, n64, hx);
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    sync_checked(c);
    const uint64_t ncomp = hx[0];

    CompRec* recs = (CompRec*)c->arena.perm(std::max<uint64_t>(ncomp * sizeof(CompRec), 16));
    const dim3 few((uint32_t)std::min<uint64_t>(l.grid.x, kTipsGridBlocks));
    hipLaunchKernelGGL(components_number_kernel, l.grid, l.block, 0, c->stream, parent, (const uint64_t*)sc, (const uint32_t*)l.rcr, n, labels, recs);
    hipLaunchKernelGGL(components_figures_kernel, few, l.block, 0, c->stream, (const uint32_t*)labels, l.counts, n, recs);
    if (ncomp)
        hipLaunchKernelGGL(components_largest_kernel, dim3((uint32_t)std::min<uint64_t>(grid_for(ncomp, kTB), kTipsGridBlocks)), l.block, 0, c->stream,
                           (const CompRec*)recs, ncomp, d_rep);
    if (marks)
        hipLaunchKernelGGL(components_popcount_kernel, dim3((uint32_t)std::min<uint64_t>(grid_for(c->cmp_mark_words, kTB), kTipsGridBlocks)), l.block, 0,
                           c->stream, marks, c->cmp_mark_words, d_rep);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(CompReport), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    sync_checked(c);
    inf.components = ncomp;
    inf.marked_edges = marks ? h->marked : n64;
    inf.largest = h->largest;
    float* ms[3] = {&inf.ms_link, &inf.ms_label, &inf.ms_figures};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    c->cmp_labels = labels; c->cmp_recs = recs; c->cmp_count = ncomp;
    *out = inf;
}

void components_build(goss_gpu_ctx* c, uint32_t flags, goss_gpu_components_info* out)
{
    if (c->words == 1) components_build<Key1>(c, flags, out); else components_build<Key2>(c, flags, out);
}

// The result becomes the whole-graph component of edge e and that of rc(e) (what -O writes,
// GossCmdCountComponents.cc:270-309): the labels of every edge, a removal bitmap, the compaction of prune-tips.
// Nothing of the context changes before the survivors are complete.
template <class K>
uint64_t components_keep(goss_gpu_ctx* c, uint32_t e)
{
    const uint64_t n64 = c->build.M;
    const uint64_t ntiles = (n64 + kRedTile - 1) / kRedTile;
    const uint64_t zap_words = ntiles * (kRedTile / 32);
    static_assert(kRedTile % 64 == 0, "a wave writes 64 bits of the bitmap");
    {
        // the links, parent (4), the bitmap, and the survivors once more while they are compacted
        const uint64_t need = link_bytes(c, "components") + n64 * 4 + zap_words * 4 + (ntiles + 1) * 8 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    uint32_t* zap = (uint32_t*)c->arena.temp(zap_words * 4);
    HIP_TRY(hipMemsetAsync(zap, 0, zap_words * 4, c->stream));
    const GraphLinks<K> l = link_graph<K>(c, "components");
    const uint32_t* parent = components_label<K>(c, l, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(components_zap_kernel, l.grid, l.block, 0, c->stream, parent, (const uint32_t*)l.rcr, l.n, e, (uint64_t*)zap);
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(tips_keep_count_kernel, dim3((uint32_t)ntiles), l.block, 0, c->stream, (const uint32_t*)zap, n64, tile_counts);
    uint64_t* hm = pinned_words(c);
    scan_with_total(c, tile_counts, ntiles, hm);
    sync_checked(c);
    const uint64_t m = hm[0];
    if (m != n64) replace_result<K>(c, l.keys, l.counts, n64, zap, tile_counts, ntiles, m);
    return m;
}

uint64_t components_keep(goss_gpu_ctx* c, uint32_t e)
{
    PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
    const uint64_t m = c->words == 1 ? components_keep<Key1>(c, e) : components_keep<Key2>(c, e);
    t.stop();
    return m;
}

// ---- build-subgraph -------------------------------------------------------------------------------------------------

constexpr uint32_t kGrowReadBack = 16;                 // passes queued between two looks at what they added

// The marks become their mirror image's union and grow by `radius` passes (GossCmdBuildSubgraph.cc:95-128, 178-199;
// kernels_subgraph.hpp states what a pass is in either mode).  The passes are queued kGrowReadBack at a time without
// a wait between them; the host then reads what each added and stops once a pass added nothing -- nothing can follow
// an empty frontier -- and the entries of `added` it did not run stay 0.  The frontier, the fringe and, with
// GOSS_GROW_LINEAR_PATHS, the segment labels and their hit flags are working arrays under an ArenaScope; the marks
// stay held, now grown.
template <class K>
void components_grow(goss_gpu_ctx* c, uint32_t radius, uint32_t flags, uint64_t* added, goss_gpu_grow_info* out)
{
    goss_gpu_grow_info inf{};
    const bool linear = (flags & GOSS_GROW_LINEAR_PATHS) != 0;
    const uint64_t n64 = c->build.M, words = c->cmp_mark_words;
    inf.marked_before = inf.mirrored = inf.marked_total = c->cmp_marked;
    if (n64 == 0) { *out = inf; return; }
    {
        // the links, the frontier and the fringe; the segment labels (4) and their hit flags (1)
        const uint64_t need = link_bytes(c, "components_grow") + words * 8 + (linear ? n64 * 5 : 0) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    uint32_t* I = c->cmp_marks;
    uint32_t* P = (uint32_t*)c->arena.temp(words * 4);
    uint32_t* fringe = (uint32_t*)c->arena.temp(words * 4);
    unsigned long long* d_added = (unsigned long long*)c->arena.temp(kGrowReadBack * 8);
    CompReport* d_rep = (CompReport*)c->arena.temp(sizeof(CompReport));
    CompReport* h = pinned_report<CompReport>(c);
    uint64_t* hx = pinned_words(c);
    static_assert(kGrowReadBack * 8 <= 128, "pinned scratch");

    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    const GraphLinks<K> l = link_graph<K>(c, "components_grow", nullptr, [&](const GraphLinks<K>&) { HIP_TRY(hipEventRecord(ev.e[1], c->stream)); });
    const uint32_t n = l.n;
    const dim3 block = l.block;
    const dim3 few((uint32_t)std::min<uint64_t>(grid_for(words, kTB), kTipsGridBlocks));

    uint32_t* label = nullptr;
    uint8_t* hit = nullptr;
    if (linear)
    {
        label = (uint32_t*)c->arena.temp(n64 * 4);
        hit = (uint8_t*)c->arena.temp(n64);
        HIP_TRY(hipMemsetAsync(hit, 0, n64, c->stream));
        hipLaunchKernelGGL(components_init_kernel, l.grid, block, 0, c->stream, (const uint32_t*)nullptr, n, label);
        hipLaunchKernelGGL(subgraph_hook_kernel, l.grid, block, 0, c->stream, (const uint32_t*)l.rcr, (const uint32_t*)l.nxt,
                           (const uint8_t*)l.info, n, label);
        hipLaunchKernelGGL(components_flatten_kernel, l.grid, block, 0, c->stream, label, n, (uint64_t*)nullptr);
        inf.launches += 3;
    }
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));

    HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(CompReport), c->stream));
    HIP_TRY(hipMemsetAsync(fringe, 0, words * 4, c->stream));
    hipLaunchKernelGGL(subgraph_mirror_kernel, l.grid, block, 0, c->stream, (const uint32_t*)l.rcr, n, I);
    hipLaunchKernelGGL(components_popcount_kernel, few, block, 0, c->stream, (const uint32_t*)I, words, d_rep);
    inf.launches += 2;
    HIP_TRY(hipMemcpyAsync(P, I, words * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(CompReport), hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    // from here on the marks are the mirrored ones whatever happens: the count follows them
    inf.mirrored = inf.marked_total = c->cmp_marked = h->marked;

    uint64_t total = inf.mirrored;                         // (once every edge is marked no pass can add)
    for (uint32_t first = 0; first < radius && total < n64; first += kGrowReadBack)
    {
        const uint32_t cnt = std::min(kGrowReadBack, radius - first);
        HIP_TRY(hipMemsetAsync(d_added, 0, kGrowReadBack * 8, c->stream));
        for (uint32_t p = 0; p < cnt; ++p)
        {
            if (linear)
            {
                hipLaunchKernelGGL(subgraph_hit_kernel, few, block, 0, c->stream, (const uint32_t*)P, words, (const uint32_t*)l.rcr,
                                   (const uint32_t*)label, hit);
                hipLaunchKernelGGL(subgraph_cover_kernel, l.grid, block, 0, c->stream, (const uint32_t*)l.rcr, (const uint32_t*)l.nxt,
                                   (const uint8_t*)l.info, (const uint32_t*)label, (const uint8_t*)hit, n, I, fringe);
                hipLaunchKernelGGL(subgraph_settle_kernel<true>, few, block, 0, c->stream, I, P, fringe, words, d_added + p);
                inf.launches += 3;
            }
            else
            {
                hipLaunchKernelGGL(subgraph_push_kernel, few, block, 0, c->stream, (const uint32_t*)P, words, (const uint32_t*)l.rcr,
                                   (const uint32_t*)l.nxt, (const uint8_t*)l.info, (const uint32_t*)I, fringe);
                hipLaunchKernelGGL(subgraph_settle_kernel<false>, few, block, 0, c->stream, I, P, fringe, words, d_added + p);
                inf.launches += 2;
            }
        }
        HIP_TRY(hipMemcpyAsync(hx, d_added, kGrowReadBack * 8, hipMemcpyDeviceToHost, c->stream));
        sync_checked(c);
        inf.passes_run += cnt;
        bool dry = false;
        for (uint32_t p = 0; p < cnt; ++p)
        {
            const uint64_t a = linear ? hx[p] - total : hx[p];     // (linear-path mode counts I itself)
            total += a;
            if (added) added[first + p] = a;
            dry = dry || a == 0;
        }
        c->cmp_marked = inf.marked_total = total;
        if (dry) break;
    }
    HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    sync_checked(c);
    float* ms[3] = {&inf.ms_link, &inf.ms_label, &inf.ms_grow};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    if (!linear) inf.ms_label = 0;                       // (two events with nothing between them)
    *out = inf;
}

void components_grow(goss_gpu_ctx* c, uint32_t radius, uint32_t flags, uint64_t* added, goss_gpu_grow_info* out)
{
    if (c->words == 1) components_grow<Key1>(c, radius, flags, added, out); else components_grow<Key2>(c, radius, flags, added, out);
}

// The result becomes its marked edges (what build-subgraph writes, GossCmdBuildSubgraph.cc:201-209): ~marks as the
// removal bitmap, the compaction of prune-tips.  The bitmap is a temporary; once it is queued the marks -- the held
// result -- are given back, so that the survivors may take the permanent room.  Nothing of the result changes before
// the survivors are complete.
template <class K>
uint64_t components_keep_marked(goss_gpu_ctx* c)
{
    const uint64_t n64 = c->build.M;
    const uint64_t ntiles = (n64 + kRedTile - 1) / kRedTile;
    const uint64_t zap_words = ntiles * (kRedTile / 32);
    {
        // the bitmap, the tile counts, and the survivors once more while they are compacted
        const uint64_t need = zap_words * 4 + (ntiles + 1) * 8 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    if (n64 == 0) { release_held(c); return 0; }
    uint32_t* zap = (uint32_t*)c->arena.temp(zap_words * 4);
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(subgraph_zap_kernel, dim3(grid_for(zap_words, kTB)), dim3(kTB), 0, c->stream, (const uint32_t*)c->cmp_marks,
                       c->cmp_mark_words, n64, zap, zap_words);
    release_held(c);
    hipLaunchKernelGGL(tips_keep_count_kernel, dim3((uint32_t)ntiles), dim3(kTB), 0, c->stream, (const uint32_t*)zap, n64, tile_counts);
    uint64_t* hm = pinned_words(c);
    scan_with_total(c, tile_counts, ntiles, hm);
    sync_checked(c);
    const uint64_t m = hm[0];
    if (m != n64) replace_result<K>(c, (const K*)c->build.res_keys, c->build.res_counts, n64, zap, tile_counts, ntiles, m);
    return m;
}

uint64_t components_keep_marked(goss_gpu_ctx* c)
{
    PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
    const uint64_t m = c->words == 1 ? components_keep_marked<Key1>(c) : components_keep_marked<Key2>(c);
    t.stop();
    return m;
}

// ---- trim-relative, merge-graph-with-reference ----------------------------------------------------------------------

constexpr uint64_t kRelativeNoEdge = ~0ULL;

struct RelativeBitmaps { uint64_t ntiles, zap_words; };
inline RelativeBitmaps relative_bitmaps(uint64_t n64)
{
    static_assert(kRedTile % 64 == 0, "a wave writes 64 bits of the bitmap");
    const uint64_t ntiles = (n64 + kRedTile - 1) / kRedTile;
    return RelativeBitmaps{ntiles, ntiles * (kRedTile / 32)};
}

// The tail both passes share: the survivors of the removal bitmap `zap`, with `counts`, become the result (always when
// `counts` are new ones, else only when an edge goes).  Returns their number.
template <class K>
uint64_t relative_compact(goss_gpu_ctx* c, const uint32_t* counts, const uint32_t* zap, const RelativeBitmaps& b, bool new_counts)
{
    const uint64_t n64 = c->build.M;
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((b.ntiles + 1) * 8);
    hipLaunchKernelGGL(tips_keep_count_kernel, dim3((uint32_t)b.ntiles), dim3(kTB), 0, c->stream, zap, n64, tile_counts);
    uint64_t* hm = pinned_words(c);
    scan_with_total(c, tile_counts, b.ntiles, hm);
    sync_checked(c);
    const uint64_t m = hm[0];
    if (m != n64 || new_counts) replace_result<K>(c, (const K*)c->build.res_keys, counts, n64, zap, tile_counts, b.ntiles, m);
    return m;
}

// trim-relative over the result (TransCmdTrimRelative.cc:81-191; kernels_relative.hpp states what is computed): judge,
// and where an edge is below its node's threshold the bucket table of the link pass, the mirror pass and the
// compaction of prune-tips.  Two bitmaps, the table (about four bytes an edge) and the survivors once more are the
// working room; none of the link arrays is built.  Nothing of the context changes before the survivors are complete.
template <class K>
void trim_relative(goss_gpu_ctx* c, double rel, goss_gpu_relative_report* out)
{
    static_assert(sizeof(goss_gpu_relative_report) == 5 * 8 && sizeof(RelativeReport) <= 128, "relative report layout");
    goss_gpu_relative_report rep{};
    const uint64_t n64 = c->build.M;
    rep.edges_before = rep.edges_after = n64;
    for (float& x : c->relative_ms) x = 0.f;
    if (n64 == 0) { *out = rep; return; }
    const uint32_t n = link_edges(c, "trim_relative");
    const uint32_t bits = tips_bucket_bits(n, c->len);
    const RelativeBitmaps b = relative_bitmaps(n64);
    {
        const uint64_t need = b.zap_words * 8 + link_table_bytes(bits) + (b.ntiles + 1) * 8 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    const K* keys = (const K*)c->build.res_keys;
    uint32_t* below = (uint32_t*)c->arena.temp(b.zap_words * 4);
    uint32_t* zap = (uint32_t*)c->arena.temp(b.zap_words * 4);
    RelativeReport* d_rep = (RelativeReport*)c->arena.temp(sizeof(RelativeReport));
    RelativeReport* h = pinned_report<RelativeReport>(c);
    const dim3 block(kTB), few((uint32_t)std::min<uint64_t>(grid_for(n64, kTB), kTipsGridBlocks));

    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    HIP_TRY(hipMemsetAsync(below, 0, b.zap_words * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(RelativeReport), c->stream));
    HIP_TRY(hipMemsetAsync(&d_rep->bad, 0xFF, 8, c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(relative_judge_kernel<K>), few, block, 0, c->stream, keys, (const uint32_t*)c->build.res_counts, n64, rel, below, d_rep);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(RelativeReport), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    sync_checked(c);
    rep.forks = h->forks;
    rep.below = h->below;
    HIP_TRY(hipEventElapsedTime(&c->relative_ms[0], ev.e[0], ev.e[1]));
    if (rep.below == 0) { *out = rep; return; }

    uint32_t* table = bits ? (uint32_t*)c->arena.temp(link_table_bytes(bits)) : nullptr;
    HIP_TRY(hipMemcpyAsync(zap, below, b.zap_words * 4, hipMemcpyDeviceToDevice, c->stream));
    if (bits)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tips_table_kernel<K>), dim3(grid_for(n64, kTB)), block, 0, c->stream, keys, n, c->len, bits, table);
    const uint64_t nwords = b.zap_words / 2;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(relative_mirror_kernel<K>), dim3((uint32_t)std::min<uint64_t>(grid_for(nwords, kTB), kTipsGridBlocks)), block, 0,
                       c->stream, (const uint64_t*)below, nwords, keys, n, c->len, bits, (const uint32_t*)table, zap, d_rep);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(RelativeReport), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    sync_checked(c);
    if (h->bad != kRelativeNoEdge)
        throw StatusError{GOSS_ERR_INVALID_ARG, "trim_relative: edge " + std::to_string(h->bad) +
                                                    " has no reverse complement in the graph (lint-graph reports such edges)"};
    const uint64_t m = relative_compact<K>(c, c->build.res_counts, zap, b, false);
    HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    sync_checked(c);
    HIP_TRY(hipEventElapsedTime(&c->relative_ms[1], ev.e[1], ev.e[2]));
    HIP_TRY(hipEventElapsedTime(&c->relative_ms[2], ev.e[2], ev.e[3]));
    rep.edges_after = m;
    rep.mirror_only = (n64 - m) - rep.below;
    *out = rep;
}

// merge-graph-with-reference over the result (TransCmdMergeGraphWithReference.cc:79-106): the edges the reference `q`
// holds stay, with its multiplicities.  The new counts (4 bytes an edge), one bitmap and the survivors once more are
// the working room.  Nothing of the context changes before the survivors are complete; the reference is only read.
template <class K>
void recount_from(goss_gpu_ctx* c, const QueryObj& q, goss_gpu_recount_report* out)
{
    goss_gpu_recount_report rep{};
    const uint64_t n64 = c->build.M;
    rep.edges_before = rep.edges_after = n64;
    for (float& x : c->relative_ms) x = 0.f;
    if (n64 == 0) { *out = rep; return; }
    const RelativeBitmaps b = relative_bitmaps(n64);
    {
        const uint64_t need = b.zap_words * 4 + n64 * 4 + (b.ntiles + 1) * 8 + n64 * (sizeof(K) + 4) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    EventPair ev;
    uint32_t* absent = (uint32_t*)c->arena.temp(b.zap_words * 4);
    uint32_t* counts = (uint32_t*)c->arena.temp(n64 * 4);
    RelativeReport* d_rep = (RelativeReport*)c->arena.temp(sizeof(RelativeReport));
    RelativeReport* h = pinned_report<RelativeReport>(c);
    const dim3 block(kTB), few((uint32_t)std::min<uint64_t>(grid_for(n64, kTB), kTipsGridBlocks));

    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    HIP_TRY(hipMemsetAsync(absent, 0, b.zap_words * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_rep, 0xFF, sizeof(RelativeReport), c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(relative_recount_kernel<K>), few, block, 0, c->stream, q, (const K*)c->build.res_keys, n64, counts, absent, d_rep);
    HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(RelativeReport), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    sync_checked(c);
    if (h->bad != kRelativeNoEdge)
        throw StatusError{GOSS_ERR_INVALID_ARG, "recount_from: the reference's index cannot answer for edge " + std::to_string(h->bad) + " (damaged object)"};
    rep.edges_after = relative_compact<K>(c, counts, absent, b, true);
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    sync_checked(c);
    HIP_TRY(hipEventElapsedTime(&c->relative_ms[0], ev.e[0], ev.e[1]));
    HIP_TRY(hipEventElapsedTime(&c->relative_ms[2], ev.e[1], ev.e[2]));
    *out = rep;
}

// ---- read links -------------------------------------------------------------------------------------------------------

// One scan of kernels_links.hpp over n slots, queued: tile aggregates, one workgroup over them, the tiles again.
template <class Op>
void links_scan(goss_gpu_ctx* c, const Op& op, uint64_t n)
{
    if (n == 0) return;
    ArenaScope scope(c->arena);
    const uint32_t ntiles = grid_for(n, kLinkTile);
    uint2* agg = (uint2*)c->arena.temp((uint64_t)ntiles * sizeof(uint2));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(links_scan_reduce_kernel<Op>), dim3(ntiles), dim3(kTB), 0, c->stream, op, n, agg);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(links_scan_tiles_kernel<Op>), dim3(1), dim3(kTB), 0, c->stream, agg, (uint64_t)ntiles);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(links_scan_apply_kernel<Op>), dim3(ntiles), dim3(kTB), 0, c->stream, op, n, (const uint2*)agg);
    // (the stream orders the kernels; the scope may give the aggregates back to later launches on it)
}

// goss_gpu_read_links_begin: link_graph, rank_lists and the numbering of the starts as entries_build has them, then the
// segment of every edge.  Working arrays under an ArenaScope; seg_of, the flags, the bucket table and the bitmap are
// permanent room on top of everything else: the held result.
template <class K>
void read_links_begin(goss_gpu_ctx* c, uint32_t flags, const uint8_t* unique, uint64_t unique_bits, goss_gpu_read_links_info* out)
{
    goss_gpu_read_links_info inf{};
    const uint64_t n64 = c->build.M;
    const uint32_t n = link_edges(c, "read_links");
    const uint32_t bits = n ? tips_bucket_bits(n, c->len) : 0;
    {
        const uint64_t need = link_bytes(c, "read_links") + n64 * (rank_bytes_per_edge(false) + 8) + n64 * 5 + link_table_bytes(bits) +
                              (unique ? unique_bits / 8 + 8 : 0) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    c->lnk_flags = flags;
    c->lnk_bits = bits;
    c->lnk_seg_of = (uint32_t*)c->arena.perm(std::max<uint64_t>(n64 * 4, 16));
    c->lnk_single = (uint8_t*)c->arena.perm(std::max<uint64_t>(n64, 16));
    c->lnk_table = bits ? (uint32_t*)c->arena.perm(link_table_bytes(bits)) : nullptr;
    uint64_t nent = 0;
    inf.edges = n64;
    if (n)
    {
        ArenaScope scope(c->arena);
        EventPair ev;
        LinkReport* d_rep = (LinkReport*)c->arena.temp(sizeof(LinkReport));
        uint64_t* hx = pinned_words(c);
        HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(LinkReport), c->stream));
        HIP_TRY(hipEventRecord(ev.e[0], c->stream));
        const GraphLinks<K> l = link_graph<K>(c, "read_links", nullptr, [&](const GraphLinks<K>&) { HIP_TRY(hipEventRecord(ev.e[1], c->stream)); });
        uint64_t* sc = (uint64_t*)c->arena.temp((n64 + 1) * 8);
        const ListRanks r = rank_lists(c, l, nullptr, [&](const uint8_t* flag) {
            hipLaunchKernelGGL(entries_flags_kernel, l.grid, l.block, 0, c->stream, flag, n, sc);
            scan_with_total(c, sc, n64, hx);
        });
        nent = hx[0];
        HIP_TRY(hipEventRecord(ev.e[2], c->stream));
        if (bits) HIP_TRY(hipMemcpyAsync(c->lnk_table, l.table, link_table_bytes(bits), hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(links_segments_kernel, l.grid, l.block, 0, c->stream, (const uint2*)r.cur, (const uint8_t*)r.st, (const uint64_t*)sc,
                           (const uint8_t*)l.info, n, c->lnk_seg_of, c->lnk_single, d_rep);
        LinkReport* h = pinned_report<LinkReport>(c);
        HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(LinkReport), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(ev.e[3], c->stream));
        sync_checked(c);
        inf.edges_without_segment = h->none;
        float* ms[3] = {&inf.ms_link, &inf.ms_rank, &inf.ms_segments};
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    }
    inf.entries = nent;
    if (nent >= 0x7FFFFFFFULL)
        throw StatusError{GOSS_ERR_INVALID_ARG, "read_links: a window's answer holds a 31-bit segment; this graph has 2^31 - 1 entry edges or more"};
    if (unique && unique_bits != nent)
        throw StatusError{GOSS_ERR_INVALID_ARG, "read_links: the bitmap has " + std::to_string(unique_bits) + " bits; the graph has " +
                                                    std::to_string(nent) + " entry edges"};
    if (unique)
    {
        const uint64_t bytes = (nent + 7) / 8, room = (bytes + 3) / 4 * 4 + 16;
        c->lnk_unique = (uint32_t*)c->arena.perm(room);
        HIP_TRY(hipMemsetAsync(c->lnk_unique, 0, room, c->stream));
        if (bytes) HIP_TRY(hipMemcpyAsync(c->lnk_unique, unique, bytes, hipMemcpyHostToDevice, c->stream));
        sync_checked(c);
    }
    c->lnk_entries = nent;
    *out = inf;
}

// What a batch of n bytes takes from the arena: its copy; win, segu, pa, nh (4 each) and the flags per slot; the
// compacted windows (4) or the records (12); the scans' aggregates.
inline uint64_t read_links_batch_bytes(uint64_t n) { return n * (1 + 4 * 4 + 1 + 12) + (n / kLinkTile + 2) * 8 + (16u << 20); }

// One batch: the windows, the aligner, and either the answers per window (`out`, up to `capacity` of them) or the
// records, which become permanent room on top of what is held.
template <class K>
void read_links_batch(goss_gpu_ctx* c, const void* bases, uint64_t nbytes, uint32_t* out, uint64_t capacity, bool accumulate,
                      goss_gpu_read_links_batch* info)
{
    goss_gpu_read_links_batch inf{};
    if (nbytes >= 0xFFFFFFFEULL) throw StatusError{GOSS_ERR_INVALID_ARG, "read_links: a batch holds fewer than 2^32 - 2 bytes"};
    if (nbytes == 0) { *info = inf; return; }
    if (accumulate && c->lnk_rows_lo)
    {
        // (another batch after a finish: the table goes, the records stay)
        c->arena.lo = c->lnk_rows_lo;
        c->lnk_rows = nullptr; c->lnk_rows_lo = 0; c->lnk_row_count = 0; c->lnk_reduced = false;
    }
    {
        const uint64_t need = read_links_batch_bytes(nbytes);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    const uint32_t n = (uint32_t)c->build.M;
    const bool carry = (c->lnk_flags & GOSS_LINKS_CARRY) != 0;
    ArenaScope scope(c->arena);
    EventPair ev;
    uint8_t* d_bases = (uint8_t*)c->arena.temp(nbytes);
    uint32_t* win = (uint32_t*)c->arena.temp(nbytes * 4);
    uint32_t* segu = (uint32_t*)c->arena.temp(nbytes * 4);
    uint8_t* flags = (uint8_t*)c->arena.temp(nbytes);
    LinkReport* d_rep = (LinkReport*)c->arena.temp(sizeof(LinkReport));
    LinkReport* h = pinned_report<LinkReport>(c);
    static_assert(sizeof(LinkReport) <= 128, "pinned scratch");
    unsigned long long* ctr = &d_rep->carried;          // (the three counters of a scan: carried, hits, records)
    const uint64_t ntiles = (nbytes + kMatchTile - 1) / kMatchTile;

    HIP_TRY(hipMemcpyAsync(d_bases, bases, nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_rep, 0, sizeof(LinkReport), c->stream));
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(links_windows_kernel<K>), unit_grid(ntiles), dim3(kTB), 0, c->stream, (const K*)c->build.res_keys, n, c->len,
                       c->lnk_bits, (const uint32_t*)c->lnk_table, (const uint8_t*)c->lnk_single, (const uint8_t*)d_bases, nbytes, ntiles,
                       (uint32_t)(((uintptr_t)d_bases & 7u) == 0), win, flags, d_rep);
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    if (carry)
    {
        links_scan(c, LinkPrevOp{win, flags, d_bases, c->k, nullptr}, nbytes);
        links_scan(c, LinkCarryOp{win, flags, c->lnk_seg_of, c->lnk_unique, segu, ctr}, nbytes);
    }
    else
        hipLaunchKernelGGL(links_exact_kernel, dim3(grid_for(nbytes, kTB)), dim3(kTB), 0, c->stream, (const uint32_t*)win,
                           (const uint32_t*)c->lnk_seg_of, (const uint32_t*)c->lnk_unique, nbytes, segu);
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));

    uint64_t nrec = 0;
    if (!accumulate)
    {
        uint32_t* packed = (uint32_t*)c->arena.temp(nbytes * 4);
        links_scan(c, LinkPackOp{segu, packed, nullptr}, nbytes);
        HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(LinkReport), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(ev.e[3], c->stream));
        sync_checked(c);
        const uint64_t m = std::min<uint64_t>(h->windows, capacity);
        if (m) HIP_TRY(hipMemcpyAsync(out, packed, m * 4, hipMemcpyDeviceToHost, c->stream));
        sync_checked(c);
    }
    else
    {
        uint32_t* pa = (uint32_t*)c->arena.temp(nbytes * 4);
        uint32_t* nh = (uint32_t*)c->arena.temp(nbytes * 4);
        links_scan(c, LinkHitOp{segu, flags, pa, nh, ctr}, nbytes);
        HIP_TRY(hipMemcpyAsync(h, d_rep, sizeof(LinkReport), hipMemcpyDeviceToHost, c->stream));
        sync_checked(c);
        nrec = h->records;
        if (nrec)
        {
            goss_gpu_ctx::LinkChunk k{};
            k.keys = (unsigned long long*)c->arena.perm(nrec * 8);
            k.gaps = (uint32_t*)c->arena.perm((nrec * 4 + 15) & ~15ULL);
            k.n = nrec;
            links_scan(c, LinkEmitOp{segu, pa, nh, k.keys, k.gaps, nullptr}, nbytes);
            c->lnk_chunks.push_back(k);
            c->lnk_records += nrec;
        }
        HIP_TRY(hipEventRecord(ev.e[3], c->stream));
        sync_checked(c);
    }
    inf.windows = h->windows; inf.misses = h->misses; inf.carried = h->carried; inf.hits = h->hits; inf.records = nrec;
    inf.reads = h->lines + (((const uint8_t*)bases)[nbytes - 1] != '\n' ? 1 : 0);
    float* ms[3] = {&inf.ms_windows, &inf.ms_scans, &inf.ms_compact};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
    *info = inf;
}

// goss_gpu_read_links_finish: the records of every batch side by side, the radix sort of count_path.hpp over the 64-bit
// key with the gaps as values, heads, their scan, and the rows.  The table is permanent room above the records.
void read_links_finish(goss_gpu_ctx* c, goss_gpu_read_links_table_info* out)
{
    goss_gpu_read_links_table_info inf{};
    if (c->lnk_rows_lo) c->arena.lo = c->lnk_rows_lo;
    c->lnk_rows = nullptr; c->lnk_rows_lo = 0; c->lnk_row_count = 0; c->lnk_reduced = false;
    const uint64_t R = c->lnk_records;
    inf.records = R;
    {
        // both arrays twice, the sort's tables, the heads; the rows stay
        const uint64_t need = R * (2 * 12 + 8 + 24) + 256ULL * 8 * (R / 1024 + 2) + (16u << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    const uint64_t rows_lo = c->arena.lo;
    uint64_t nrows = 0;
    LinkRow* rows = nullptr;
    if (R)
    {
        ArenaScope scope(c->arena);
        EventPair ev;
        Key1* ka = (Key1*)c->arena.temp(R * 8);
        Key1* kb = (Key1*)c->arena.temp(R * 8);
        uint32_t* va = (uint32_t*)c->arena.temp(R * 4);
        uint32_t* vb = (uint32_t*)c->arena.temp(R * 4);
        uint64_t* head = (uint64_t*)c->arena.temp((R + 1) * 8);
        uint64_t at = 0;
        for (const auto& k : c->lnk_chunks)
        {
            HIP_TRY(hipMemcpyAsync(ka + at, k.keys, k.n * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(va + at, k.gaps, k.n * 4, hipMemcpyDeviceToDevice, c->stream));
            at += k.n;
        }
        HIP_TRY(hipEventRecord(ev.e[0], c->stream));
        const bool in_b = radix_sort<Key1, true>(c, ka, kb, va, vb, R, 8);
        const unsigned long long* keys = (const unsigned long long*)(in_b ? kb : ka);
        const uint32_t* gaps = in_b ? vb : va;
        HIP_TRY(hipEventRecord(ev.e[1], c->stream));
        hipLaunchKernelGGL(links_heads_kernel, dim3(grid_for(R, kTB)), dim3(kTB), 0, c->stream, keys, R, head);
        nrows = scan_total(c, head, R);
        rows = (LinkRow*)c->arena.perm(nrows * sizeof(LinkRow));
        HIP_TRY(hipMemsetAsync(rows, 0, nrows * sizeof(LinkRow), c->stream));
        hipLaunchKernelGGL(links_rows_kernel, dim3(grid_for(R, kTB)), dim3(kTB), 0, c->stream, keys, gaps, (const uint64_t*)head, R, rows);
        HIP_TRY(hipEventRecord(ev.e[2], c->stream));
        sync_checked(c);
        HIP_TRY(hipEventElapsedTime(&inf.ms_sort, ev.e[0], ev.e[1]));
        HIP_TRY(hipEventElapsedTime(&inf.ms_reduce, ev.e[1], ev.e[2]));
    }
    c->lnk_rows = rows; c->lnk_rows_lo = rows_lo; c->lnk_row_count = nrows; c->lnk_reduced = true;
    inf.rows = nrows;
    *out = inf;
}
