// count_path.hpp -- the plain path from keys to runs, and the merge of runs.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, before fused_path.hpp, which counts through the
// same passes): device scan and radix sort, counts beyond 32 bits, run compaction, the plain extraction kernels' launch,
// the distinct-key estimates, the segment passes (SegStage: segment_reduce, segment_reduce32, count_overflowed_units,
// and the two segment ways of merge_runs), count_keys, and the passes that bring a run of strand representatives
// into the full key space.
#pragma once

// ---- device-wide exclusive scan (in place) -------------------------------------------
void exclusive_scan_u64(goss_gpu_ctx* c, uint64_t* a, uint64_t n)
{
    if (n == 0) return;
    uint64_t nchunks = (n + kScanChunk - 1) / kScanChunk;
    if (nchunks == 1)
    {
        hipLaunchKernelGGL(scan_apply_kernel, dim3(1), dim3(kTB), 0, c->stream, a, n, (const uint64_t*)nullptr);
        return;
    }
    ArenaScope scope(c->arena);
    uint64_t* partial = (uint64_t*)c->arena.temp(nchunks * 8);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(grid_for(n, kScanChunk)), dim3(kTB), 0, c->stream, (const uint64_t*)a, n, partial);
    exclusive_scan_u64(c, partial, nchunks);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(grid_for(n, kScanChunk)), dim3(kTB), 0, c->stream, a, n, (const uint64_t*)partial);
    // the stream orders the kernels; the scratch can be reused by later launches on the
    // same stream once the scope has given it back
}

// a[0, n) becomes its exclusive prefix sums and a[n] their total, which is on its way to *total (pinned) when this
// returns: the caller's next synchronisation delivers it.
inline void scan_with_total(goss_gpu_ctx* c, uint64_t* a, uint64_t n, uint64_t* total)
{
    HIP_TRY(hipMemsetAsync(a + n, 0, 8, c->stream));
    exclusive_scan_u64(c, a, n + 1);
    HIP_TRY(hipMemcpyAsync(total, a + n, 8, hipMemcpyDeviceToHost, c->stream));
}
// ... for the caller that needs the number at once: through the first pinned word, waited for
inline uint64_t scan_total(goss_gpu_ctx* c, uint64_t* a, uint64_t n)
{
    uint64_t* h = (uint64_t*)c->h_pinned;
    scan_with_total(c, a, n, h);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return h[0];
}

// ---- LSD radix sort -------------------------------------------------------------------
// Stable passes on the 8-bit digits at bit first_shift, first_shift+8, ... (ndigits of them).
// Returns true if the result is in (kb, vb).
//
// One pass with per-tile histogram table: histogram kernel, device scan, stable scatter.
template <class K, bool HAS_VAL>
void radix_pass_table(goss_gpu_ctx* c, const K* src, const uint32_t* vs, K* dst, uint32_t* vd, uint64_t n, uint32_t d,
                      uint64_t ntiles, uint64_t* table)
{
    constexpr int tile = SortCfg<K, HAS_VAL>::kTile;
    {
        PhaseTimer t(c, GOSS_T_HIST, n);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_hist_kernel<K, HAS_VAL>), dim3(grid_for(n, tile)), dim3(kTB), 0, c->stream,
                           src, n, d, ntiles, table);
        t.stop();
    }
    {
        PhaseTimer t(c, GOSS_T_SCAN, 256ULL * ntiles);
        exclusive_scan_u64(c, table, 256ULL * ntiles);
        t.stop();
    }
    {
        PhaseTimer t(c, GOSS_T_SCATTER, n);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_scatter_kernel<K, HAS_VAL>), dim3(grid_for(n, tile)), dim3(kTB), 0, c->stream,
                           src, vs, dst, vd, n, d, ntiles, (const uint64_t*)table);
        t.stop();
    }
}

template <class K, bool HAS_VAL>
bool radix_sort(goss_gpu_ctx* c, K* ka, K* kb, uint32_t* va, uint32_t* vb, uint64_t n, uint32_t ndigits,
                uint32_t first_shift = 0, const unsigned long long* prehist = nullptr)
{
    if (n < 2) return false;
    constexpr int tile = SortCfg<K, HAS_VAL>::kTile;
    const uint64_t ntiles = (n + tile - 1) / tile;
    ArenaScope scope(c->arena);
    bool in_b = false;
    // the per-tile table (classic passes) and the look-back status words share one buffer
    uint64_t* table = (uint64_t*)c->arena.temp(256ULL * ntiles * 8);
    unsigned long long* status = (unsigned long long*)table;
    unsigned long long* hist = nullptr;
    unsigned long long* cursors = nullptr;
    LookbackCtl* ctl = nullptr;
    LookbackCtl* hctl = (LookbackCtl*)((uint8_t*)c->h_pinned + 128);
    bool lookback = c->knobs.lookback && ndigits <= 16;
    if (lookback)
    {
        // single-pass form: all digit histograms in one read of the keys, then one look-back
        // scatter per digit
        hist = (unsigned long long*)c->arena.temp(ndigits * 256 * 8);
        ctl = (LookbackCtl*)c->arena.temp(sizeof(LookbackCtl));
        cursors = (unsigned long long*)c->arena.temp(256 * kCursorStride * 8);
        HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(LookbackCtl), c->stream));
        if (prehist)
            HIP_TRY(hipMemcpyAsync(hist, prehist, ndigits * 256 * 8, hipMemcpyDeviceToDevice, c->stream));
        else
        {
            HIP_TRY(hipMemsetAsync(hist, 0, ndigits * 256 * 8, c->stream));
            PhaseTimer t(c, GOSS_T_HIST, n);
            uint32_t grid = (uint32_t)std::min<uint64_t>(2048, (n + kTB - 1) / kTB);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(global_hist_kernel<K>), dim3(grid), dim3(kTB), 0, c->stream,
                               (const K*)ka, n, first_shift, ndigits, hist);
            t.stop();
        }
        {
            PhaseTimer t(c, GOSS_T_SCAN, ndigits * 256);
            hipLaunchKernelGGL(scan_rows256_kernel, dim3(ndigits), dim3(kTB), 0, c->stream, hist);
            t.stop();
        }
    }
    for (uint32_t di = 0; di < ndigits; ++di)
    {
        const uint32_t d = first_shift + 8 * di;       // bit offset of this pass's digit
        K* src = in_b ? kb : ka; K* dst = in_b ? ka : kb;
        uint32_t* vs = in_b ? vb : va; uint32_t* vd = in_b ? va : vb;
        bool done = false;
        if (lookback)
        {
            // pass 0 may place tiles in any order: atomic bucket cursors instead of the chain
            unsigned long long* cur = di == 0 ? cursors : nullptr;
            if (cur) HIP_TRY(hipMemsetAsync(cursors, 0, 256 * kCursorStride * 8, c->stream));
            else HIP_TRY(hipMemsetAsync(status, 0, ntiles * 256 * 8, c->stream));
            {
                PhaseTimer t(c, GOSS_T_SCATTER, n);
                if (c->knobs.ordered_tiles)
                {
                    HIP_TRY(hipMemsetAsync(&ctl->ticket, 0, 4, c->stream));
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_onesweep_kernel<K, HAS_VAL, true>), dim3(grid_for(n, tile)), dim3(kTB), 0,
                                       c->stream, (const K*)src, (const uint32_t*)vs, dst, vd, n, d, first_shift,
                                       (const unsigned long long*)(hist + di * 256), status, ctl, cur);
                }
                else
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_onesweep_kernel<K, HAS_VAL, false>), dim3(grid_for(n, tile)), dim3(kTB), 0,
                                       c->stream, (const K*)src, (const uint32_t*)vs, dst, vd, n, d, first_shift,
                                       (const unsigned long long*)(hist + di * 256), status, ctl, cur);
                t.stop();
            }
            // the source buffer is still intact: a chain that gave up is redone below
            HIP_TRY(hipMemcpyAsync(hctl, ctl, sizeof(LookbackCtl), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
#if defined(GOSS_LB_STATS)
            std::fprintf(stderr, "lookback pass d=%u: tiles=%llu walk_steps=%llu (%.2f/tile) spin_polls=%llu (%.2f/tile) max_depth=%llu\n", d,
                         hctl->tiles, hctl->walk_steps, (double)hctl->walk_steps / (double)(hctl->tiles ? hctl->tiles : 1),
                         hctl->spin_polls, (double)hctl->spin_polls / (double)(hctl->tiles ? hctl->tiles : 1), hctl->max_depth);
            HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(LookbackCtl), c->stream));
#endif
            if (hctl->error)
            {
                std::fprintf(stderr, "libgossgpu: radix look-back chain gave up; redoing the pass with histogram tables\n");
                c->stats.lookback_failures++;
                if (!c->knobs.ordered_tiles) c->knobs.ordered_tiles = true;     // next passes take tickets
                HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(LookbackCtl), c->stream));
            }
            else done = true;
        }
        if (!done) radix_pass_table<K, HAS_VAL>(c, src, vs, dst, vd, n, d, ntiles, table);
        in_b = !in_b;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return in_b;
}

// ---- counts beyond 32 bits (graph mode) ----------------------------------------------------
// After a step that summed counts into `out` (run lengths, run sums, segment merge) and raised the
// overflow flag: the entries of `out` that carry the marker get their exact u64 count from the inputs
// the step read (`keys`/`vals` in `nruns` sorted pieces; vals == nullptr: raw keys, each worth 1) plus
// what the input runs' own big maps hold for the key.  A k-mer set stores no counts: nothing to do.
constexpr uint32_t kMaxBig = 256;
// The entries of a run that carry 0xFFFFFFFF: how many there are, and the place and the key (hi, lo) of the first kMaxBig.
struct Saturated { uint64_t n = 0; std::vector<uint64_t> at; std::vector<std::pair<uint64_t, uint64_t>> key; };
static Saturated find_saturated(goss_gpu_ctx* c, const void* keys, const uint32_t* counts, uint64_t m)
{
    Saturated s;
    ArenaScope scope(c->arena);
    unsigned long long* found = (unsigned long long*)c->arena.temp((kMaxBig + 1) * 8);
    HIP_TRY(hipMemsetAsync(found, 0, 8, c->stream));
    hipLaunchKernelGGL(find_saturated_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m, found, kMaxBig);
    std::vector<unsigned long long> hfound(kMaxBig + 1);
    HIP_TRY(hipMemcpyAsync(hfound.data(), found, (kMaxBig + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    s.n = hfound[0];
    const uint32_t nq = (uint32_t)std::min<unsigned long long>(hfound[0], kMaxBig);
    for (uint32_t q = 0; q < nq; ++q)
    {
        uint64_t kw[2] = {0, 0};
        HIP_TRY(hipMemcpy(kw, (const uint8_t*)keys + hfound[1 + q] * c->words * 8, c->words * 8, hipMemcpyDeviceToHost));
        s.at.push_back(hfound[1 + q]);
        s.key.emplace_back(c->words == 2 ? kw[1] : 0ULL, kw[0]);
    }
    return s;
}

template <class K>
void resolve_big_counts(goss_gpu_ctx* c, Run& out, const K* keys, const uint32_t* vals, const std::vector<uint64_t>& run_off,
                        const std::vector<int>& in_bigs)
{
    if (c->mode != GOSS_MODE_GRAPH || out.m == 0) return;
    uint32_t* hf = (uint32_t*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(hf, c->d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!hf[0]) return;
    ArenaScope scope(c->arena);
    const Saturated sat = find_saturated(c, out.keys, out.counts, out.m);
    if (sat.n > kMaxBig) throw StatusError{GOSS_ERR_COUNT_OVERFLOW, "more than 256 keys occurred 2^32 times or more"};
    const uint32_t nruns = (uint32_t)run_off.size() - 1;
    if (nruns > 1024) throw StatusError{GOSS_ERR_COUNT_OVERFLOW, "a key occurred 2^32 times or more in a merge of more than 1024 runs"};
    const uint32_t nq = (uint32_t)sat.n;
    if (nq)
    {
        std::vector<K> hq(nq);
        for (uint32_t q = 0; q < nq; ++q)
        {
            if constexpr (sizeof(K) == 8) hq[q] = K{sat.key[q].second}; else hq[q] = K{sat.key[q].second, sat.key[q].first};
        }
        K* dq = (K*)c->arena.temp(nq * sizeof(K));
        uint64_t* doff = (uint64_t*)c->arena.temp((nruns + 1) * 8);
        unsigned long long* dsum = (unsigned long long*)c->arena.temp(2 * nq * 8);
        HIP_TRY(hipMemcpyAsync(dq, hq.data(), nq * sizeof(K), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(doff, run_off.data(), (nruns + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(dsum, 0, 2 * nq * 8, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(sum_equal_kernel<K>), dim3(nq), dim3(std::max<uint32_t>(64, (nruns + 63) / 64 * 64)), 0, c->stream,
                           keys, vals, (const uint64_t*)doff, nruns, (const K*)dq, nq, dsum, dsum + nq);
        std::vector<unsigned long long> hs(2 * nq);
        HIP_TRY(hipMemcpyAsync(hs.data(), dsum, 2 * nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        BigMap bm;
        for (uint32_t q = 0; q < nq; ++q)
        {
            const std::pair<uint64_t, uint64_t>& kk = sat.key[q];
            uint64_t exact = hs[q], markers = 0;
            for (int b : in_bigs)
                if (b >= 0)
                {
                    auto it = c->build.big_maps[b].find(kk);
                    if (it != c->build.big_maps[b].end()) { exact += it->second; ++markers; }
                }
            // an entry 0xFFFFFFFF that no input map accounts for came in with a pushed run (goss_gpu_push_run_*: a graph
            // read from disk, a caller's own run), and there it is no marker but the multiplicity 2^32 - 1 itself; where no
            // run was pushed every marker has its map, and one without is a bookkeeping error as before
            if (markers > hs[nq + q] || (!c->build.pushed_counts && markers != hs[nq + q]))
                throw StatusError{GOSS_ERR_HIP, "count bookkeeping: a saturated entry without its exact count"};
            exact += (hs[nq + q] - markers) * 0xFFFFFFFFULL;
            bm[kk] = exact;
        }
        c->build.big_maps.push_back(std::move(bm));
        out.big = (int)c->build.big_maps.size() - 1;
    }
    HIP_TRY(hipMemsetAsync(c->d_flags, 0, 4, c->stream));
}

// A pushed run that reaches the result through no merge (it was the only one): its entries 0xFFFFFFFF are the
// multiplicity 2^32 - 1 itself, and a graph's result lists every count that large beside the run (goss_gpu_big_counts).
template <class K>
void adopt_literal_counts(goss_gpu_ctx* c, Run& r)
{
    if (c->mode != GOSS_MODE_GRAPH || r.m == 0 || r.big >= 0) return;
    const Saturated sat = find_saturated(c, r.keys, r.counts, r.m);
    if (sat.n > kMaxBig) throw StatusError{GOSS_ERR_COUNT_OVERFLOW, "more than 256 keys occurred 2^32 times or more"};
    if (!sat.n) return;
    BigMap bm;
    for (const auto& kk : sat.key) bm[kk] = 0xFFFFFFFFULL;
    c->build.big_maps.push_back(std::move(bm));
    r.big = (int)c->build.big_maps.size() - 1;
}

// ---- run compaction ---------------------------------------------------------------------
// keys sorted (n).  Produces a permanent Run (distinct keys + u32 counts).  If vals != null
// the counts are sums of vals over each run, else run lengths.  `scratch_keys` is a buffer
// of >= n keys that may be clobbered (the free half of the sort ping-pong).
template <class K>
Run reduce_runs(goss_gpu_ctx* c, const K* keys, const uint32_t* vals, uint64_t n, K* scratch_keys, const std::vector<int>* in_bigs = nullptr)
{
    Run r{nullptr, nullptr, 0};
    if (n == 0) return r;
    ArenaScope scope(c->arena);
    const uint64_t ntiles = (n + kRedTile - 1) / kRedTile;
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(heads_count_kernel<K>), dim3(grid_for(n, kRedTile)), dim3(kTB), 0, c->stream,
                       keys, n, tile_counts);
    const uint64_t m = scan_total(c, tile_counts, ntiles);
    uint64_t* starts = (uint64_t*)c->arena.temp(m * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(heads_write_kernel<K>), dim3(grid_for(n, kRedTile)), dim3(kTB), 0, c->stream,
                       keys, n, (const uint64_t*)tile_counts, scratch_keys, starts);
    // permanent storage
    r.m = m;
    r.keys = c->arena.perm(m * sizeof(K));
    r.counts = (uint32_t*)c->arena.perm(m * 4);
    HIP_TRY(hipMemcpyAsync(r.keys, scratch_keys, m * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
    if (vals)
        hipLaunchKernelGGL(run_sums_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                           (const uint64_t*)starts, m, n, vals, r.counts, c->d_flags);
    else
        hipLaunchKernelGGL(run_lengths_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                           (const uint64_t*)starts, m, n, r.counts, c->d_flags);
    HIP_TRY(hipStreamSynchronize(c->stream));   // the temporaries go with the scope
    resolve_big_counts<K>(c, r, keys, vals, std::vector<uint64_t>{0, n}, in_bigs ? *in_bigs : std::vector<int>());
    return r;
}

// ---- packed strings ------------------------------------------------------------------------------------------------
// groups of a packed staging buffer of `cap` positions, and its two arrays
static inline uint64_t pk_groups(uint64_t cap) { return cap / 16 + 4; }
static inline uint32_t* pk_codes_of(uint8_t* buf) { return (uint32_t*)buf; }
static inline uint16_t* pk_bad_of(uint8_t* buf, uint64_t cap) { return (uint16_t*)(buf + pk_groups(cap) * 4); }
// Run-time choices -> template arguments of a kernel: f is called with a std::bool_constant of the value (with int_c<N>
// for the choices the caller makes itself).
template <class F> void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <int N> using int_c = std::integral_constant<int, N>;
// Bytes of `n` positions of the packed string `p`, for the kernels that have no packed form (the plain extraction of
// small inputs and of the fallback sequence -- never the fused path's): unpacked into a temporary of the arena (the
// caller releases its mark).  Returns the byte string over the temporary.
static ReadSrc pk_unpack_temp(goss_gpu_ctx* c, const ReadSrc& p, uint64_t n)
{
    const ReadSrc::Launch in = p.launch();
    const uint64_t groups = (n + in.mis + 15) / 16;
    c->stats.pk_unpacked_chunks++;
    uint8_t* out = (uint8_t*)c->arena.temp((groups + 1) * 16 + 64);
    hipLaunchKernelGGL(unpack_bases_kernel, dim3(grid_for(groups + 1, kTB)), dim3(kTB), 0, c->stream, (const uint32_t*)in.base, in.bad, groups,
                       n + in.mis, out);
    return ReadSrc::of_bytes(out + in.mis);
}

// The plain kernels: extract_dispatch takes bytes or records (a packed string is unpacked first, process_chunk), and
// `rep` says that the keys are strand representatives -- the key space of the fused path, whose sample this then is.
template <class K>
void extract_dispatch(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, K* out, bool rep);
inline void refuse_packed(const ReadSrc& src)
{
    if (src.packed()) throw StatusError{GOSS_ERR_STATE, "a packed string handed to a kernel that reads bytes"};
}
template <class K> bool use_segment_path(const goss_gpu_ctx* c);
template <int MODE, int P, int G>
void launch_extract1(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, Key1* out, bool rep)
{
    refuse_packed(src);
    const ReadSrc::Launch in = src.launch();
    constexpr int T = kTB * P * G;
    const uint64_t nsuper = (nstarts + T - 1) / T;
    // persistent grid: 4 workgroups per CU (LDS-limited), 256 CUs
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nsuper ? nsuper : 1, 1024 * 2);
    // fused digit histograms for the 16-bit partition that follows on the segment path
    c->extract_hist_shift = use_segment_path<Key1>(c) ? 2 * c->len - kSegBits : 0xFFFFFFFFu;
#define GOSS_LAUNCH_E1(NB)                                                                                              \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(extract1_kernel<MODE, P, G, NB>), dim3(grid), dim3(kTB), 0, c->stream, in.base, in.mis, \
                       nstarts, navail, c->len, out, c->d_ctr, c->extract_hist_shift, nsuper)
    if (MODE == 1) { GOSS_LAUNCH_E1(8); return; }          // graph mode does not hash
    if (MODE == 0 && rep)
    {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract1_kernel<MODE, P, G, 8, true>), dim3(grid), dim3(kTB), 0, c->stream, in.base, in.mis,
                           nstarts, navail, c->len, out, c->d_ctr, c->extract_hist_shift, nsuper);
        return;
    }
    switch ((2 * c->len + 7) / 8)
    {
        case 1: GOSS_LAUNCH_E1(1); break;
        case 2: GOSS_LAUNCH_E1(2); break;
        case 3: GOSS_LAUNCH_E1(3); break;
        case 4: GOSS_LAUNCH_E1(4); break;
        case 5: GOSS_LAUNCH_E1(5); break;
        case 6: GOSS_LAUNCH_E1(6); break;
        case 7: GOSS_LAUNCH_E1(7); break;
        default: GOSS_LAUNCH_E1(8); break;
    }
#undef GOSS_LAUNCH_E1
}
// window slots of a record (the most windows one holds): a string of n records counts as 16 n window starts
inline uint32_t rec_slots(const goss_gpu_ctx*) { return (uint32_t)ReadSrc::kRecSlots; }
// bytes of a record: 12 for one-word keys (SkRec), 20 for two-word keys (SkRec2)
inline uint64_t rec_bytes(const goss_gpu_ctx* c) { return c->words == 1 ? sizeof(SkRec) : sizeof(SkRec2); }
inline ReadSrc records_src(const goss_gpu_ctx* c, const void* first) { return ReadSrc::of_records(first, (uint32_t)rec_bytes(c)); }

// records -> keys with the plain kernel: all records (slice_groups = 0) or slices of them (the fused path's sample)
void launch_extract_records(goss_gpu_ctx* c, const SkRec* recs, uint64_t nrecs, Key1* out, uint64_t ngroups, uint64_t slice_groups,
                            uint64_t slice_stride, bool rep)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ngroups, 1), 256 * 16);
    if (c->mode == GOSS_MODE_GRAPH && !rep)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records_kernel<1, false>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out,
                           c->d_ctr, ngroups, slice_groups, slice_stride);
    else if (rep)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records_kernel<0, true>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out,
                           c->d_ctr, ngroups, slice_groups, slice_stride);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records_kernel<0, false>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out,
                           c->d_ctr, ngroups, slice_groups, slice_stride);
}

// the same for two-word records (rep: graph builds counted as strand pairs)
void launch_extract_records2(goss_gpu_ctx* c, const SkRec2* recs, uint64_t nrecs, Key2* out, uint64_t ngroups, uint64_t slice_groups,
                             uint64_t slice_stride, bool rep)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ngroups, 1), 256 * 16);
    if (c->mode == GOSS_MODE_GRAPH && !rep)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records2_kernel<1, false>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out, c->d_ctr, ngroups,
                           slice_groups, slice_stride);
    else if (rep)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records2_kernel<0, true>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out, c->d_ctr, ngroups,
                           slice_groups, slice_stride);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract_records2_kernel<0, false>), dim3(grid), dim3(kTB), 0, c->stream, recs, nrecs, c->len, out, c->d_ctr, ngroups,
                           slice_groups, slice_stride);
}

template <>
void extract_dispatch<Key1>(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, Key1* out, bool rep)
{
    c->extract_hist_shift = 0xFFFFFFFFu;
    if (src.records())
    {
        const uint64_t nrecs = nstarts / rec_slots(c);
        launch_extract_records(c, (const SkRec*)src.bytes, nrecs, out, (nrecs + kRecGroup - 1) / kRecGroup, 0, 0, rep);
        return;
    }
    // (rep in graph mode: one strand representative per window -- the fused path's key space for graphs)
    if (c->mode == GOSS_MODE_KMER_SET || rep) launch_extract1<0, 16, 8>(c, src, nstarts, navail, out, rep);
    else launch_extract1<1, 8, 8>(c, src, nstarts, navail, out, false);
}
// significant bytes of a two-word key's high word, rounded up to the instantiated classes 2/4/6/8
inline int key2_nbh(const goss_gpu_ctx* c) { const int nb = (int)(2 * c->len + 7) / 8 - 8; return nb <= 2 ? 2 : nb <= 4 ? 4 : nb <= 6 ? 6 : 8; }

// (bytes or a packed string -- only the fused path's sample comes here with one: the plain extraction of a whole chunk unpacks first)
template <int MODE, int P, int G>
void launch_extract2(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, Key2* out,
                     uint64_t slice_tiles = 0, uint64_t slice_stride = 0, uint64_t nsuper_override = 0, bool rep = false)
{
    constexpr int T = kTB * P * G;
    const uint64_t nsuper = nsuper_override ? nsuper_override : (nstarts + T - 1) / T;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nsuper ? nsuper : 1, 1024 * 2);
    const ReadSrc::Launch in = src.launch();
    auto launch = [&](auto nbh) {
        with_bool(in.kind == ReadSrc::Packed, [&](auto pk) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(extract2_kernel<MODE, P, G, decltype(nbh)::value, decltype(pk)::value>), dim3(grid), dim3(kTB), 0,
                               c->stream, in.base, in.mis, nstarts, navail, c->len, out, c->d_ctr, nsuper, slice_tiles, slice_stride, in.bad);
        });
    };
    if (MODE == 1) { launch(int_c<8>{}); return; }             // graph mode does not hash
    if (rep) { launch(int_c<0>{}); return; }                   // strand representatives (NBH 0): no hash either
    switch (key2_nbh(c))
    {
        case 2: launch(int_c<2>{}); break;
        case 4: launch(int_c<4>{}); break;
        case 6: launch(int_c<6>{}); break;
        default: launch(int_c<8>{}); break;
    }
}
template <>
void extract_dispatch<Key2>(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, Key2* out, bool rep)
{
    if (src.records())
    {
        // two-word records -> keys with the plain kernel (their counting goes through the unfused sequence)
        const uint64_t nrecs = nstarts / rec_slots(c);
        launch_extract_records2(c, (const SkRec2*)src.bytes, nrecs, out, (nrecs + kRecGroup - 1) / kRecGroup, 0, 0, rep);
        return;
    }
    refuse_packed(src);
    if (c->mode == GOSS_MODE_KMER_SET || rep) launch_extract2<0, 8, 8>(c, src, nstarts, navail, out, 0, 0, 0, rep);
    else launch_extract2<1, 4, 8>(c, src, nstarts, navail, out);
}

inline uint32_t key_digits(const goss_gpu_ctx* c) { return (2 * c->len + 7) / 8; }

// ---- fast path: radix partition on the top bits + per-segment LDS hash table -------------
template <class K> bool use_segment_path(const goss_gpu_ctx* c)
{
    if (c->path == 1) return false;                   // LSD only
    return 2 * c->len >= 24;                          // enough key bits below the partition bits
}
template bool use_segment_path<Key1>(const goss_gpu_ctx*);
template bool use_segment_path<Key2>(const goss_gpu_ctx*);

template <class K> struct SegCfg;
template <> struct SegCfg<Key1> { static constexpr uint64_t kLimit = kSegLimit; };
template <> struct SegCfg<Key2> { static constexpr uint64_t kLimit = kSegLimit2; };

// Grid of `units` workgroups for the kernels that number their workgroup with unit_block(): x up
// to 2^20, the rest in y (units is a power of two above that).  HIP refuses gridDim.x * blockDim.x
// >= 2^32 -- and a refused launch leaves the output counters at zero, which reads as "no keys".
inline dim3 unit_grid(uint64_t units)
{
    const uint64_t kx = 1u << 20;
    if (units <= kx) return dim3((uint32_t)std::max<uint64_t>(units, 1));
    return dim3((uint32_t)kx, (uint32_t)((units + kx - 1) / kx));
}
inline void check_launch(const char* what)
{
    // the thread's error state was cleared when the entry point was entered (guarded): whatever
    // is there now was raised by this library's own calls -- it never polls, so not even
    // hipErrorNotReady is expected
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw StatusError{GOSS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)};
}

// The counting table of segment_reduce.
enum class SegTable {
    Small,               // 4096 slots, one workgroup of 256 threads per segment
    Big,                 // one-word keys: 8192 slots, two-word keys: 4096 slots; 1024 threads, 2^rounds workgroups share a segment
    Wide,                // two-word keys: 6144 slots, one workgroup per segment
    Rem96,               // two-word keys: 8192 slots of 96-bit remainders, one workgroup per segment
    Rem96Packed          // ... fed the 12-byte records of the remainders that the second level wrote
};
struct SegCount { SegTable table = SegTable::Small; uint32_t rounds = 0; };

inline void launch_seg_hash(goss_gpu_ctx* c, uint32_t nseg, const Key1* keys, const uint64_t* seg_off, const uint64_t* seg_end,
                            SegOut* so, uint64_t* seg_pos, uint64_t* seg_cnt, Key1* sk, uint32_t* sc, uint32_t rem_bits, SegCount how)
{
    if (how.table == SegTable::Big && how.rounds)
        hipLaunchKernelGGL(seg_hash_reduce_shared_kernel, unit_grid((uint64_t)nseg << how.rounds), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end,
                           so, seg_pos, seg_cnt, sk, sc, rem_bits, how.rounds);
    else if (how.table == SegTable::Big)
        hipLaunchKernelGGL(seg_hash_reduce_big_kernel, unit_grid(nseg), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end,
                           so, seg_pos, seg_cnt, sk, sc, rem_bits, 0u);
    else
        hipLaunchKernelGGL(seg_hash_reduce_kernel, unit_grid(nseg), dim3(kTB), 0, c->stream, keys, seg_off, seg_end, so, seg_pos, seg_cnt, sk, sc,
                           rem_bits);
}
inline void launch_seg_hash(goss_gpu_ctx* c, uint32_t nseg, const Key2* keys, const uint64_t* seg_off, const uint64_t* seg_end,
                            SegOut* so, uint64_t* seg_pos, uint64_t* seg_cnt, Key2* sk, uint32_t* sc, uint32_t rem_bits, SegCount how)
{
    if (how.table == SegTable::Rem96Packed)
        hipLaunchKernelGGL(seg_hash_reduce96p_kernel, unit_grid(nseg), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end, so,
                           seg_pos, seg_cnt, sk, sc, rem_bits);
    else if (how.table == SegTable::Rem96)
        hipLaunchKernelGGL(seg_hash_reduce96_kernel, unit_grid(nseg), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end, so,
                           seg_pos, seg_cnt, sk, sc, rem_bits);
    else if (how.table == SegTable::Wide)
        hipLaunchKernelGGL(seg_hash_reduce2_wide_kernel, unit_grid(nseg), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end, so,
                           seg_pos, seg_cnt, sk, sc, rem_bits);
    else if (how.table == SegTable::Big)
        hipLaunchKernelGGL(seg_hash_reduce2_big_kernel, unit_grid((uint64_t)nseg << how.rounds), dim3(kSegBigThreads), 0, c->stream, keys, seg_off, seg_end, so,
                           seg_pos, seg_cnt, sk, sc, rem_bits, how.rounds);
    else
        hipLaunchKernelGGL(seg_hash_reduce2_kernel, unit_grid(nseg), dim3(kTB), 0, c->stream, keys, seg_off, seg_end, so, seg_pos, seg_cnt, sk, sc,
                           rem_bits);
}

// Number of distinct keys in the chunk, estimated from its first keys (reads arrive in no
// particular order, so a prefix is a sample): with s sampled keys of which d are distinct,
// M ~ s^2 / (2 (s - d)) (birthday estimate), never less than d.  Returns 0 when the sample has
// no repeated key at all (M unknown, presumably of the order of n).
// Exact number of distinct keys among the first s keys (sorts a copy of them).
template <class K>
uint64_t count_distinct_sample(goss_gpu_ctx* c, const K* keys, uint64_t s)
{
    if (s < 2) return s;
    ArenaScope scope(c->arena);
    K* a = (K*)c->arena.temp(s * sizeof(K));
    K* b = (K*)c->arena.temp(s * sizeof(K));
    HIP_TRY(hipMemcpyAsync(a, keys, s * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
    // auxiliary sort of the sample: histogram-table kernels, kept out of the per-kernel timing
    // so that the partition kernel's launch statistics describe the partition only
    bool in_b;
    {
        Scoped<bool> plain(&c->knobs.lookback, false), mute(&c->mute_timing, true);
        in_b = radix_sort<K, false>(c, a, b, nullptr, nullptr, s, key_digits(c));
    }
    const uint64_t ntiles = (s + kRedTile - 1) / kRedTile;
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(heads_count_kernel<K>), dim3(grid_for(s, kRedTile)), dim3(kTB), 0, c->stream,
                       (const K*)(in_b ? b : a), s, tile_counts);
    return scan_total(c, tile_counts, ntiles);
}

// Number of equally likely keys M from which s draws show d distinct ones: the root of
// d = M (1 - exp(-s / M)) (~ s^2 / (2 (s - d)) when almost every draw is new, ~ d when the
// sample saturates the population).  0 = no repeated key at all (unknown, at least of the order of s).
inline uint64_t birthday_estimate(uint64_t s, uint64_t d)
{
    if (d >= s) return 0;
    double lo = (double)d, hi = (double)d;
    auto seen = [&](double m) { return m * -std::expm1(-(double)s / m); };
    while (seen(hi) < (double)d && hi < 1e19) hi *= 2.0;
    for (int it = 0; it < 80; ++it)
    {
        const double mid = 0.5 * (lo + hi);
        if (seen(mid) < (double)d) lo = mid; else hi = mid;
    }
    return std::max<uint64_t>(d, (uint64_t)hi);
}

// Number of distinct keys of a population of `population` keys of which keys[0, avail) are a random part
// (any prefix of a chunk: reads arrive in no particular order).  The birthday estimate above assumes
// that every key is equally frequent; sequencing reads are not like that -- the k-mers of the genome occur
// `coverage` times each, the k-mers that contain a base-calling error once -- and it then reports little more
// than the genome (1e8 for C2 with 0.1 % errors, where 3.3e8 is right): the counting tables overflow and the
// chunk is redone with more partition bits, several times.  So: the multiplicity SPECTRUM of a slice of
// the key space.  The keys whose mixed bits are zero (all copies of a key or none) are sorted and the keys
// seen exactly once / twice / three times counted (f1, f2, f3).  A key that occurs c times in the population
// shows Poisson(c p) copies in the part (p = avail / population): the frequent component is fitted from
// f2 and f3 (lambda = 3 f3 / f2, G = 2 f2 e^lambda / lambda^2), the singletons it does not explain are
// population keys of multiplicity ~1 seen with probability p each.  Never less than the plain estimate.
template <class K>
uint64_t spectrum_estimate(goss_gpu_ctx* c, const K* keys, uint64_t avail, double population, uint64_t* rare_out = nullptr)
{
    // *rare_out: of the estimate, the keys of multiplicity ~1 in the population (more of the same input brings more
    // of THEM; the frequent keys it mostly brings again); the whole estimate where the spectrum could not be fitted
    if (rare_out) *rare_out = avail;
    if (avail < 2) return avail;
    const uint64_t scan = std::min<uint64_t>(avail, 1ULL << 30);
    uint32_t q = 1;
    while ((scan / q) > (3u << 20) && q < (1u << 16)) q <<= 1;          // 1.5 to 3 M keys survive
    const uint64_t cap = scan / q + scan / q / 4 + (1u << 16);
    ArenaScope scope(c->arena);
    K* a = (K*)c->arena.temp(cap * sizeof(K));
    K* b = (K*)c->arena.temp(cap * sizeof(K));
    unsigned long long* ctr = (unsigned long long*)c->arena.temp(64);
    HIP_TRY(hipMemsetAsync(ctr, 0, 64, c->stream));
    Scoped<bool> mute(&c->mute_timing, true);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(slice_filter_kernel<K>), dim3((uint32_t)std::min<uint64_t>(2048, (scan + kTB - 1) / kTB)), dim3(kTB), 0, c->stream,
                       keys, scan, q - 1, a, ctr, cap);
    unsigned long long* h = (unsigned long long*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(h, ctr, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t sf = std::min<uint64_t>(h[0], cap);
    uint64_t est = 0;
    if (sf >= 2)
    {
        const bool in_b = [&]() { Scoped<bool> plain(&c->knobs.lookback, false); return radix_sort<K, false>(c, a, b, nullptr, nullptr, sf, key_digits(c)); }();
        HIP_TRY(hipMemsetAsync(ctr, 0, 64, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(spectrum_kernel<K>), dim3((uint32_t)std::min<uint64_t>(1024, (sf + kTB - 1) / kTB)), dim3(kTB), 0, c->stream,
                           (const K*)(in_b ? b : a), sf, ctr);
        HIP_TRY(hipMemcpyAsync(h, ctr, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const double d = (double)h[0], f1 = (double)h[1], f2 = (double)h[2], f3 = (double)h[3];
        const double p = std::min(1.0, (double)scan / std::max(population, (double)scan));
        const double scale_q = (double)q;
        // plain estimate on the slice (equally frequent keys), scaled to the key space
        const uint64_t plain = scan >= (uint64_t)population ? (uint64_t)(d * scale_q) : (uint64_t)((double)birthday_estimate(sf, (uint64_t)d) * scale_q);
        double model = 0, rare_keys = -1.0;
        if (p >= 1.0) { model = d; rare_keys = f1; }              // the whole population was looked at
        else if (f2 >= 256.0 && f3 >= 64.0)
        {
            const double lambda = 3.0 * f3 / f2;
            const double G = 2.0 * f2 * std::exp(lambda) / (lambda * lambda);
            const double rare = std::max(0.0, f1 - G * lambda * std::exp(-lambda)) / p;
            // (seen but fitted by neither: the keys seen four times and more are part of G already)
            model = G + rare;
            rare_keys = rare;
        }
        est = std::max<uint64_t>(plain, (uint64_t)(model * scale_q));
        est = std::max<uint64_t>(est, (uint64_t)(d * scale_q));
        if (plain == 0 && model == 0) est = 0;                    // no repeated key at all: unknown
        if (rare_out) *rare_out = rare_keys < 0 ? est : std::min<uint64_t>(est, (uint64_t)(rare_keys * scale_q));
        if (c->knobs.debug)
            std::fprintf(stderr, "libgossgpu: spectrum of 1/%u of the key space over %llu keys (p = %.4f): d %.0f f1 %.0f f2 %.0f f3 %.0f -> plain %llu, fitted %.0f, estimate %llu\n",
                         q, (unsigned long long)scan, p, d, f1, f2, f3, (unsigned long long)plain, model * scale_q, (unsigned long long)est);
    }
    return est;
}

template <class K>
uint64_t estimate_distinct(goss_gpu_ctx* c, const K* keys, uint64_t n)
{
    if (n < 2) return n;
    if (n <= (4u << 20)) return count_distinct_sample<K>(c, keys, n);
    // a prefix of the chunk stands for the chunk: reads arrive in no particular order
    return spectrum_estimate<K>(c, keys, std::min<uint64_t>(n, 256u << 20), (double)n);
}

// The staging area of a segment pass -- a kernel counts or merges every unit (a segment, or one of the 2^rounds shares of
// one) into `keys` / `counts` at the cursor of the device's SegOut, and notes where (`pos`) and how many (`cnt`) -- with
// its bookkeeping: taken from the arena under the caller's scope, read back, and gathered in unit order into a run.
template <class K>
struct SegStage {
    goss_gpu_ctx* c;
    uint32_t nunit;
    K* keys; uint32_t* counts; uint64_t cap;          // the staged entries and how many there is room for
    uint64_t* pos; uint64_t* cnt; uint64_t* dst;      // per unit: first staged entry, entries, first entry in the run
    SegOut* out;                                      // the device's cursor and overflow word
    SegOut h{};                                       // ... as read() found it: a copy, nothing else writes it

    SegStage(goss_gpu_ctx* ctx, uint32_t units, K* stage_keys, uint32_t* stage_counts, uint64_t stage_cap)
        : c(ctx), nunit(units), keys(stage_keys), counts(stage_counts), cap(stage_cap)
    {
        pos = (uint64_t*)c->arena.temp((uint64_t)nunit * 8);
        cnt = (uint64_t*)c->arena.temp(((uint64_t)nunit + 1) * 8);
        dst = (uint64_t*)c->arena.temp(((uint64_t)nunit + 1) * 8);
        out = (SegOut*)c->arena.temp(sizeof(SegOut));
        h.stage_cap = cap;
        HIP_TRY(hipMemcpyAsync(out, &h, sizeof(SegOut), hipMemcpyHostToDevice, c->stream));
    }
    // staged (key,count) pairs share one spare buffer of n keys: cap entries of keys, then the counts
    SegStage(goss_gpu_ctx* ctx, uint32_t units, K* spare, uint64_t n)
        : SegStage(ctx, units, spare, (uint32_t*)(spare + n * sizeof(K) / (sizeof(K) + 4)), n * sizeof(K) / (sizeof(K) + 4)) {}

    // What the kernel left in the device's SegOut (waits for it).  The pinned bytes it comes through belong to whoever
    // reads back next -- reduce_runs, under count_overflowed_units -- so the copy is what is kept.
    SegOut& read()
    {
        HIP_TRY(hipMemcpyAsync(c->h_pinned, out, sizeof(SegOut), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        h = *(const SegOut*)c->h_pinned;
        return h;
    }
    // The staged entries in unit order into permanent room: *run is the run (launched, not waited for).
    void gather(Run* run)
    {
        HIP_TRY(hipMemcpyAsync(dst, cnt, (uint64_t)nunit * 8, hipMemcpyDeviceToDevice, c->stream));
        exclusive_scan_u64(c, dst, nunit);
        run->m = h.cursor;
        run->keys = c->arena.perm(std::max<uint64_t>(run->m, 1) * sizeof(K));
        run->counts = (uint32_t*)c->arena.perm(std::max<uint64_t>(run->m, 1) * 4);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_gather_kernel<K>), unit_grid(nunit), dim3(kTB), 0, c->stream,
                           (const K*)keys, (const uint32_t*)counts, (const uint64_t*)pos,
                           (const uint64_t*)dst, (const uint64_t*)cnt, (K*)run->keys, run->counts);
    }
};

// Units (segments) whose counting table overflowed are counted by themselves -- all of them in one sort -- into the staging
// area the kernel filled for the others (round 6).  A FEW giant segments are what skew looks like -- reads with homopolymer stretches:
// every window that begins with nine T's lies in one 17-bit segment, tens of millions of distinct keys where a table
// holds thousands -- and the ladder of "the whole chunk again with more bits" neither splits them (the bits below the
// prefix are all T as well) nor ends before the full sort of the chunk: 3.8 s for 2.5 G windows that now take 0.1 s.
// `expand(unit, first, n, dst)` queues the unit's n keys as full keys at dst.  Returns 0 (all counted: the stage's host
// SegOut updated, the device's pos / cnt patched), or the code the caller hands on: 1 -- too many such units, no room for
// their sort, a count beyond 32 bits: the old ladder takes over -- or 2, the staging area is full.
constexpr size_t kMaxOverflowUnits = 4096;
template <class K, class Expand, class UnitLow>
int count_overflowed_units(SegStage<K>& st, const uint64_t* d_beg, const uint64_t* d_end, Expand expand, UnitLow unit_low)
{
    // (`unit_low(u)`: the smallest key a key of unit u can be -- the units are ranges of the key space in unit order)
    goss_gpu_ctx* c = st.c;
    const uint32_t nunit = st.nunit;
    std::vector<uint64_t> cnt(nunit), beg(nunit), end(nunit);
    HIP_TRY(hipMemcpyAsync(cnt.data(), st.cnt, (size_t)nunit * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(beg.data(), d_beg, (size_t)nunit * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(end.data(), d_end, (size_t)nunit * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> units;
    uint64_t total = 0;
    for (uint32_t u = 0; u < nunit; ++u)
        if (cnt[u] == kSegOverflowed) { units.push_back(u); total += end[u] - beg[u]; if (units.size() > kMaxOverflowUnits) return 1; }
    if (units.empty() || total == 0) return 1;          // (the flag without a marked unit: not this function's case)
    // ALL of them in one sort (their keys are full keys: the units stay apart) -- one by one, a few hundred small sorts
    // cost half a millisecond of launches and waits each
    const uint64_t need = total * (3 * sizeof(K) + 16) + units.size() * (2 * sizeof(K) + 16) + (64ULL << 20);
    if (c->arena.avail() < need) return 1;
    ArenaScope scope(c->arena);
    // the permanent end is put back on every way out, an exception included: r's permanent blocks are only a stopover
    // on the way into the staging area
    Scoped<uint64_t> perm_end(&c->arena.lo, c->arena.lo);
    const size_t maps0 = c->build.big_maps.size();
    K* a = (K*)c->arena.temp(total * sizeof(K));
    K* b = (K*)c->arena.temp(total * sizeof(K));
    {
        uint64_t at = 0;
        for (uint32_t u : units) { expand(u, beg[u], end[u] - beg[u], a + at); at += end[u] - beg[u]; }
    }
    Run r{nullptr, nullptr, 0};
    {
        // (the sort's passes belong to the counting phase that is being timed; put back also when the sort gives up)
        Scoped<bool> mute(&c->mute_timing, true);
        const bool moved = radix_sort<K, false>(c, a, b, nullptr, nullptr, total, key_digits(c));
        r = reduce_runs<K>(c, moved ? b : a, nullptr, total, moved ? a : b);
    }
    int rc = 0;
    if (r.big >= 0 || c->build.big_maps.size() != maps0) { c->build.big_maps.resize(maps0); rc = 1; }          // (a count of 2^32 - 1 or more: the general way keeps those)
    else if (st.h.cursor + r.m > st.h.stage_cap) rc = 2;
    else
    {
        const uint32_t nu = (uint32_t)units.size();
        std::vector<K> lows(nu), highs(nu);
        std::vector<uint8_t> last(nu);
        for (uint32_t i = 0; i < nu; ++i)
        {
            lows[i] = unit_low(units[i]);
            last[i] = units[i] + 1 == nunit ? 1 : 0;
            highs[i] = last[i] ? lows[i] : unit_low(units[i] + 1);
        }
        K* d_lows = (K*)c->arena.temp(nu * sizeof(K));
        K* d_highs = (K*)c->arena.temp(nu * sizeof(K));
        uint32_t* d_units = (uint32_t*)c->arena.temp(nu * 4 + 16);
        uint8_t* d_last = (uint8_t*)c->arena.temp(nu + 16);
        HIP_TRY(hipMemcpyAsync(d_lows, lows.data(), nu * sizeof(K), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_highs, highs.data(), nu * sizeof(K), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_units, units.data(), nu * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_last, last.data(), nu, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(st.keys + st.h.cursor, r.keys, r.m * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(st.counts + st.h.cursor, r.counts, r.m * 4, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(unit_bounds_kernel<K>), dim3(grid_for(nu, kTB)), dim3(kTB), 0, c->stream, (const K*)r.keys, r.m, (const K*)d_lows,
                           (const K*)d_highs, (const uint8_t*)d_last, (const uint32_t*)d_units, nu, (unsigned long long)st.h.cursor, st.pos, st.cnt);
        HIP_TRY(hipStreamSynchronize(c->stream));          // (the host vectors go)
        st.h.cursor += r.m;
        st.h.overflow = 0;
        c->stats.overflow_units += nu;
        if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: %u segment(s) with more distinct keys than a table holds counted by sort (%llu keys, %llu distinct)\n",
                                   nu, (unsigned long long)total, (unsigned long long)r.m);
    }
    return rc;
}

// How segment_reduce and segment_reduce32 end once their kernel's SegOut is read: tables that overflowed and nothing
// else go by sort where the form allows it (`by_sort`; `expand` and `unit_low` as count_overflowed_units takes them);
// what overflow is left is the answer -- 1 a table, 2 the staging area -- and else the staged entries become *out.
// Stops the caller's timer either way; the caller's scope gives the temporaries back.
template <class K, class Expand, class UnitLow>
int finish_segments(SegStage<K>& st, bool by_sort, const uint64_t* seg_beg, const uint64_t* seg_end, PhaseTimer& t, Run* out,
                    Expand expand, UnitLow unit_low)
{
    goss_gpu_ctx* c = st.c;
    if (st.h.overflow == 1u && by_sort && c->knobs.overflow_by_sort && count_overflowed_units<K>(st, seg_beg, seg_end, expand, unit_low) == 2)
        st.h.overflow = 2u;
    if (st.h.overflow)
    {
        const int why = (st.h.overflow & 1u) ? 1 : 2;
        t.stop();
        return why;
    }
    st.gather(out);
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Count every segment of the partitioned keys `part` in LDS; `spare` (n keys) is the staging area.
// Segment s is part[seg_beg[s], seg_end[s]) when the bounds are given (sub-region layout), else
// the bounds are found by binary search in the dense, partitioned array.
template <class K>
int segment_reduce(goss_gpu_ctx* c, K* part, K* spare, uint64_t n, uint32_t segbits, Run* out, const uint64_t* seg_beg = nullptr,
                   const uint64_t* seg_end = nullptr, SegCount how = {})
{
    const uint32_t keybits = 2 * c->len;
    const uint32_t shift = keybits - segbits;
    const uint32_t nseg = 1u << segbits;
    const uint32_t nunit = nseg << how.rounds;      // (segment, round) units of the staging area
    ArenaScope scope(c->arena);
    PhaseTimer t(c, GOSS_T_REDUCE, n);
    uint64_t* seg_off = (uint64_t*)c->arena.temp(((uint64_t)nseg + 1) * 8);
    SegStage<K> st(c, nunit, spare, n);
    if (!seg_beg)
    {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_bounds_kernel<K>), dim3(nseg / 256 + 1), dim3(256), 0, c->stream,
                           (const K*)part, n, shift, nseg, seg_off);
        seg_beg = seg_off; seg_end = seg_off + 1;
    }
    launch_seg_hash(c, nseg, (const K*)part, seg_beg, seg_end, st.out, st.pos, st.cnt, st.keys, st.counts, shift, how);
    check_launch("segment counting kernel");
    st.read();
    // (by sort: not the forms in which several workgroups share a segment, whose units are not ranges of `part`)
    return finish_segments(st, how.rounds == 0, seg_beg, seg_end, t, out,
        [&](uint32_t u, uint64_t first, uint64_t cnt_u, K* dst) {
            if constexpr (std::is_same<K, Key2>::value)
            {
                if (how.table == SegTable::Rem96Packed)          // (12-byte records of the remainders: the second level's packed form)
                {
                    hipLaunchKernelGGL(expand_rem96_kernel, dim3(grid_for(cnt_u, kTB)), dim3(kTB), 0, c->stream,
                                       reinterpret_cast<const Rem96*>(part) + first, cnt_u, (uint64_t)u, shift, dst);
                    return;
                }
            }
            HIP_TRY(hipMemcpyAsync(dst, part + first, cnt_u * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        },
        [&](uint32_t u) -> K {
            if constexpr (std::is_same<K, Key2>::value)
            {
                const unsigned __int128 v = (unsigned __int128)u << shift;
                return Key2{(uint64_t)v, (uint64_t)(v >> 64)};
            }
            else return Key1{(uint64_t)u << shift};
        });
}

// Partition ka on its top `segbits` bits (result back in ka or kb), count every segment in LDS.
// Returns 0 on success; 1 if some segment holds too many distinct keys (retry with more
// partition bits); 2 if the staging area is too small (use the full sort).  The keys stay,
// permuted, in ka or kb (*in_b_out).
template <class K>
int segment_count(goss_gpu_ctx* c, K* ka, K* kb, uint64_t n, uint32_t segbits, bool* in_b_out, Run* out)
{
    const uint32_t keybits = 2 * c->len;
    const uint32_t shift = keybits - segbits;
    const uint32_t npass = (segbits + 7) / 8;
    const unsigned long long* prehist =
        (segbits == kSegBits && c->extract_hist_shift == shift && c->knobs.lookback && !*in_b_out) ? c->d_ctr->hist : nullptr;
    K* src = *in_b_out ? kb : ka;
    K* dst = *in_b_out ? ka : kb;
    bool moved = radix_sort<K, false>(c, src, dst, nullptr, nullptr, n, npass, shift, prehist);
    K* part = moved ? dst : src;          // partitioned keys
    K* spare = moved ? src : dst;         // free half of the ping-pong: staging area
    *in_b_out = (part == kb);
    return segment_reduce<K>(c, part, spare, n, segbits, out);
}

// What segment_reduce32 counts, as count_rem32 laid it out.
struct Rem32Layout {
    const uint64_t* seg_beg; const uint64_t* seg_end; uint32_t nseg;          // segment s is rems[seg_beg[s], seg_end[s])
    int slots;                                        // of a counting table: 2048, 8192, 16384; any other value means 4096
    bool squeeze, image;
    uint32_t rbits, sqbit, split_bits;                // bits of a remainder (before the squeeze), the squeezed bit, third-level bits
};
// The same for the 32-bit-remainder form (subpart32_kernel's output): nseg = 2^17 .. 2^20 segments of u32 remainders, counted by
// seg_hash_reduce32b_kernel in tables of `slots` slots; `spare` (n one-word keys) is the staging area.  `image`: the
// sub-regions hold the images of the remainders (goss_words.hpp), as the second level writes them when no third level follows.
// Returns 0, 1 (a table overflowed) or 2 (staging area too small) like segment_reduce.
int segment_reduce32(goss_gpu_ctx* c, const uint32_t* rems, Key1* spare, uint64_t n, Run* out, const Rem32Layout& lay)
{
    const bool squeeze = lay.squeeze, image = lay.image;
    const uint32_t rbits = lay.rbits, sqbit = lay.sqbit, split_bits = lay.split_bits;
    ArenaScope scope(c->arena);
    PhaseTimer t(c, GOSS_T_REDUCE, n);
    SegStage<Key1> st(c, lay.nseg, spare, n);
    // (buckets of four remainders, home bucket only in the fast path)
    auto launch = [&](auto slots) {
        with_bool(squeeze, [&](auto sq) { with_bool(image, [&](auto img) {
            constexpr int SLOTS = decltype(slots)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_hash_reduce32b_kernel<SLOTS, decltype(sq)::value, decltype(img)::value>), unit_grid(lay.nseg),
                               dim3(SLOTS <= 4096 ? kTB : SLOTS / 4096 * kTB), 0, c->stream, rems, lay.seg_beg, lay.seg_end, st.out, st.pos, st.cnt,
                               st.keys, st.counts, rbits, sqbit, split_bits);
        }); });
    };
    if (lay.slots == 2048) launch(int_c<2048>{});
    else if (lay.slots == 8192) launch(int_c<8192>{});
    else if (lay.slots == 16384) launch(int_c<16384>{});
    else launch(int_c<4096>{});
    check_launch("32-bit segment counting kernel");
    st.read();
#if defined(GOSS_STAMPS)
    if (st.h.stamps[7])
        std::fprintf(stderr, "libgossgpu: counting stamps per segment (cycles of wave 0): set-up %.0f  loads+copy %.0f  fast path %.0f  slow path %.0f  closing barrier %.0f  ordering %.0f  write-out %.0f   (%llu segments)\n",
                     (double)st.h.stamps[0] / st.h.stamps[7], (double)st.h.stamps[1] / st.h.stamps[7], (double)st.h.stamps[2] / st.h.stamps[7], (double)st.h.stamps[3] / st.h.stamps[7],
                     (double)st.h.stamps[4] / st.h.stamps[7], (double)st.h.stamps[5] / st.h.stamps[7], (double)st.h.stamps[6] / st.h.stamps[7], (unsigned long long)st.h.stamps[7]);
#endif
    return finish_segments(st, true, lay.seg_beg, lay.seg_end, t, out,
        [&](uint32_t u, uint64_t first, uint64_t cnt_u, Key1* dst) {
            const uint64_t prefix = (uint64_t)(u >> split_bits) << rbits;          // (as the counting kernel's write-out)
            with_bool(squeeze, [&](auto sq) { with_bool(image, [&](auto img) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(expand_rem32_kernel<decltype(sq)::value, decltype(img)::value>), dim3(grid_for(cnt_u, kTB)), dim3(kTB), 0,
                                   c->stream, rems + first, cnt_u, prefix, sqbit, dst);
            }); });
        },
        [&](uint32_t u) -> Key1 {
            // the unit's smallest key: its segment's prefix, and the unit's number in the top split_bits of the remainder
            // (a plain remainder put together here, nothing read from a sub-region: images come with split_bits = 0)
            const uint32_t rem_bits = rbits - (squeeze ? 1u : 0u);
            const uint32_t sub = split_bits ? (u & ((1u << split_bits) - 1u)) << (rem_bits - split_bits) : 0u;
            const uint64_t low = squeeze ? rem32_unpack<true>(sub, sqbit) : rem32_unpack<false>(sub, sqbit);
            return Key1{((uint64_t)(u >> split_bits) << rbits) | low};
        });
}

// Count a chunk of n extracted keys (in ka): segment path with as many partition bits as the
// estimated number of distinct keys asks for, more bits after an overflow, finally the full
// LSD sort + run compaction.
template <class K>
Run count_keys(goss_gpu_ctx* c, K* ka, K* kb, uint64_t n)
{
    Run r{nullptr, nullptr, 0};
    bool in_b = false;
    if (use_segment_path<K>(c))
    {
        const uint32_t keybits = 2 * c->len;
        const uint64_t limit = SegCfg<K>::kLimit;
        const uint64_t m_est = n <= (uint64_t)(1u << kSegBits) * (limit / 2) ? n : estimate_distinct<K>(c, ka, n);
        // worth it only with real duplication (and the staging area needs M <= ~2n/3)
        if (m_est != 0 && (m_est <= n / 3 || n <= (uint64_t)(1u << kSegBits) * (limit / 2)))
        {
            uint32_t segbits = kSegBits;
            while (segbits < kSegBitsMax && (m_est >> segbits) > limit * 3 / 4) segbits += 4;   // margin for skew
            for (; segbits <= kSegBitsMax && segbits + 8 <= keybits; segbits += 4)
            {
                if ((m_est >> segbits) > limit) continue;
                int rc = segment_count<K>(c, ka, kb, n, segbits, &in_b, &r);
                if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: count_keys: %llu keys, %u segment bits -> %d (%llu distinct)\n",
                                           (unsigned long long)n, segbits, rc, (unsigned long long)(rc == 0 ? r.m : 0));
                if (rc == 0) return r;
                if (rc == 2) break;
                c->stats.segment_retries++;
            }
        }
    }
    K* src = in_b ? kb : ka;
    K* dst = in_b ? ka : kb;
    bool moved = radix_sort<K, false>(c, src, dst, nullptr, nullptr, n, key_digits(c));
    PhaseTimer t(c, GOSS_T_REDUCE, n);
    r = reduce_runs<K>(c, moved ? dst : src, nullptr, n, moved ? src : dst);
    t.stop();
    if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: count_keys: full sort of %llu keys -> %llu distinct\n", (unsigned long long)n, (unsigned long long)r.m);
    return r;
}

// A run counted in strand-representative space (extract1_part_kernel, MODE 0) -> the run the rest of
// the library expects: every key replaced by gossamer's canonical form (the strand with the smaller
// FNV-1a hash), then (key,count) pairs put back in key order.  The map is a bijection between the
// two choices of representative, so counts carry over and no two entries collide.
template <class K>
void canonicalize_run(goss_gpu_ctx* c, Run& r)
{
    const uint64_t m = r.m;
    r.rep = false;
    if (m == 0) return;
    PhaseTimer t(c, GOSS_T_ORDER, m);
    // the run's own storage is one side of the sort's ping-pong, a temporary copy the other
    const uint64_t need = m * sizeof(K) + m * 4 + 512;
    if (c->arena.avail() < need + (256ULL << 20)) grow_arena(c, need + (256ULL << 20));      // (rebases r: it lives in c->build.runs)
    ArenaScope scope(c->arena);
    K* ka = (K*)r.keys;
    uint32_t* va = r.counts;
    K* kb = (K*)c->arena.temp(m * sizeof(K));
    uint32_t* vb = (uint32_t*)c->arena.temp(m * 4);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(canonical_map_kernel<K>), dim3(grid_for(m, kTB)), dim3(kTB), 0, c->stream,
                       (const K*)ka, ka, m, c->len);
    Scoped<bool> mute(&c->mute_timing, true);          // the sort's passes belong to this phase, not to the partition classes
    bool in_b = false, ordered = false;
    const uint32_t keybits = 2 * c->len;
    if constexpr (std::is_same<K, Key1>::value)
    {
        // canonical forms are uniform on their leading bits: two (three) radix passes group the pairs by their
        // top 16 (17 .. 24) bits, then every group (~m / 2^bits pairs, at most 4 096) is ordered in LDS -- three or
        // four passes over the pairs instead of one per key byte.  More than 16 bits for runs above 157 M keys
        // (reads with errors; the ranks of a multi-GPU build hold up to the whole k-mer set before the exchange)
        uint32_t sb = 16;
        while (sb < 24 && m > (1ULL << sb) * 2400) ++sb;                // the fewest groups of at most ~2 400 pairs
        if (c->knobs.order_bits) sb = c->knobs.order_bits;
        if (keybits >= sb + 10 && m >= (1u << 20) && m <= (1ULL << sb) * 2400)
        {
            const uint32_t nseg = 1u << sb;
            in_b = radix_sort<K, true>(c, ka, kb, va, vb, m, (sb + 7) / 8, keybits - sb);
            K* sk = in_b ? kb : ka;
            uint32_t* sv = in_b ? vb : va;
            ArenaScope groups(c->arena);          // (given back before the full sort below asks for its tables)
            uint64_t* soff = (uint64_t*)c->arena.temp(((uint64_t)nseg + 1) * 8);
            uint32_t* flag = (uint32_t*)c->arena.temp(16);
            HIP_TRY(hipMemsetAsync(flag, 0, 4, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_bounds_kernel<K>), dim3(nseg / 256 + 1), dim3(256), 0, c->stream,
                               (const K*)sk, m, keybits - sb, nseg, soff);
            hipLaunchKernelGGL(seg_sort_pairs_kernel, unit_grid(nseg), dim3(kTB), 0, c->stream, sk, sv, (const uint64_t*)soff,
                               keybits - sb, flag);
            uint32_t* hf = (uint32_t*)c->h_pinned;
            HIP_TRY(hipMemcpyAsync(hf, flag, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            ordered = hf[0] == 0;
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: canonical order of %llu keys by %u-bit groups: %s\n", (unsigned long long)m, sb, ordered ? "done" : "skewed, full sort");
            if (!ordered)
            {
                // skewed bits: order everything by the remaining digits as well (the top bits are in place,
                // a full stable sort from the current buffer is simply the general answer)
                if (in_b) { std::swap(ka, kb); std::swap(va, vb); }
                in_b = false;
            }
        }
    }
    if (!ordered) in_b = radix_sort<K, true>(c, ka, kb, va, vb, m, key_digits(c));
    if ((in_b ? kb : ka) != (K*)r.keys)
    {
        HIP_TRY(hipMemcpyAsync(r.keys, in_b ? kb : ka, m * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(r.counts, in_b ? vb : va, m * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
}

// A run of a graph build counted in strand-pair space (one representative per window, process_chunk_fused) -> both
// strands: run `ri` keeps its keys (palindromic edges get their count doubled: the adapter yields them twice per
// window), and a second run holds the reverse complements with the same counts, sorted; both are in the full key space
// and disjoint, the caller merges them.  Exact counts beyond 32 bits are mirrored in the runs' maps.
template <class K>
void expand_graph_run(goss_gpu_ctx* c, size_t ri)
{
    const uint64_t m = c->build.runs[ri].m;
    c->build.runs[ri].rep = false;
    if (m == 0) return;
    PhaseTimer t(c, GOSS_T_ORDER, m);
    {
        const uint64_t need = 3 * m * (sizeof(K) + 4) + (256ULL << 20);
        if (c->arena.avail() < need) grow_arena(c, need);          // (rebases the runs: fetched by index below)
    }
    ArenaScope scope(c->arena);
    K* bk = (K*)c->arena.temp(m * sizeof(K));
    uint32_t* bc = (uint32_t*)c->arena.temp(m * 4);
    K* tk = (K*)c->arena.temp(m * sizeof(K));
    uint32_t* tc = (uint32_t*)c->arena.temp(m * 4);
    unsigned long long* dbig = (unsigned long long*)c->arena.temp((2 + 3 * kMaxBig) * 8);
    unsigned long long* npal = dbig + 1 + 3 * kMaxBig;
    HIP_TRY(hipMemsetAsync(dbig, 0, (2 + 3 * kMaxBig) * 8, c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(graph_expand_kernel<K>), dim3(grid_for(m, kTB)), dim3(kTB), 0, c->stream, (const K*)c->build.runs[ri].keys,
                       c->build.runs[ri].counts, m, c->len, bk, bc, dbig, kMaxBig, npal);
    // (the pads -- all ones, in the slots of the palindromes -- must end up BEHIND every key: where the key's 2 len bits
    // fill whole digits (len a multiple of four: 12, 16, .. 28, 32, ..) the edge T..T has every digit a pad has, a stable
    // sort on those digits alone leaves the two kinds in input order, and the cut below dropped T..T for a pad whenever a
    // palindrome stood in front of it: one digit more -- zeros for a key, ones for a pad -- tells them apart)
    const uint32_t nd = key_digits(c) + ((2 * c->len) % 8 == 0 ? 1u : 0u);
    const bool in_b = [&]() {
        Scoped<bool> mute(&c->mute_timing, true);          // the sort's passes belong to this phase
        return radix_sort<K, true>(c, bk, tk, bc, tc, m, nd);
    }();
    std::vector<unsigned long long> hb(2 + 3 * kMaxBig);
    HIP_TRY(hipMemcpyAsync(hb.data(), dbig, hb.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t npads = hb[1 + 3 * kMaxBig];
    if (hb[0] > kMaxBig) throw StatusError{GOSS_ERR_COUNT_OVERFLOW, "more than 256 keys occurred 2^32 times or more"};
    const uint64_t mb = m - npads;
    // exact counts: the representative's entry stays (doubled for a palindrome), its reverse complement gets the same
    BigMap ma, mbm;
    if (c->build.runs[ri].big >= 0)
        for (const auto& kv : c->build.big_maps[c->build.runs[ri].big])
        {
            K k;
            if constexpr (sizeof(K) == 8) k = K{kv.first.second}; else k = K{kv.first.second, kv.first.first};
            const K r = revcomp(k, c->len);
            if (r == k) ma[kv.first] = 2 * kv.second;
            else { ma[kv.first] = kv.second; mbm[std::make_pair((uint64_t)key_hi_word(r), (uint64_t)key_lo_word(r))] = kv.second; }
        }
    for (uint64_t i = 0; i < hb[0]; ++i) ma[std::make_pair((uint64_t)hb[2 + 3 * i], (uint64_t)hb[1 + 3 * i])] = hb[3 + 3 * i];
    c->build.runs[ri].big = -1;
    if (!ma.empty()) { c->build.big_maps.push_back(std::move(ma)); c->build.runs[ri].big = (int)c->build.big_maps.size() - 1; }
    if (mb)
    {
        Run b{nullptr, nullptr, mb};
        b.keys = c->arena.perm(mb * sizeof(K));
        b.counts = (uint32_t*)c->arena.perm(mb * 4);
        HIP_TRY(hipMemcpyAsync(b.keys, in_b ? tk : bk, mb * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(b.counts, in_b ? tc : bc, mb * 4, hipMemcpyDeviceToDevice, c->stream));
        if (!mbm.empty()) { c->build.big_maps.push_back(std::move(mbm)); b.big = (int)c->build.big_maps.size() - 1; }
        c->build.runs.push_back(b);
    }
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: %llu strand pairs expanded (%llu palindromes)\n", (unsigned long long)m, (unsigned long long)npads);
}

// ---- merging runs ---------------------------------------------------------------------------
// What the three ways of merging share: the runs concatenated in (ka, va) -- run r is [run_off[r], run_off[r + 1]) --
// and the free half of the ping-pong (kb, vb).  Each way leaves the merged run in *out, above the rewound permanent end;
// the first two answer false where they decline, with the input intact.
template <class K>
struct MergeInput {
    goss_gpu_ctx* c;
    K* ka; K* kb; uint32_t* va; uint32_t* vb;
    std::vector<uint64_t> run_off;
    std::vector<int> in_bigs;                       // the inputs' counts beyond 32 bits (graph mode)
    uint64_t total; uint32_t nruns;

    // every run's segment bounds, run r's nseg + 1 offsets at bounds + r (nseg + 1)
    void launch_bounds(uint32_t nseg, uint32_t shift, uint64_t* bounds) const
    {
        for (uint32_t r = 0; r < nruns; ++r)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_bounds_kernel<K>), dim3(nseg / 256 + 1), dim3(256), 0, c->stream,
                               (const K*)(ka + run_off[r]), run_off[r + 1] - run_off[r], shift, nseg,
                               bounds + (uint64_t)r * (nseg + 1));
    }
};

// Two-word keys with at most 96 bits below a 16-bit prefix: the runs' entries are counted into the LDS table
// of the counting kernel, segment by segment (seg_hash_merge96_kernel).  The runs of a high-coverage build all
// hold the same keys, so 65 536 tables of 8192 slots take them; a segment with more than 6144 distinct keys, or
// a count that reaches 2^31, sends the merge down the general path.
inline bool merge_by_table(const MergeInput<Key2>& in, Run* out)
{
    goss_gpu_ctx* c = in.c;
    const uint32_t keybits = 2 * c->len, nruns = in.nruns;
    if (!(c->knobs.table96 && keybits >= 16 + 8 && keybits - 16 <= 96 && nruns <= (uint32_t)kMergeRuns && in.total >= c->knobs.hash_merge_min)) return false;
    const uint32_t nseg = 65536, shift = keybits - 16;
    ArenaScope scope(c->arena);
    uint64_t* bounds = (uint64_t*)c->arena.temp((uint64_t)nruns * (nseg + 1) * 8);
    uint64_t* d_off = (uint64_t*)c->arena.temp((nruns + 1) * 8);
    SegStage<Key2> st(c, nseg, in.kb, in.vb, in.total);
    HIP_TRY(hipMemcpyAsync(d_off, in.run_off.data(), (nruns + 1) * 8, hipMemcpyHostToDevice, c->stream));
    PhaseTimer t(c, GOSS_T_REDUCE, in.total);
    in.launch_bounds(nseg, shift, bounds);
    hipLaunchKernelGGL(seg_hash_merge96_kernel, unit_grid(nseg), dim3(kSegBigThreads), 0, c->stream, (const Key2*)in.ka, (const uint32_t*)in.va,
                       (const uint64_t*)d_off, (const uint64_t*)bounds, nruns, st.out, st.pos, st.cnt, in.kb, in.vb, shift);
    if (st.read().overflow) { t.stop(); return false; }
    st.gather(out);
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stats.seg_merges++;
    c->stats.hash_merges++;
    return true;
}

// Merge by segments (seg_merge_kernel): every entry read once, written once.  Needs every
// segment's entries of all runs to fit kMergeCap; else the concatenation is sorted again.
template <class K>
bool merge_by_segments(const MergeInput<K>& in, Run* out)
{
    goss_gpu_ctx* c = in.c;
    const uint32_t keybits = 2 * c->len, nruns = in.nruns;
    if (!(nruns <= (uint32_t)kMergeRuns && in.total >= 1024)) return false;
    uint32_t segbits = 8;
    while (segbits < 26 && segbits + 1 <= keybits && (in.total >> segbits) > (uint64_t)kMergeCap / 2) ++segbits;
    for (int attempt = 0; attempt < 3 && segbits <= 26 && segbits <= keybits; ++attempt, segbits += 2)
    {
        const uint32_t nseg = 1u << segbits, shift = keybits - segbits;
        ArenaScope attempt_scope(c->arena);
        const uint64_t need = (uint64_t)nruns * (nseg + 1) * 8 + (uint64_t)nseg * 32 + (1u << 20);
        if (c->arena.avail() < need) break;
        uint64_t* bounds = (uint64_t*)c->arena.temp((uint64_t)nruns * (nseg + 1) * 8);
        uint64_t* d_off = (uint64_t*)c->arena.temp((nruns + 1) * 8);
        unsigned long long* d_max = (unsigned long long*)c->arena.temp(16);
        HIP_TRY(hipMemcpyAsync(d_off, in.run_off.data(), (nruns + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(d_max, 0, 16, c->stream));
        PhaseTimer t(c, GOSS_T_REDUCE, in.total);
        in.launch_bounds(nseg, shift, bounds);
        hipLaunchKernelGGL(seg_totals_kernel, dim3(nseg / 256 + 1), dim3(256), 0, c->stream, (const uint64_t*)bounds, nruns, nseg, d_max);
        unsigned long long* hmax = (unsigned long long*)c->h_pinned;
        HIP_TRY(hipMemcpyAsync(hmax, d_max, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (hmax[0] > (unsigned long long)kMergeCap) { t.stop(); continue; }
        SegStage<K> st(c, nseg, in.kb, in.vb, in.total);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_merge_kernel<K>), unit_grid(nseg), dim3(kTB), 0, c->stream, (const K*)in.ka, (const uint32_t*)in.va,
                           (const uint64_t*)d_off, (const uint64_t*)bounds, nruns, nseg, st.out, st.pos, st.cnt, in.kb, in.vb, c->d_flags);
        if (st.read().overflow) { t.stop(); break; }
        st.gather(out);
        t.stop();
        HIP_TRY(hipStreamSynchronize(c->stream));
        resolve_big_counts<K>(c, *out, in.ka, in.va, in.run_off, in.in_bigs);
        c->stats.seg_merges++;
        return true;
    }
    return false;
}

// The general way: the concatenation sorted, equal keys summed.
template <class K>
void merge_by_sort(const MergeInput<K>& in, Run* out)
{
    goss_gpu_ctx* c = in.c;
    bool in_b = radix_sort<K, true>(c, in.ka, in.kb, in.va, in.vb, in.total, key_digits(c));
    PhaseTimer t(c, GOSS_T_REDUCE, in.total);
    *out = reduce_runs<K>(c, in_b ? in.kb : in.ka, in_b ? in.vb : in.va, in.total, in_b ? in.ka : in.kb, &in.in_bigs);
    t.stop();
}

// Merge all runs into one (concatenate, sort pairs, sum equal keys).
template <class K>
void merge_runs(goss_gpu_ctx* c)
{
    if (c->build.runs.size() <= 1) return;
    bool all_rep = true, any_rep = false;
    for (auto& r : c->build.runs) { all_rep = all_rep && r.rep; any_rep = any_rep || r.rep; }
    if (any_rep && !all_rep)
    {
        const size_t nr = c->build.runs.size();
        for (size_t i = 0; i < nr; ++i)
            if (c->build.runs[i].rep)
            {
                if (c->mode == GOSS_MODE_GRAPH) expand_graph_run<K>(c, i);          // (appends the reverse complements as a run of their own)
                else if constexpr (std::is_same<K, Key1>::value) canonicalize_run<K>(c, c->build.runs[i]);
                else throw StatusError{GOSS_ERR_STATE, "a two-word run in representative space"};
            }
    }
    const bool rep_out = all_rep;
    uint64_t total = 0;
    for (auto& r : c->build.runs) total += r.m;
    {
        // two copies of all entries + segment tables; low-duplication inputs do not shrink
        const uint64_t need = 2 * total * (sizeof(K) + 4) + (512ULL << 20);
        if (c->arena.avail() < need) grow_arena(c, need);
    }
    ArenaScope scope(c->arena);
    MergeInput<K> in;
    in.c = c; in.total = total; in.nruns = (uint32_t)c->build.runs.size();
    in.ka = (K*)c->arena.temp(total * sizeof(K));
    in.kb = (K*)c->arena.temp(total * sizeof(K));
    in.va = (uint32_t*)c->arena.temp(total * 4);
    in.vb = (uint32_t*)c->arena.temp(total * 4);
    uint64_t off = 0;
    for (auto& r : c->build.runs)
    {
        HIP_TRY(hipMemcpyAsync(in.ka + off, r.keys, r.m * sizeof(K), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(in.va + off, r.counts, r.m * 4, hipMemcpyDeviceToDevice, c->stream));
        in.run_off.push_back(off);
        in.in_bigs.push_back(r.big);
        off += r.m;
    }
    in.run_off.push_back(off);
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the old runs' permanent storage is dead now: rewind the permanent end to the first run
    c->arena.lo = (uint64_t)((uint8_t*)c->build.runs.front().keys - c->arena.base);
    c->build.runs.clear();

    Run r{nullptr, nullptr, 0};
    bool merged = false;
    if constexpr (std::is_same<K, Key2>::value) merged = merge_by_table(in, &r);
    if (!merged && !merge_by_segments(in, &r)) merge_by_sort(in, &r);
    r.rep = rep_out;
    c->build.runs.push_back(r);
}
