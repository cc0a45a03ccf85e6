// chunk_loop.hpp -- a push cut into chunks that fit the arena, and one chunk counted into a run.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, after fused_path.hpp, which a chunk tries first).
#pragma once

// Process window starts [0, nstarts) of a device-resident source (bytes or packed: navail readable positions,
// navail >= nstarts; records: navail 0): extract -> sort -> reduce -> append a run.
template <class K>
void process_chunk(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail)
{
    const uint32_t S = c->mode == GOSS_MODE_GRAPH ? 2 : 1;
    const uint64_t cap = nstarts * S;              // upper bound on keys
    ArenaScope scope(c->arena);
    // the fused path wants room for its bucket regions (expected keys + slack): up to cap/8 more
    // slots in the first buffer when the arena can spare them beyond the two buffers and the
    // partition / segment tables
    uint64_t ka_slots = cap, kb_slots = cap;
    auto full_slots = [&](uint64_t basis) {
        ka_slots = basis; kb_slots = basis;
        const uint64_t extra = basis / 8 + 256 * 16;
        const uint64_t need = (2 * basis + extra) * sizeof(K) + basis / 2 + (uint64_t)(1u << kSegBits) * kSegLimit * 12 + (64u << 20);
        if (c->arena.avail() >= need) ka_slots = basis + extra;
    };
    bool reduced = false;
    if (c->knobs.fused && nstarts >= c->knobs.fused_min)
    {
        // (strand pairs: ONE key per window of a graph on the fused path -- what chunk_capacity cut the chunk for; the
        // sequence a declined chunk falls back to emits both strands and gets its buffers then, below)
        const uint64_t capf = c->mode == GOSS_MODE_GRAPH && c->knobs.graph_rep ? nstarts : cap;
        // a chunk whose sample is a set of slices (not the whole chunk): buffers for the expected
        // number of keys -- bucket regions with 6 % of slack, sub-regions with 13 %
        if (c->valid_frac < 0.97 && nstarts > kValidSizingMin)
        {
            // (+ the blocks the first level's workgroups hold in every region -- 256 regions x 768 workgroups x two blocks
            // of up to 256 slots: an eighth of a chunk of 0.8 G windows, which the slack alone did not cover -- every
            // staged chunk of a FASTQ build was sampled twice, 2 x 2 ms of joint histogram among it)
            ka_slots = std::min<uint64_t>(cap, (uint64_t)((double)capf * c->valid_frac * kValidSlackA) + (1u << 20) + std::min<uint64_t>(capf / 8, 104u << 20));
            kb_slots = std::min<uint64_t>(cap, (uint64_t)((double)capf * c->valid_frac * kValidSlackB) + (8u << 20));
            reduced = ka_slots < cap || kb_slots < cap;
        }
        if (!reduced) { full_slots(capf); reduced = capf < cap; }
    }
    K* ka = (K*)c->arena.temp(ka_slots * sizeof(K));
    K* kb = (K*)c->arena.temp(kb_slots * sizeof(K));
    int frc = process_chunk_fused<K>(c, src, nstarts, navail, ka, ka_slots, kb, kb_slots);
    if (frc == kFusedDone) { if (reduced) c->stats.valid_sized_chunks++; return; }
    if (reduced)
    {
        c->stats.valid_resizes++;
        // the unfused kernels (and a fused retry) want one slot per window start
        scope.rewind();
        c->valid_frac = 1.0;
        full_slots(cap);
        ka = (K*)c->arena.temp(ka_slots * sizeof(K));
        kb = (K*)c->arena.temp(kb_slots * sizeof(K));
        if (frc == kFusedNeedFull && process_chunk_fused<K>(c, src, nstarts, navail, ka, ka_slots, kb, kb_slots) == kFusedDone) return;
    }
    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, sizeof(ExtractCounters), c->stream));
    {
        PhaseTimer t(c, GOSS_T_EXTRACT, nstarts);
        // (a packed string outside the fused path -- a small input, or the sequence a chunk falls back to: the plain
        // kernels read bytes, and this chunk's are made here; released with the chunk's other temporaries)
        extract_dispatch<K>(c, src.packed() ? pk_unpack_temp(c, src, navail) : src, nstarts, navail, ka, false);
        t.stop();
    }
    ExtractCounters* h = (ExtractCounters*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(h, c->d_ctr, 16 /* keys_out, windows */, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n = h->keys_out;
    const uint64_t nwin = n / S;              // S keys per valid window
    if (n)
    {
        Run r = count_keys<K>(c, ka, kb, n);
        c->build.runs.push_back(r);
    }
    c->build.windows += nwin;           // only once the chunk has succeeded (it may be retried)
    c->build.keys_total += n;
}

// Largest number of window starts one chunk may cover with the memory currently free.
// optimistic: size the chunk for the segment-hash path (two key buffers + look-back status;
// its output is bounded by kSegCount * kSegLimit entries).  If a chunk then needs the full
// sort with a large output and runs out of memory, push_source halves it and retries.
uint64_t chunk_capacity(goss_gpu_ctx* c, bool optimistic)
{
    const uint64_t ksz = c->words * 8;
    // (keys per window: two for a graph -- but ONE where the fused path counts strand pairs (round 4) and makes the other
    // strand from the counted pairs: sized for two, C4's chunks were half of what the arena holds, seven where four do;
    // a chunk the fused path declines after all asks for its full buffers and is cut in halves if they are not there)
    const uint32_t S = c->mode == GOSS_MODE_GRAPH && !(optimistic && c->knobs.graph_rep && c->knobs.fused) ? 2 : 1;
    uint64_t avail = c->arena.avail();
    double per_key;
    if (optimistic)
    {
        const uint64_t fixed = (uint64_t)(1u << kSegBits) * kSegLimit * (ksz + 4) + (256u << 20);
        if (avail <= fixed) return 0;
        avail -= fixed;
        per_key = 2.0 * ksz + 0.6;
        if (c->valid_frac < 0.97) per_key = (kValidSlackA + kValidSlackB) * c->valid_frac * ksz + 0.6;
    }
    else
    {
        // per key: two key buffers + histogram table + worst-case output (keys, counts, starts)
        per_key = 2.0 * ksz + 1.2 + (ksz + 12.0);
    }
    uint64_t keys = (uint64_t)((double)avail * 0.95 / per_key);
    uint64_t starts = keys / S;
    if (optimistic && c->valid_frac < 0.97 && starts <= kValidSizingMin + 4096)
        starts = (uint64_t)((double)avail * 0.95 / (2.0 * ksz + 0.6)) / S;     // such chunks get full buffers
    starts &= ~4095ULL;
    return starts;
}

// Share of the window starts of a pushed string that begin a valid window, estimated from 64 MB of
// evenly spread slices: a non-base removes at most `len` windows.  One point of margin; the
// fused path checks the figure against its own sample and asks for full buffers when it was low.
double estimate_valid_fraction(goss_gpu_ctx* c, const ReadSrc& d, uint64_t nbytes)
{
    constexpr uint32_t kSlice = 16384;
    constexpr uint64_t kSlices = 4096;
    const uint64_t skip = d.to_next16();
    if (nbytes < skip + 2 * kSlices * kSlice) return 1.0;
    const uint64_t stride = ((nbytes - skip - kSlice) / (kSlices - 1)) & ~15ULL;
    const ReadSrc::Launch al = d.advance(skip).launch();          // (the first whole sixteen: mis 0)
    Scoped<bool> mute(&c->mute_timing, true);
    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, 16, c->stream));
    with_bool(d.packed(), [&](auto pk) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(nonbase_sample_kernel<decltype(pk)::value>), dim3(1024), dim3(kTB), 0, c->stream,
                           decltype(pk)::value ? (const uint8_t*)al.bad : al.base, kSlices, stride, kSlice, (unsigned long long*)c->d_ctr);
    });
    unsigned long long* h = (unsigned long long*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(h, c->d_ctr, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[1] == 0) return 1.0;
    const double f = 1.0 - (double)h[0] / (double)h[1] * (double)c->len + 0.01;
    return std::min(1.0, std::max(0.05, f));
}

// One push, counted in chunks: `n` bytes / positions of a base string, or `n` super-k-mer records (kernels_route.hpp),
// which count like a string of bases -- a "window start" being one of a record's 16 window slots.  nwindows (records;
// 0 = unknown) sizes the key buffers where a base string is sampled for its share of valid windows.
template <class K>
void push_source(goss_gpu_ctx* c, const ReadSrc& src, uint64_t n, uint64_t nwindows = 0)
{
    const bool recs = src.records();
    if (recs ? n == 0 : n < c->len) return;
    ensure_arena(c);
    const uint64_t nstarts_total = recs ? n * rec_slots(c) : n - c->len + 1;
    Scoped<double> frac(&c->valid_frac, 1.0);          // (this push's share, from here on; 1.0 again behind it)
    if (c->knobs.size_by_valid && c->knobs.fused && c->path == 0 && nstarts_total > kValidSizingMin)
    {
        if (recs) { if (nwindows) c->valid_frac = std::min(1.0, std::max(0.05, (double)nwindows / (double)nstarts_total + 0.01)); }
        else
        {
            c->valid_frac = estimate_valid_fraction(c, src, n);
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: valid windows per window start, estimated: %.3f\n", c->valid_frac);
        }
    }
    uint64_t done = 0;
    uint64_t limit = 0;                 // chunk size cap after an out-of-memory retry
    // (staging buffers are outside the arena: growing it moves nothing the bases live in)
    while (done < nstarts_total)
    {
        const bool optimistic = use_segment_path<K>(c);
        uint64_t capn = chunk_capacity(c, optimistic);
        if (capn < 4096) capn = chunk_capacity(c, false);
        if (capn < 4096)
        {
            // try to make room by merging what we have
            if (c->build.runs.size() > 1) { merge_runs<K>(c); capn = chunk_capacity(c, false); }
            if (capn < 4096 && grow_arena(c, 0)) capn = chunk_capacity(c, false);
            if (capn < 4096) throw StatusError{GOSS_ERR_OOM, "HBM budget too small for one chunk"};
        }
        if (limit && capn > limit) capn = limit;
        // equal chunks rather than full ones and a small remainder: a remainder covers the
        // genome too thinly for the segment path and would go through the full sort
        {
            const uint64_t left = nstarts_total - done;
            if (left > capn)
            {
                const uint64_t parts = (left + capn - 1) / capn;
                capn = std::min<uint64_t>(capn, ((left + parts - 1) / parts + 4095) & ~4095ULL);
            }
        }
        const uint64_t ns = std::min(capn, nstarts_total - done);          // (a multiple of 4096 slots = whole records, but for the last)
        const uint64_t navail = recs ? 0 : std::min(n - done, ns + c->len - 1);
        const uint64_t lo0 = c->arena.lo;
        const size_t runs0 = c->build.runs.size();
        // (behind this chunk of a base string: the rest of this push and what the push's own caller has said lies behind
        // IT; a push of records leaves the figure as it is)
        Scoped<uint64_t> more(&c->more_starts, c->more_starts + (recs ? 0 : nstarts_total - done - ns));
        try
        {
            process_chunk<K>(c, src.advance(done), ns, navail);
        }
        catch (const StatusError& e)
        {
            if (e.status != GOSS_ERR_OOM || ns <= 8192) throw;
            // undo the partial chunk; retry it in a larger arena if the budget may grow, else in halves
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->arena.lo = lo0;               // (the temporaries went with process_chunk's scope)
            c->build.runs.resize(runs0);
            if (grow_arena(c, 0)) continue;
            limit = (ns / 2) & ~4095ULL;
            continue;
        }
        done += ns;
        // keep the accumulated runs from eating the budget
        uint64_t run_bytes = 0;
        for (auto& r : c->build.runs) run_bytes += r.m * (c->words * 8 + 4);
        if (c->build.runs.size() > 1 && run_bytes > c->arena.size / 4)
        {
            // merging needs two more copies of the runs: possible now, or after growing; else the
            // runs wait for finish
            if (c->arena.avail() >= 2 * run_bytes + (512ULL << 20) || grow_arena(c, 2 * run_bytes + (512ULL << 20))) merge_runs<K>(c);
        }
    }
}
// (the key width is the context's)
void push_source(goss_gpu_ctx* c, const ReadSrc& src, uint64_t n, uint64_t nwindows = 0)
{
    if (c->words == 1) push_source<Key1>(c, src, n, nwindows); else push_source<Key2>(c, src, n, nwindows);
}
