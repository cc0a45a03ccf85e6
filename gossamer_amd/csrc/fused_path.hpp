// fused_path.hpp -- extraction fused with the first partition level, and the counting that follows it.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, once the helpers it calls are defined): the form
// a chunk is counted in (FusedForm, choose_form), one function per stage, and the driver process_chunk_fused.
//
// Two forms.  LSD (any number of partition digits): the fused kernel partitions on the lowest
// partition digit into 256 bucket regions, the remaining digits are look-back passes (the first
// of them reads the regions).  MSD (exactly two digits, the common case): the fused kernel
// partitions on the HIGH digit and the second pass places the keys of region b by their LOW digit
// into 65 536 sub-regions -- the segments of the counting kernel -- with atomic cursors: no
// look-back chain and no digit histograms at all.  Region and sub-region sizes come from a sample
// of the input (the whole chunk when it is small), with 5 / 6 standard deviations of slack.
#pragma once

// process_chunk_fused returns kFusedDone, kFusedDeclined (the caller runs the unfused sequence on the same, untouched
// input) or kFusedNeedFull (the key buffers were sized for fewer valid windows than the sample shows: the caller retries
// with buffers of one key per window start).  Inside this file a stage also answers kFusedGoOn (nothing to report: the
// driver takes its next step) and the driver kFusedAgain (context adjusted: the chunk once more from the top).
enum { kFusedDeclined = 0, kFusedDone = 1, kFusedNeedFull = 2, kFusedGoOn = -1, kFusedAgain = -2 };
constexpr uint32_t kFusedGrid = 256 * GOSS_E1_OCC;                         // workgroups of extract1_part_kernel: 3 per CU (52 KB of LDS each)
#ifndef GOSS_FUSED_NKEYS2
#define GOSS_FUSED_NKEYS2 14          // keys per thread of extract2_part_kernel (tile of 3584 keys + carry = 70 KB of LDS)
#endif
#ifndef GOSS_FUSED_GRID2
#define GOSS_FUSED_GRID2 512
#endif
constexpr uint32_t kFusedGrid2 = GOSS_FUSED_GRID2;                        // ... of extract2_part_kernel: 2 per CU (75 KB)
constexpr double kValidSlackA = 1.06, kValidSlackB = 1.17;   // key buffer slots per expected key (bucket regions; sub-regions with their six sigma each: 1.149 measured on C4's two-word keys)
constexpr uint64_t kValidSizingMin = 640u << 20;             // window starts: smaller chunks are sampled whole into a full buffer

// ---- the form ----------------------------------------------------------------------------------
// How a chunk is counted: chosen once (choose_form) from the distinct-key estimate; a later stage that finds the form
// does not do -- sub-regions that do not fit, a table that overflowed -- derives the next one from it.
struct FusedForm {
    enum Table {
        kSmall,      // the 4096-slot table of whole keys
        kBig,        // the big table, every 16-bit segment shared by 2^rounds workgroups
        kWide,       // two-word keys: the 6144-slot table
        k96,         // two-word keys: 96-bit remainders in 16-byte slots (the second level writes 12-byte records)
        kRem32       // one-word keys: 32-bit remainders below an (8 + r32_bits)-bit prefix, segments split r32_split bits further
    };
    Table table = kSmall;
    uint32_t segbits = kSegBits;         // segment bits of the forms that count whole keys
    bool msd = false;                    // the two-level form (sub-regions); else look-back passes
    uint32_t rounds = 0;                 // kBig
    uint32_t r32_bits = 0, r32_split = 0, rbits32 = 0;          // kRem32: second-level bits, third-level bits, bits of a remainder (before the squeeze)
    int r32_slots = 0;                   // ... slots of its counting table
    bool squeeze = false, narrow = false;          // ... the always-clear bit of an odd k-mer's representative dropped / remainder + digit between the levels

    bool rem32() const { return table == kRem32; }
    uint32_t r32_regions() const { return 256u << r32_bits; }
    // what segment_reduce is told
    SegCount seg_count() const
    {
        switch (table)
        {
            case kBig: return {SegTable::Big, rounds};
            case kWide: return {SegTable::Wide, 0};
            case k96: return {SegTable::Rem96Packed, 0};
            default: return {SegTable::Small, 0};
        }
    }
    // the 32-bit sub-regions do not fit: 8-byte keys in 16-bit segments
    FusedForm eight_byte() const { FusedForm f; f.segbits = kSegBits; f.msd = msd; return f; }
    // the 8-byte sub-regions do not fit: look-back passes over the same segments
    FusedForm one_level() const { FusedForm f = *this; f.msd = false; return f; }
    // a table of whole one-word keys overflowed: 8192 slots, then 2 and 4 workgroups per segment
    FusedForm larger_table() const { FusedForm f = *this; f.rounds = table == kBig ? rounds + 1 : 0; f.table = kBig; return f; }
    // a table of remainders overflowed: the next larger one
    FusedForm larger_r32_table() const { FusedForm f = *this; f.r32_slots = r32_slots < 4096 ? 4096 : 2 * r32_slots; return f; }
};

template <class K>
FusedForm choose_form(const goss_gpu_ctx* c, uint32_t keybits, uint64_t m_est, bool graph_mode, bool canon_l1)
{
    constexpr bool kOne = std::is_same<K, Key1>::value;
    const uint64_t limit = SegCfg<K>::kLimit;
    FusedForm f;
    f.segbits = kSegBits;
    while (f.segbits < (uint32_t)kSegBitsMax && (m_est >> f.segbits) > limit * 3 / 4) f.segbits += 4;
    const bool big_ok = c->knobs.fused_msd && c->knobs.big_table && f.segbits > (uint32_t)kSegBits;
    // one-word keys: between 3/4 of the small table and 3/4 of the big one per 16-bit segment, the
    // two-level form with the big counting table saves the third partition digit
    // (up to 4 workgroups sharing a segment, each counting the keys of one value of the next bits)
    if (kOne && big_ok && keybits >= (uint32_t)kSegBits + 8 + 2)
        for (int r = std::max(0, c->knobs.big_rounds_min); r <= kBigRoundsMax; ++r)
            if ((m_est >> (kSegBits + r)) <= (uint64_t)kSegBigLimit * 17 / 20) { f.segbits = kSegBits; f.table = FusedForm::kBig; f.rounds = (uint32_t)r; break; }   // (an overflow costs one more counting pass, no more)
    // two-word keys: the 4096-slot table, up to two workgroups per segment (a pass over 16-byte
    // keys costs more than one over 8-byte keys)
    // two-word keys whose bits below a 16-bit prefix fit 96: 16-byte slots, 8192 of them
    if (!kOne && big_ok && c->knobs.table96 && keybits - kSegBits <= 96 && c->knobs.big_rounds_min == 0 && (m_est >> kSegBits) <= (uint64_t)kSeg96Limit * 3 / 4)
    { f.segbits = kSegBits; f.table = FusedForm::k96; }
    else if (!kOne && big_ok)
        for (int r = std::max(0, c->knobs.big_rounds_min); r <= std::min(1, kBigRoundsMax); ++r)
        {
            if ((m_est >> (kSegBits + r)) <= (uint64_t)kSegBigLimit2 * 3 / 4) { f.segbits = kSegBits; f.table = FusedForm::kBig; f.rounds = (uint32_t)r; break; }
            // between the two: the 6144-slot table, still one workgroup (and one read) per segment
            if (r == 0 && c->knobs.wide_table && (m_est >> kSegBits) <= (uint64_t)kSegWideLimit2 * 3 / 4) { f.segbits = kSegBits; f.table = FusedForm::kWide; break; }
        }
    // one-word keys whose bits below a 17- to 20-bit prefix fit 32 (an odd-length k-mer's strand representative has one
    // bit that is always clear): 9 to 12 bits at the second level, which then writes -- and the counting kernel reads --
    // 4-byte remainders instead of 8-byte keys (kernels_partition.hpp: subpart32_kernel).  The fewest bits whose
    // segments hold the estimated distinct keys in an LDS table (2048 slots at 9 bits when they do, else 4096).
    if (kOne && c->knobs.rem32 && c->knobs.fused_msd && c->knobs.big_rounds_min == 0)
    {
        // (second-level bits, third-level bits) in the order of what they cost on C2's 12.6 G keys: the second level 31 ms
        // with 9 bits and 46 with 10 (shorter runs), the third level ~30 ms whatever it splits into -- so ten bits before a
        // third level, and nine bits + a third level before ten + a third level.  The first pair whose remainder fits 32
        // bits and whose segments hold the estimated distinct keys in an LDS table (2048 slots at (9, 0) when they
        // do, else 4096 with a quarter to spare).
        // Reads with errors (round 5): where ten bits and the 4 096-slot table do not do, the tables of 8 192 and 16 384 slots
        // (512 / 1 024 threads) come BEFORE a third level -- that level is a pass over all keys (~30 ms on C2's 12.6 G), the
        // larger table the same counting on fewer, longer segments.  Third element: the largest table of the candidate.
        static const uint32_t order[][3] = {{9, 0, 4096}, {10, 0, 4096}, {10, 0, 8192}, {10, 0, 16384}, {9, 1, 4096}, {9, 2, 4096}, {9, 3, 4096}, {9, 4, 4096},
                                            {10, 1, 4096}, {10, 2, 4096}, {10, 3, 4096}, {10, 4, 4096}};
        for (const auto& cand : order)
        {
            const uint32_t b2 = cand[0], b3 = cand[1], table = cand[2];
            if (table > 4096u && c->knobs.rem32_slots) continue;          // (a forced table: the candidates' own do not apply)
            if (b2 < c->knobs.rem32_bits_min || b3 < c->knobs.rem32_split_min) continue;
            if (keybits < 8 + b2 + 8) continue;
            const uint32_t rb = keybits - 8 - b2;
            const bool sq = !graph_mode && !canon_l1 && (c->len & 1u) && rb == 33;
            if (rb - (sq ? 1u : 0u) > 32 || rb - (sq ? 1u : 0u) < b3 + 8) continue;
            const uint64_t per = m_est >> (8 + b2 + b3);
            int slots = 0;
            if (c->knobs.rem32_slots) slots = per <= (uint64_t)(c->knobs.rem32_slots / 4 * 3) || (b2 == 10 && b3 == (uint32_t)kSub32SplitMax) ? c->knobs.rem32_slots : 0;
            // (buckets of four: what is not at home costs a second look, and at a load of 0.37 that is 1.5 % of the keys, at
            // 0.19 a per-mille -- the small table only where it stays that empty)
            else if (per <= (c->knobs.r32_small_max ? c->knobs.r32_small_max : 400u) && b3 == 0 && b2 == (uint32_t)kSub32BitsMin) slots = 2048;
            else if (per <= (uint64_t)table / 4 * 3 * 3 / 4) slots = (int)table;
            if (!slots) continue;
            f = FusedForm{};
            f.table = FusedForm::kRem32; f.segbits = kSegBits;
            f.r32_slots = slots; f.r32_bits = b2; f.rbits32 = rb; f.squeeze = sq; f.r32_split = b3;
            f.narrow = c->knobs.narrow;          // remainder + digit between the two levels, 5.33 bytes a key
            break;
        }
    }
    f.msd = c->knobs.fused_msd && f.segbits == 16;
    return f;
}

// ---- what the stages share ---------------------------------------------------------------------
// The chunk as process_chunk_fused was handed it, and what the context says about it.  In graph mode the path wants both
// strands of every window (ReverseComplementAdapter.hh:34-55), and both always come together: it counts ONE strand
// representative per window -- half the keys through the partition and the tables -- and the run is expanded into both
// strands after counting (expand_graph_run).  Inside this file such a chunk is a k-mer-set chunk of (k+1)-mers in
// representative space.
template <class K>
struct FusedChunk {
    static constexpr bool kOne = std::is_same<K, Key1>::value;          // one-word keys
    goss_gpu_ctx* c;
    ReadSrc src;
    uint64_t nstarts, navail;
    K* ka; uint64_t ka_slots;
    K* kb; uint64_t kb_slots;
    uint32_t keybits;
    bool rep_graph;          // a graph build counted as strand pairs
    bool rep_kmer;           // one-word k-mer sets: representatives, canonical forms after counting
    bool use_rep;
    bool graph_mode;         // both strands of every window are keys
    bool reduced;            // the key buffers were sized from the estimated share of valid windows (process_chunk)
    std::chrono::steady_clock::time_point t_begin;

    int decline(const char* why) const
    {
        if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: fused path declined (%s), %llu window starts\n", why, (unsigned long long)nstarts);
        return (int)kFusedDeclined;
    }
    void lap(const char* what) const
    {
        if (!c->knobs.debug) return;
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::fprintf(stderr, "libgossgpu: fused path: %-28s at %8.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    }
};

// The sample: nslices slices of slice_starts window starts, slice_stride apart; ns keys came out of it.
struct FusedSample {
    uint64_t super = 0;          // window starts per super-tile of the plain kernels
    uint64_t nslices = 0, slice_starts = 0, slice_stride = 0;
    uint64_t ns = 0;             // keys of the sample
    bool exact = false;          // the sample is the chunk
    double scale = 1.0;          // window starts of the chunk per window start of the sample
    uint64_t n_exp = 0;          // expected number of keys of the chunk
};

// ---- 1. the sample -----------------------------------------------------------------------------
// Slices spread evenly over the chunk, extracted with the plain kernel.  The two-level form needs the joint histogram of
// two digits (65 536 bins), hence a larger sample: 1/64 of the chunk but at least 160 M window starts; a chunk of up to
// 640 M window starts is sampled whole (exact sizes, +4 % extraction work at most).
template <class K>
int plan_sample(const FusedChunk<K>& ch, FusedSample* sm)
{
    constexpr bool kOne = FusedChunk<K>::kOne;
    const goss_gpu_ctx* c = ch.c;
    const uint64_t nstarts = ch.nstarts;
    const bool want_msd = c->knobs.fused_msd;
    uint64_t sample_starts = nstarts <= (16u << 20) ? nstarts : (4u << 20);
    if (want_msd) sample_starts = nstarts <= (640u << 20) ? nstarts : std::max<uint64_t>(160u << 20, nstarts / 64);
    // keys that the 32-bit-remainder forms take (by their width): half the sample -- their sub-regions are 4-byte slots,
    // which have the room for the wider six-sigma margins of a smaller sample (22 % instead of 15 % on C2), and the
    // sample's extraction, spectrum and joint histogram are 3 ms of a 97 ms step
    {
        bool width_ok = false;
        if (kOne && c->knobs.rem32 && ch.keybits >= 8 + 9 + 8)
            for (uint32_t b2 = kSub32BitsMin; b2 <= (uint32_t)kSub32BitsMax; ++b2)
            {
                const uint32_t rb = ch.keybits - 8 - b2;
                const bool sq = (ch.rep_kmer || ch.rep_graph) && (c->len & 1u) && rb == 33;
                width_ok = width_ok || rb - (sq ? 1u : 0u) <= 32;
            }
        if (want_msd && width_ok && nstarts > (640u << 20)) sample_starts = std::max<uint64_t>(80u << 20, nstarts / 128);
    }
    // slices are whole super-tiles of the plain kernel (32 768 window starts) and lie a multiple
    // of 16 bytes apart, so that ONE strided launch extracts them all
    // window starts per super-tile of the plain kernels: extract1_kernel<0,16,8> / <1,8,8>, extract2_kernel<0,8,8> / <1,4,8>
    sm->super = 8ULL * kTB * (kOne ? (ch.graph_mode ? 8 : 16) : (ch.graph_mode ? 4 : 8));
    // a slice is ONE super-tile (~217 reads of 150 bp): thousands of slices follow a drifting
    // k-mer distribution (sorted inputs) far better than a few long ones
    sm->nslices = sample_starts >= nstarts ? 1 : std::max<uint64_t>(64, sample_starts / sm->super);
    sm->slice_starts = sample_starts >= nstarts ? nstarts : sm->super;
    if (sm->nslices > 1 && nstarts < 4 * sm->nslices * sm->slice_starts) return ch.decline("chunk smaller than the sample");
    // key buffers sized from the estimated share of valid windows (process_chunk): they must hold
    // the sample whatever it contains
    const uint64_t kps = ch.graph_mode ? 2 : 1;
    if (ch.reduced && (sm->nslices == 1 || sm->nslices * sm->slice_starts * kps > std::min(ch.ka_slots, ch.kb_slots))) return (int)kFusedNeedFull;
    sm->slice_stride = sm->nslices > 1 ? ((nstarts - sm->slice_starts) / (sm->nslices - 1)) & ~15ULL : 0;
    sm->exact = sm->nslices == 1;
    sm->scale = (double)nstarts / (double)(sm->nslices * sm->slice_starts);
    return kFusedGoOn;
}

// The slices of one-word keys from bytes or a packed string, with the plain kernel told where they lie.
template <int MODE, int P, bool REP>
void launch_sample1(goss_gpu_ctx* c, const ReadSrc::Launch& in, uint64_t nstarts, uint64_t navail, Key1* ka, uint64_t nsuper, uint64_t slice_tiles,
                    uint64_t slice_stride)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nsuper, 2048);
    with_bool(in.kind == ReadSrc::Packed, [&](auto pk) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(extract1_kernel<MODE, P, 8, 8, REP, decltype(pk)::value>), dim3(grid), dim3(kTB), 0, c->stream, in.base, in.mis,
                           nstarts, navail, c->len, ka, c->d_ctr, 0xFFFFFFFFu, nsuper, slice_tiles, slice_stride, in.bad);
    });
}

// The sample's keys into ch.ka; returns how many.  rep: one-word k-mer sets in strand-representative space (what the
// fused kernel counts in, unless the first level computes canonical forms).
template <class K>
uint64_t extract_sample(const FusedChunk<K>& ch, const FusedSample& sm, bool rep)
{
    constexpr bool kOne = FusedChunk<K>::kOne;
    goss_gpu_ctx* c = ch.c;
    const ReadSrc& src = ch.src;
    const uint64_t nstarts = ch.nstarts, navail = ch.navail, nslices = sm.nslices, slice_starts = sm.slice_starts, slice_stride = sm.slice_stride;
    K* ka = ch.ka;
    Scoped<bool> mute(&c->mute_timing, true);
    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, sizeof(ExtractCounters), c->stream));
    {
        // (a packed string whose sample is the whole chunk: the slice kernels below, told to take every tile in turn --
        // they have a packed form, the plain kernels behind extract_dispatch read bytes)
        const bool whole_pk = nslices == 1 && src.packed();
        const uint64_t slice_tiles = whole_pk ? 0 : slice_starts / sm.super, nsuper = whole_pk ? (nstarts + sm.super - 1) / sm.super : slice_tiles * nslices;
        if (nslices == 1 && !whole_pk) extract_dispatch<K>(c, src, nstarts, navail, ka, ch.use_rep && rep);
        else if (!kOne && src.records())
        {
            // slices of a super-tile's window slots of two-word records
            const uint64_t P = rec_slots(c);
            const uint64_t slice_groups = std::max<uint64_t>(1, slice_starts / P / kRecGroup);
            launch_extract_records2(c, (const SkRec2*)src.bytes, nstarts / P, (Key2*)ka, slice_groups * nslices, slice_groups, slice_stride / P,
                                    ch.rep_graph && rep);
        }
        else if constexpr (!kOne)
        {
            if (ch.graph_mode) launch_extract2<1, 4, 8>(c, src, nstarts, navail, ka, slice_tiles, slice_stride, nsuper);
            else launch_extract2<0, 8, 8>(c, src, nstarts, navail, ka, slice_tiles, slice_stride, nsuper, ch.rep_graph && rep);
        }
        else if (src.records())
        {
            // slices of a super-tile's window slots = 2048 records each, in strand-representative space for k-mer sets
            const uint64_t P = rec_slots(c);
            const uint64_t slice_groups = slice_starts / P / kRecGroup;
            launch_extract_records(c, (const SkRec*)src.bytes, nstarts / P, (Key1*)ka, slice_groups * nslices, slice_groups, slice_stride / P,
                                   ch.use_rep && rep);
        }
        else if (ch.graph_mode) launch_sample1<1, 8, false>(c, src.launch(), nstarts, navail, ka, nsuper, slice_tiles, slice_stride);
        // strand representatives: the key space the fused kernel counts in
        else if (rep) launch_sample1<0, 16, true>(c, src.launch(), nstarts, navail, ka, nsuper, slice_tiles, slice_stride);
        else launch_sample1<0, 16, false>(c, src.launch(), nstarts, navail, ka, nsuper, slice_tiles, slice_stride);
    }
    c->extract_hist_shift = 0xFFFFFFFFu;
    ExtractCounters* hcs = (ExtractCounters*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(hcs, c->d_ctr, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return (uint64_t)hcs->keys_out;
}

// ---- the key space -----------------------------------------------------------------------------
// Whether the first level of this chunk computes gossamer's canonical form itself.  The only stage that writes
// c->build.space_choice.
// One-word k-mer sets are counted as strand representatives and mapped to gossamer's canonical form afterwards -- a
// re-ordering of the DISTINCT keys (0.06 ms per million), cheap beside two FNV hashes per WINDOW in the first level
// (+ ~2.4 ms per 10^9 windows) while distinct keys are few.  Reads with many errors turn that round (2e9 distinct
// 25-mers of 12.6e9 windows: 116 ms of re-ordering against ~30 ms of hashing): from 5 % distinct keys per window on
// (kCanonL1At) the first level computes the canonical form itself and the run needs no re-ordering.
// A chunk that is ONE OF SEVERAL shares the re-ordering with the others -- the runs are merged in representative
// space and re-ordered once -- so what counts is the whole build: its windows W (what the caller said it will push,
// goss_gpu_expect_bases; else what has been counted plus this chunk, times four when more is known to follow) and
// its distinct keys D = the chunk's frequent keys (more of the same input mostly brings THEM again) + its keys of
// multiplicity ~1 scaled to W (every chunk brings its own).  C2 from FASTQ: thirteen chunks of 0.8 G windows each
// see all 10^8 k-mers of the genome (12 % of their windows) -- per chunk that read "canonical", 67 ms of first
// level where representatives take 31, ten second-level bits, a re-ordering per run; of the build's 12.6 G windows
// they are 0.8 %.  Once a chunk has chosen, the chunks that follow count in the same space while its run waits:
// a run in canonical space among runs of representatives sends every one of those through a re-ordering of its own.
inline bool choose_key_space(goss_gpu_ctx* c, bool rep_kmer, uint64_t m_est, uint64_t m_rare, uint64_t n_exp)
{
    bool canon_auto = (double)m_est > kCanonL1At * (double)n_exp;
    if (rep_kmer && c->knobs.canon_l1 == 1)
    {
        if (c->build.space_choice >= 0 && !c->build.runs.empty()) canon_auto = c->build.space_choice == 1;
        else
        {
            const double w_c = (double)n_exp;
            // (what follows: known for the rest of the push being counted; a guess -- three times as much again -- when
            // that push is a staging buffer that filled up under a caller who goes on pushing)
            const double w_push = w_c + (double)c->more_starts * std::min(1.0, c->valid_frac);          // this push, from this chunk on
            double w_all = (double)c->build.windows + w_push * (c->more_follows ? 4.0 : 1.0);
            if (c->build.expect_bases) w_all = std::max(w_all, (double)c->build.expect_bases * std::min(1.0, c->valid_frac));
            const double d_all = (double)(m_est - m_rare) + (double)m_rare * (w_all / w_c);
            canon_auto = d_all > kCanonL1At * w_all;
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: fused path: %.0f distinct keys (%.0f of multiplicity ~1) of %.0f windows here, %.0f of %.0f in all: %s\n",
                                       (double)m_est, (double)m_rare, w_c, d_all, w_all, canon_auto ? "canonical forms in the first level" : "strand representatives");
        }
    }
    const bool canon_l1 = rep_kmer && (c->knobs.canon_l1 == 2 || (c->knobs.canon_l1 == 1 && canon_auto));
    if (rep_kmer && c->knobs.canon_l1 == 1) c->build.space_choice = canon_l1 ? 1 : 0;
    return canon_l1;
}

// ---- 2. histograms of the sample ---------------------------------------------------------------
// Joint over both digits for the two-level form, else of the first partition digit only.
struct SampleHist {
    std::vector<unsigned long long> hh = std::vector<unsigned long long>(256, 0);          // the fused kernel's digit
    std::vector<uint64_t> joint;                         // [high*256 + low], two-level form only
    std::vector<uint64_t> joint17;                       // [high*512 + low9], 32-bit-remainder form
};

template <class K>
SampleHist sample_histograms(const FusedChunk<K>& ch, const FusedForm& form, uint64_t ns)
{
    goss_gpu_ctx* c = ch.c;
    const uint32_t shift = ch.keybits - form.segbits;
    SampleHist h;
    if (form.msd)
    {
        // the sample's joint histogram of both digits (kept out of the per-kernel timing): one pass over the sample
        // with the bins in LDS (a 16-bit partition of the sample + segment bounds took 2.4 ms on C2, this 0.9);
        // 17 bits (four sweeps) for the 32-bit-remainder form, whose pairs of bins are the 16-bit form's
        const uint32_t jbins = form.rem32() ? form.r32_regions() : 65536u;
        unsigned long long* jh = (unsigned long long*)c->arena.temp((uint64_t)jbins * 8);
        HIP_TRY(hipMemsetAsync(jh, 0, (uint64_t)jbins * 8, c->stream));
        {
            Scoped<bool> mute(&c->mute_timing, true);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(joint_hist_kernel<K>), dim3(256), dim3(kJointThreads), 0, c->stream, (const K*)ch.ka, ns,
                               form.rem32() ? form.rbits32 : shift, jh, jbins / 32768u);
        }
        std::vector<uint64_t> ho(jbins);
        HIP_TRY(hipMemcpyAsync(ho.data(), jh, (uint64_t)jbins * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        h.joint.resize(65536);
        if (form.rem32())
        {
            h.joint17.swap(ho);
            const uint32_t fold = form.r32_regions() / 65536u;          // bins of this form per bin of the 16-bit form
            for (uint32_t i = 0; i < 65536; ++i) { uint64_t a = 0; for (uint32_t j = 0; j < fold; ++j) a += h.joint17[i * fold + j]; h.joint[i] = a; }
        }
        else h.joint.swap(ho);
        for (uint32_t i = 0; i < 65536; ++i) h.hh[i >> 8] += h.joint[i];
    }
    else
    {
        unsigned long long* shist = (unsigned long long*)c->arena.temp(256 * 8);
        HIP_TRY(hipMemsetAsync(shist, 0, 256 * 8, c->stream));
        {
            Scoped<bool> mute(&c->mute_timing, true);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(global_hist_kernel<K>), dim3(256), dim3(kTB), 0, c->stream, (const K*)ch.ka, ns, shift, 1u, shist);
        }
        HIP_TRY(hipMemcpyAsync(h.hh.data(), shist, 256 * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return h;
}

// ---- sizing: pure functions of the sample's histograms -----------------------------------------
// Sub-regions of the second buffer (two-level form): expected size + six standard deviations of the sample count.
// Each answers with its table and the slots it needs; `misfit` says why the table cannot be used (nullptr: it can).

// 32-bit-remainder form: 2^17 .. 2^20 sub-regions of 4-byte slots in the second key buffer; every start a multiple of
// four slots (the counting kernel loads 16 bytes per lane).  First slot and capacity of every sub-region.
struct Sub32Regions { std::vector<uint64_t> start; std::vector<uint32_t> cap; uint64_t slots = 0; const char* misfit = nullptr; };
inline Sub32Regions size_sub32_regions(const std::vector<uint64_t>& joint17, const FusedForm& form, const FusedSample& sm, double capscale,
                                       uint64_t ka_slots, uint64_t kb_slots)
{
    const uint32_t regions = form.r32_regions(), digits = 1u << form.r32_bits;
    Sub32Regions s;
    s.start.resize(regions);
    s.cap.resize(regions);
    uint64_t at = 0;
    bool fits = true;
    for (uint32_t i = 0; i < regions; ++i)
    {
        const double h = (double)joint17[i];
        const uint64_t cap = sm.exact ? (((uint64_t)(h * capscale)) + 3) & ~3ULL
                                      : (((uint64_t)(((h + 6.0 * std::sqrt(h + 1.0) + 4.0) * sm.scale + 64.0) * capscale) + 15) & ~15ULL);
        if (cap > 0xFFFF0000ULL) fits = false;
        s.start[i] = at; s.cap[i] = (uint32_t)cap;
        at += cap;
        // (the second level addresses a region's sub-regions with 32-bit offsets from the region's first)
        if ((i & (digits - 1u)) == digits - 1u && at - s.start[i - (digits - 1u)] > 0xFFFF0000ULL) fits = false;
    }
    s.slots = at;
    if (!fits) s.misfit = "a region's sub-regions exceed 32-bit offsets";
    else if (at > 2 * kb_slots) s.misfit = "more slots than the second key buffer has";
    else if (form.r32_split && at > 2 * ka_slots) s.misfit = "more slots than the first key buffer has";          // (the third level writes the remainders into the first buffer)
    return s;
}

// 8-byte form: 65 536 sub-regions of whole keys.
struct Sub8Regions { std::vector<SubTable> table; uint64_t slots = 0; };
inline Sub8Regions size_sub8_regions(const std::vector<uint64_t>& joint, const FusedSample& sm, double capscale)
{
    Sub8Regions s;
    s.table.resize(1);
    uint64_t at = 0;
    for (uint32_t i = 0; i < 65536; ++i)
    {
        const double h = (double)joint[i];
        // exact counts need no slack (and a small chunk cannot afford 65 536 paddings)
        const uint64_t cap = sm.exact ? (uint64_t)(h * capscale)
                                      : (((uint64_t)(((h + 6.0 * std::sqrt(h + 1.0) + 4.0) * sm.scale + 64.0) * capscale) + 15) & ~15ULL);
        s.table[0].start[i] = at; s.table[0].cap[i] = cap;
        at += cap;
    }
    s.slots = at;
    return s;
}

// Bucket regions of the first buffer: expected size of every bucket plus five standard
// deviations of the sample count; whatever room the key buffer has beyond that (up to 25 %)
// is handed out proportionally, so that a mildly non-stationary input still fits.
// Every workgroup of the fused kernel appends to a private block of B slots per bucket and pads the
// unused tail of its last blocks, so a region also needs one block per workgroup; B is the largest
// power of two (one 64-byte granule .. 256 slots) that keeps that padding within 3 % of the keys: a small
// chunk gets fewer workgroups, then smaller blocks.  Workgroups per CU: 3 for one-word keys (52 KB of
// LDS each), 2 for two-word keys (75 KB).
struct BucketRegions {
    GapTable gt{};
    uint32_t grid = 0;           // workgroups of the fused kernel the regions were sized for
    uint32_t blk_log2 = 0;       // log2 of B
    uint64_t super = 0;          // window starts per super-tile of the fused kernel
    bool fits = false;
};
template <class K>
void size_bucket_regions(const std::vector<unsigned long long>& hh, const FusedSample& sm, uint64_t nstarts, bool graph_mode, uint64_t ka_slots,
                         double capscale, uint32_t blk_log2_max, BucketRegions* br)
{
    constexpr bool kOne = std::is_same<K, Key1>::value;
    const uint32_t kGranule = kOne ? 8 : 4;                       // keys per 64 bytes
    br->super = kOne ? (uint64_t)kTB * (graph_mode ? GOSS_E1_NK / 2 : GOSS_E1_NK)
                     : (uint64_t)kTB * (graph_mode ? GOSS_FUSED_NKEYS2 / 2 : GOSS_FUSED_NKEYS2);
    const double pad_budget = 0.03 * (double)sm.n_exp;
    uint32_t fgrid = (uint32_t)std::min<uint64_t>((nstarts + br->super - 1) / br->super, (uint64_t)(kOne ? kFusedGrid : kFusedGrid2));
    fgrid = (uint32_t)std::max(16.0, std::min((double)fgrid, pad_budget / (256.0 * kGranule)));
    uint32_t blk_log2 = kOne ? 3 : 2;
    while (blk_log2 < 8 && (double)fgrid * 256.0 * (double)(2u << blk_log2) <= pad_budget) ++blk_log2;
    if (blk_log2_max) blk_log2 = std::min(blk_log2, std::max(blk_log2_max, kOne ? 3u : 2u));
    br->grid = fgrid; br->blk_log2 = blk_log2;
    const uint64_t B = 1ULL << blk_log2;
    // (a workgroup also holds a reserved block per bucket that it may never open)
    const double blk_extra = (double)fgrid * (double)B * 2.0;
    double base[256], base_sum = 0;
    for (int d = 0; d < 256; ++d)
    {
        const double h = (double)hh[d];
        base[d] = sm.exact ? h + 64.0 : (h + 5.0 * std::sqrt(h + 1.0) + 16.0) * sm.scale + 1024.0;    // exact counts need no slack
        base_sum += base[d];
    }
    double slack = std::min(1.25, ((double)ka_slots - 256.0 * ((double)B + blk_extra)) / base_sum);
    br->fits = !(slack < (sm.exact ? 1.0 : 1.02));
    if (!br->fits) return;
    slack *= capscale;
    uint64_t at = 0;
    for (int d = 0; d < 256; ++d)
    {
        uint64_t cap = ((uint64_t)(base[d] * slack + blk_extra * capscale) + B - 1) & ~(B - 1);
        br->gt.reg_start[d] = at; br->gt.reg_cap[d] = cap;
        at += cap;
    }
}

// ---- 3. extraction that partitions -------------------------------------------------------------
// Run-time choices -> template arguments of the first-level kernels (with_bool, and for the digit histograms): f is
// called with a std::integral_constant of the value.
template <class F> void with_digit_hists(int nh, F&& f)
{
    if (nh == 0) f(std::integral_constant<int, 0>{});
    else if (nh == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}

struct FirstLevelLaunch {
    ReadSrc::Launch in;
    uint64_t nstarts, navail;
    void* ka; PartCounters* pc; const GapTable* dgt;
    uint32_t part_shift; uint64_t nsuper; uint32_t blk_log2, grid;
    int nh;          // digit histograms the kernel takes for the look-back passes behind it (0: two-level form)
};

// One-word keys.  MODE 1: both strands (graph); REPK 0 / 1 / 2: strand representatives of an even / odd k, canonical forms.
// The 32-bit forms of the kernel (FAST) and remainder + digit, twelve keys to a granule, ahead of the 32-bit-remainder
// second level (NARROW: kernels_extract.hpp) exist for the two-level form alone.
template <int MODE, int REPK>
void launch_extract1_part(goss_gpu_ctx* c, const FirstLevelLaunch& a, bool fastk, bool narrow, uint32_t nr_rbits, uint32_t nr_sqbit, uint32_t nr_dmask,
                          uint32_t nr_capg)
{
    with_digit_hists(a.nh, [&](auto nh_c) { with_bool(fastk, [&](auto fast_c) { with_bool(narrow, [&](auto narrow_c) {
        constexpr int NH = decltype(nh_c)::value;
        constexpr bool FAST = NH == 0 && decltype(fast_c)::value, NRW = NH == 0 && decltype(narrow_c)::value;
        if (a.in.kind == ReadSrc::Records)          // (navail: the records)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(extract1_part_kernel<MODE, NH, REPK, true, FAST, NRW>), dim3(a.grid), dim3(kTB), 0, c->stream,
                               a.in.base, a.in.mis, a.nstarts, a.nstarts / rec_slots(c), c->len, (Key1*)a.ka, a.pc, a.dgt, a.part_shift, a.nsuper, a.blk_log2,
                               nr_rbits, nr_sqbit, nr_dmask, nr_capg);
        else
            with_bool(a.in.kind == ReadSrc::Packed, [&](auto pk) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(extract1_part_kernel<MODE, NH, REPK, false, FAST, NRW, decltype(pk)::value>), dim3(a.grid), dim3(kTB), 0,
                                   c->stream, a.in.base, a.in.mis, a.nstarts, a.navail, c->len, (Key1*)a.ka, a.pc, a.dgt, a.part_shift, a.nsuper, a.blk_log2,
                                   nr_rbits, nr_sqbit, nr_dmask, nr_capg, a.in.bad);
            });
    }); }); });
}

// Two-word keys.  NBH: significant bytes of the high word (key2_nbh), 0 for strand representatives.
template <int MODE, int NBH>
void launch_extract2_part(goss_gpu_ctx* c, const FirstLevelLaunch& a)
{
    with_digit_hists(a.nh, [&](auto nh_c) {
        constexpr int NH = decltype(nh_c)::value;
        if constexpr (MODE == 0)
            if (a.in.kind == ReadSrc::Records)
            {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(extract2_part_kernel<0, NH, GOSS_FUSED_NKEYS2, NBH, true>), dim3(a.grid), dim3(kTB), 0, c->stream,
                                   a.in.base, a.in.mis, a.nstarts, a.nstarts / rec_slots(c), c->len, (Key2*)a.ka, a.pc, a.dgt, a.part_shift, a.nsuper, a.blk_log2);
                return;
            }
        with_bool(a.in.kind == ReadSrc::Packed, [&](auto pk) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(extract2_part_kernel<MODE, NH, GOSS_FUSED_NKEYS2, NBH, false, decltype(pk)::value>), dim3(a.grid), dim3(kTB), 0,
                               c->stream, a.in.base, a.in.mis, a.nstarts, a.navail, c->len, (Key2*)a.ka, a.pc, a.dgt, a.part_shift, a.nsuper, a.blk_log2, a.in.bad);
        });
    });
}

template <class K>
void launch_first_level(const FusedChunk<K>& ch, const FusedForm& form, bool canon_l1, const BucketRegions& br, const GapTable* dgt, PartCounters* pc)
{
    goss_gpu_ctx* c = ch.c;
    const uint32_t shift = ch.keybits - form.segbits, npass = (form.segbits + 7) / 8;
    FirstLevelLaunch a{};
    a.in = ch.src.launch();
    if (ch.src.packed()) c->stats.pk_fused_chunks++;
    a.nstarts = ch.nstarts; a.navail = ch.navail;
    a.ka = ch.ka; a.pc = pc; a.dgt = dgt;
    a.part_shift = form.msd ? ch.keybits - 8 : shift;           // the fused kernel's digit
    a.nsuper = (ch.nstarts + br.super - 1) / br.super;
    a.blk_log2 = br.blk_log2;
    a.grid = br.grid;                                            // the regions were sized for this many workgroups
    a.nh = form.msd ? 0 : (npass > 2 ? 2 : 1);
    PhaseTimer t(c, GOSS_T_EXTRACT, ch.nstarts);
    if constexpr (FusedChunk<K>::kOne)
    {
        // the 32-bit forms of the kernel: the partition digit is the key's top eight bits (msd) and lies at bit 34 or above
        const bool fastk = a.nh == 0 && 2 * c->len >= 32 && a.part_shift >= 34 && !c->knobs.no_fast32;
        const bool narrow = form.msd && form.rem32() && form.narrow;
        const uint32_t nr_rbits = form.rbits32, nr_sqbit = form.squeeze ? c->len - 1 : 0u, nr_dmask = (1u << form.r32_bits) - 1u;
        const uint32_t nr_capg = std::max(576u, c->knobs.narrow_capg);          // (the kernel takes its LDS layout's own number of granules where that is less: kernels_extract.hpp, kSlots)
        if (ch.graph_mode) launch_extract1_part<1, 0>(c, a, fastk, narrow, nr_rbits, nr_sqbit, nr_dmask, nr_capg);
        // gossamer's canonical form computed per window (many distinct keys: choose_key_space)
        else if (canon_l1) launch_extract1_part<0, 2>(c, a, fastk, narrow, nr_rbits, nr_sqbit, nr_dmask, nr_capg);
        // k-mer sets are counted as strand representatives and mapped to the canonical form
        // afterwards (canonicalize_run); odd k: the central base picks the strand
        else if (c->len & 1u) launch_extract1_part<0, 1>(c, a, fastk, narrow, nr_rbits, nr_sqbit, nr_dmask, nr_capg);
        else launch_extract1_part<0, 0>(c, a, fastk, narrow, nr_rbits, nr_sqbit, nr_dmask, nr_capg);
    }
    else
    {
        if (ch.graph_mode) launch_extract2_part<1, 8>(c, a);
        else if (ch.rep_graph) launch_extract2_part<0, 0>(c, a);          // (NBH 0: strand representatives)
        else
            switch (key2_nbh(c))
            {
                case 2: launch_extract2_part<0, 2>(c, a); break;
                case 4: launch_extract2_part<0, 4>(c, a); break;
                case 6: launch_extract2_part<0, 6>(c, a); break;
                default: launch_extract2_part<0, 8>(c, a); break;
            }
    }
    t.stop();
}

// What the first level left: n keys in the bucket regions (their counts now in *gt, on the host and the device), read by
// `tiles` tiles of the pass that follows.
struct FirstLevelResult { uint64_t n = 0, tiles = 0, windows = 0; };

template <class K>
int read_first_level(const FusedChunk<K>& ch, const FusedForm& form, const BucketRegions& br, const PartCounters* pc, GapTable* gt, GapTable* dgt,
                     FirstLevelResult* out)
{
    goss_gpu_ctx* c = ch.c;
    std::vector<unsigned long long> hpc(sizeof(PartCounters) / 8);
    HIP_TRY(hipMemcpyAsync(hpc.data(), pc, sizeof(PartCounters), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const PartCounters* hp = (const PartCounters*)hpc.data();
    if (hp->overflow) { c->stats.fused_overflows++; return ch.decline("a bucket region overflowed"); }
    ch.lap("extraction + first level");
#if defined(GOSS_STAMPS)
    // (timing build: wave 0's cycles per phase and tile, averaged over the workgroups)
    if (hp->hist[505])
        std::fprintf(stderr, "libgossgpu: stamps per tile (cycles): A %.0f  B %.0f  C %.0f  scatter %.0f  D %.0f   (%llu tiles)\n",
                     (double)hp->hist[500] / hp->hist[505], (double)hp->hist[501] / hp->hist[505], (double)hp->hist[502] / hp->hist[505],
                     (double)hp->hist[503] / hp->hist[505], (double)hp->hist[504] / hp->hist[505], (unsigned long long)hp->hist[505]);
    if (hp->hist[505] && hp->hist[506])
        std::fprintf(stderr, "libgossgpu: stamps, finer: C = scan %.0f + bookkeeping %.0f + barrier; scatter = LDS %.0f + encoder %.0f + barrier; D = stores %.0f + absorb %.0f + barrier %.0f\n",
                     (double)hp->hist[506] / hp->hist[505], (double)hp->hist[507] / hp->hist[505], (double)hp->hist[510] / hp->hist[505],
                     (double)hp->hist[511] / hp->hist[505], (double)hp->hist[508] / hp->hist[505], (double)hp->hist[509] / hp->hist[505],
                     (double)hp->hist[504] / hp->hist[505]);
#endif
    const uint64_t n = hp->keys_out;
    if (n == 0) return kFusedDeclined;
    if (n > ch.ka_slots || n > ch.kb_slots) return ch.decline("more keys than the buffers hold");
    const bool narrow = form.rem32() && form.narrow;
    uint64_t tiles = 0, sum = 0;
    // of the pass that reads the regions
    const uint64_t tile_keys = narrow ? (uint64_t)(form.r32_bits == 9 ? Sub32N<9>::kTileSlots : Sub32N<10>::kTileSlots)
                             : form.rem32() ? (uint64_t)kSub32Tile : form.msd ? (uint64_t)SubCfg<K>::kTile : (uint64_t)SortCfg<K, false>::kTile;
    for (int d = 0; d < 256; ++d)
    {
        // one-word keys: slots handed out in whole blocks, padding included (the next pass skips it)
        gt->cnt[d] = hp->cursors[d * kCursorStride];
        gt->tile_first[d] = tiles;
        tiles += (gt->cnt[d] + tile_keys - 1) / tile_keys;
        sum += gt->cnt[d];
    }
    gt->tile_first[256] = tiles;
    // (the 8-byte slots handed out hold the keys: one each, or -- narrow form -- twelve to a granule of eight)
    const uint64_t n_slots = narrow ? n / 3 * 2 : n;
    const uint64_t B = 1ULL << br.blk_log2;
    if (sum < n_slots || sum > n_slots + 8 + (uint64_t)br.grid * 256 * (2 * B + 8))
        throw StatusError{GOSS_ERR_HIP, "fused extraction: bucket counts do not add up"};
    HIP_TRY(hipMemcpyAsync(dgt, gt, sizeof(GapTable), hipMemcpyHostToDevice, c->stream));
    out->n = n; out->tiles = tiles; out->windows = hp->windows;
    return kFusedGoOn;
}

// ---- 4. counting: one of three sequences, each with its own retries ----------------------------
struct FusedLookback { LookbackCtl* ctl; LookbackCtl* hctl; };          // the look-back / overflow word of the passes: device, pinned host

// 4a'. second level, 32-bit-remainder form: keys of region b go to sub-region (b, next 9 or 10 bits) as u32 remainders;
// an optional third level; the counting, in the next larger table while one overflows.  kFusedAgain: this form does not
// take the chunk -- the context now asks for more sub-segments or for the 8-byte form.
inline int count_rem32(const FusedChunk<Key1>& ch, FusedForm form, const Sub32Regions& sub, const FirstLevelResult& fl, const GapTable* dgt,
                       FusedLookback lb, Run* r)
{
    goss_gpu_ctx* c = ch.c;
    Key1* ka = ch.ka; Key1* kb = ch.kb;
    const uint64_t n = fl.n, tiles = fl.tiles;
    const uint32_t r32_regions = form.r32_regions(), r32_bits = form.r32_bits, r32_split = form.r32_split, rbits32 = form.rbits32;
    const uint32_t sqbit32 = c->len - 1;
    const bool narrow = form.narrow, squeeze = form.squeeze;
    // The sub-regions hold the remainders' images (goss_words.hpp: the counting kernel's mix, done here where the issue slots
    // are idle) unless a third level follows, which splits on the remainder's top bits and must keep key order.
    const bool image = r32_split == 0;
    // (both levels' kernels take the squeeze form's field and digit from goss_words.hpp, which is made for this one shape)
    if (squeeze && (rbits32 != kNarrowSqRbits || r32_bits != kNarrowSqDigitBits))
        throw StatusError{GOSS_ERR_HIP, "fused path: the squeeze form with other than 33-bit remainders under nine second-level bits"};
    SubTable32* dsub = (SubTable32*)c->arena.temp(sizeof(SubTable32));
    unsigned long long* cur2 = (unsigned long long*)c->arena.temp((uint64_t)r32_regions * 4);     // pairs of 32-bit cursors
    uint64_t* seg_beg = (uint64_t*)c->arena.temp((uint64_t)r32_regions * 8);
    uint64_t* seg_end = (uint64_t*)c->arena.temp((uint64_t)r32_regions * 8);
    Tile32* tdesc = (Tile32*)c->arena.temp(std::max<uint64_t>(tiles, 1) * sizeof(Tile32));
    // (only the used part of the table travels: the starts, then the capacities)
    HIP_TRY(hipMemcpyAsync(dsub->start, sub.start.data(), (uint64_t)r32_regions * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dsub->cap, sub.cap.data(), (uint64_t)r32_regions * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(cur2, 0, (uint64_t)r32_regions * 4, c->stream));
    if (narrow && r32_bits == 9)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tiles32_kernel<Sub32N<9>::kTileSlots>), dim3(grid_for(tiles, 256)), dim3(256), 0, c->stream,
                           dgt, tdesc, (uint32_t)tiles);
    else if (narrow)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tiles32_kernel<Sub32N<10>::kTileSlots>), dim3(grid_for(tiles, 256)), dim3(256), 0, c->stream,
                           dgt, tdesc, (uint32_t)tiles);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tiles32_kernel<kSub32Tile>), dim3(grid_for(tiles, 256)), dim3(256), 0, c->stream,
                           dgt, tdesc, (uint32_t)tiles);
    {
        PhaseTimer t(c, GOSS_T_SCATTER, n);
        const dim3 g2((uint32_t)((tiles + 7) / 8 * 8));
#define GOSS_LAUNCH_S32I(SQ, B2, NRW, IMG)                                                                               \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(subpart32_kernel<SQ, B2, NRW, IMG>), g2, dim3(kTB), 0, c->stream, (const Key1*)ka, (uint32_t*)kb, rbits32, \
                       sqbit32, cur2, (const Tile32*)tdesc, (uint32_t)tiles, (const SubTable32*)dsub, lb.ctl)
#define GOSS_LAUNCH_S32N(SQ, B2, NRW) do { if (image) GOSS_LAUNCH_S32I(SQ, B2, NRW, true); else GOSS_LAUNCH_S32I(SQ, B2, NRW, false); } while (0)
#define GOSS_LAUNCH_S32(SQ, B2) do { if (narrow) GOSS_LAUNCH_S32N(SQ, B2, true); else GOSS_LAUNCH_S32N(SQ, B2, false); } while (0)
        if (squeeze) GOSS_LAUNCH_S32(true, 9);          // (only the 9-bit form of an odd k-mer set needs the squeeze)
        else if (r32_bits == 9) GOSS_LAUNCH_S32(false, 9);
        else GOSS_LAUNCH_S32(false, 10);
#undef GOSS_LAUNCH_S32
#undef GOSS_LAUNCH_S32N
#undef GOSS_LAUNCH_S32I
        t.stop();
    }
    hipLaunchKernelGGL(sub_bounds32_kernel, dim3(r32_regions / 256), dim3(256), 0, c->stream, (const SubTable32*)dsub,
                       (const uint32_t*)cur2, r32_regions, seg_beg, seg_end);
    HIP_TRY(hipMemcpyAsync(lb.hctl, lb.ctl, sizeof(LookbackCtl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (lb.hctl->error) { c->stats.fused_overflows++; return ch.decline("a 32-bit sub-region overflowed"); }
    ch.lap("second level (32-bit remainders)");
    // third level: every segment split into 2^r32_split sub-segments, from kb into ka (same offsets); the counts are
    // then staged in kb
    const uint32_t* rems = (const uint32_t*)kb;
    Key1* spare32 = ka;
    uint32_t nseg32 = r32_regions;
    if (r32_split)
    {
        nseg32 = r32_regions << r32_split;
        uint64_t* sub_beg = (uint64_t*)c->arena.temp((uint64_t)nseg32 * 8);
        uint64_t* sub_end = (uint64_t*)c->arena.temp((uint64_t)nseg32 * 8);
        {
            PhaseTimer t(c, GOSS_T_SCATTER, n);
            hipLaunchKernelGGL(subsplit32_kernel, unit_grid(r32_regions), dim3(kTB), 0, c->stream, (const uint32_t*)kb, (uint32_t*)ka,
                               (const uint64_t*)seg_beg, (const uint64_t*)seg_end, rbits32 - (squeeze ? 1u : 0u), r32_split, sub_beg, sub_end);
            t.stop();
        }
        check_launch("third-level split kernel");
        seg_beg = sub_beg; seg_end = sub_end;
        rems = (const uint32_t*)ka;
        spare32 = kb;
        ch.lap("third level (sub-segments)");
    }
    int rc;
    for (;;)
    {
        const Rem32Layout lay{seg_beg, seg_end, nseg32, form.r32_slots, squeeze, image, rbits32, sqbit32, r32_split};
        rc = segment_reduce32(c, rems, spare32, n, r, lay);
        if (rc != 1 || form.r32_slots >= 16384 || c->knobs.rem32_slots) break;
        // the remainders are still in their sub-regions: only the counting is redone, in the next larger table
        c->stats.segment_retries++;
        form = form.larger_r32_table();
    }
    if (rc != 0)
    {
        // more distinct keys per segment than this form takes: the chunk again
        c->stats.segment_retries++;
        // more second-level bits while the remainder allows them (the chunk's first level is redone: the staging of
        // the counts has overwritten its regions), else the 8-byte form and its ladder of tables
        if (rc == 1 && r32_split < (uint32_t)kSub32SplitMax) c->knobs.rem32_split_min = r32_split + 1;
        else c->knobs.rem32 = false;
        if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: fused path: 32-bit form with %u + %u bits overflowed (%d), redoing the chunk %s\n", r32_bits, r32_split, rc,
                                   c->knobs.rem32 ? "with more sub-segments" : "in the 8-byte form");
        return kFusedAgain;
    }
    c->stats.fused_msd_chunks++;
    c->stats.rem32_chunks++;
    if (narrow) c->stats.narrow_chunks++;
    c->stats.rem32_bits_last = r32_bits;
    c->stats.rem32_split_last = r32_split;
    return kFusedGoOn;
}

// 4a. second level: keys of region b go to sub-region (b, low digit) by atomic cursors; the counting, with the next larger
// form while a table of one-word keys overflows.
template <class K>
int count_sub8(const FusedChunk<K>& ch, FusedForm form, const Sub8Regions& sub, const FirstLevelResult& fl, const GapTable* dgt, FusedLookback lb, Run* r)
{
    goss_gpu_ctx* c = ch.c;
    const uint64_t n = fl.n;
    const uint32_t shift = ch.keybits - form.segbits;
    SubTable* dsub = (SubTable*)c->arena.temp(sizeof(SubTable));
    unsigned long long* cur2 = (unsigned long long*)c->arena.temp(65536ULL * kSubCursorStride * 8);
    uint64_t* seg_beg = (uint64_t*)c->arena.temp(65536 * 8);
    uint64_t* seg_end = (uint64_t*)c->arena.temp(65536 * 8);
    HIP_TRY(hipMemcpyAsync(dsub, sub.table.data(), sizeof(SubTable), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(cur2, 0, 65536ULL * kSubCursorStride * 8, c->stream));
    {
        PhaseTimer t(c, GOSS_T_SCATTER, n);
        // (a multiple of 8 workgroups: the kernel deals the tiles out by XCD; the 96-bit table is fed 12-byte records)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_onesweep_kernel<K, false, false, true, SubCfg<K>::kItems>), dim3((uint32_t)((fl.tiles + 7) / 8 * 8)), dim3(kTB), 0,
                           c->stream, (const K*)ch.ka, (const uint32_t*)nullptr, ch.kb, (uint32_t*)nullptr, n, shift, shift,
                           (const unsigned long long*)nullptr, (unsigned long long*)nullptr, lb.ctl, cur2,
                           dgt, (const SubTable*)dsub, form.table == FusedForm::k96 ? 1u : 0u);
        t.stop();
    }
    hipLaunchKernelGGL(sub_bounds_kernel, dim3(256), dim3(256), 0, c->stream, (const SubTable*)dsub,
                       (const unsigned long long*)cur2, seg_beg, seg_end);
    HIP_TRY(hipMemcpyAsync(lb.hctl, lb.ctl, sizeof(LookbackCtl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (lb.hctl->error) { c->stats.fused_overflows++; return ch.decline("a sub-region overflowed"); }
    ch.lap("second level");
    int rc;
    for (;;)
    {
        rc = segment_reduce<K>(c, ch.kb, ch.ka, n, form.segbits, r, seg_beg, seg_end, form.seg_count());
        // a table that overflowed (one-word keys): the keys are still in their sub-regions, so only the counting
        // is redone, with the next larger form -- 8192 slots, then 2 and 4 workgroups per segment -- instead of
        // the whole chunk with the unfused kernels
        const bool ladder = form.table == FusedForm::kSmall || (form.table == FusedForm::kBig && form.rounds < (uint32_t)kBigRoundsMax);
        if (rc != 1 || !FusedChunk<K>::kOne || !c->knobs.big_table || !ladder) break;
        c->stats.segment_retries++;
        form = form.larger_table();
        if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: fused path: a counting table overflowed, next form %d\n", 1 + (int)form.rounds);
    }
    if (rc != 0)
    {
        c->stats.segment_retries++;
        // this input is too skewed for it: the next smaller form from now on
        if (form.table == FusedForm::k96) c->knobs.table96 = false;
        else if (form.table == FusedForm::kWide) c->knobs.wide_table = false;
        else if (form.table == FusedForm::kBig) c->knobs.big_table = false;
        return ch.decline("a segment table overflowed");
    }
    c->stats.fused_msd_chunks++;
    if (form.table != FusedForm::kSmall) c->stats.big_table_chunks++;
    if (form.table == FusedForm::kWide) c->stats.wide_table_chunks++;
    if (form.table == FusedForm::k96) c->stats.table96_chunks++;
    return kFusedGoOn;
}

// 4b. remaining partition passes: the first reads the bucket regions, the others are dense; then the counting.
// `chunk`: the arena scope of the chunk -- everything taken under it is given back before the counting.
template <class K>
int count_dense(const FusedChunk<K>& ch, const FusedForm& form, const FirstLevelResult& fl, const GapTable* dgt, PartCounters* pc, FusedLookback lb,
                ArenaScope& chunk, Run* r)
{
    goss_gpu_ctx* c = ch.c;
    constexpr int kTile = SortCfg<K, false>::kTile;
    const uint64_t n = fl.n, tiles = fl.tiles;
    const uint32_t shift = ch.keybits - form.segbits, npass = (form.segbits + 7) / 8;
    const uint64_t ntiles_dense = (n + kTile - 1) / kTile;
    unsigned long long* status = (unsigned long long*)c->arena.temp(256ULL * std::max(tiles, ntiles_dense) * 8);
    {
        PhaseTimer t(c, GOSS_T_SCAN, 512);
        hipLaunchKernelGGL(scan_rows256_kernel, dim3(2), dim3(kTB), 0, c->stream, pc->hist);
        t.stop();
    }
    K* src = ch.ka; K* dst = ch.kb;
    for (uint32_t di = 1; di < npass; ++di)
    {
        const uint32_t d = shift + 8 * di;
        const bool gapped = di == 1;
        const uint64_t nt = gapped ? tiles : ntiles_dense;
        HIP_TRY(hipMemsetAsync(status, 0, nt * 256 * 8, c->stream));
        {
            PhaseTimer t(c, GOSS_T_SCATTER, n);
            if (gapped)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_onesweep_kernel<K, false, false, true>), dim3((uint32_t)nt), dim3(kTB), 0,
                                   c->stream, (const K*)src, (const uint32_t*)nullptr, dst, (uint32_t*)nullptr, n, d, shift,
                                   (const unsigned long long*)(pc->hist + (di - 1) * 256), status, lb.ctl,
                                   (unsigned long long*)nullptr, dgt, (const SubTable*)nullptr);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(radix_onesweep_kernel<K, false, false, false>), dim3((uint32_t)nt), dim3(kTB), 0,
                                   c->stream, (const K*)src, (const uint32_t*)nullptr, dst, (uint32_t*)nullptr, n, d, shift,
                                   (const unsigned long long*)(pc->hist + (di - 1) * 256), status, lb.ctl,
                                   (unsigned long long*)nullptr, (const GapTable*)nullptr, (const SubTable*)nullptr);
            t.stop();
        }
        HIP_TRY(hipMemcpyAsync(lb.hctl, lb.ctl, sizeof(LookbackCtl), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lb.hctl->error)
        {
            std::fprintf(stderr, "libgossgpu: radix look-back chain gave up in the fused path; redoing the chunk unfused\n");
            c->stats.lookback_failures++;
            c->knobs.ordered_tiles = true;
            return kFusedDeclined;
        }
        std::swap(src, dst);
    }
    // src = partitioned keys (dense: npass >= 2), dst = spare
    chunk.rewind();
    const int rc = segment_reduce<K>(c, src, dst, n, form.segbits, r);
    if (rc != 0) { c->stats.segment_retries++; return ch.decline("a segment table overflowed"); }
    return kFusedGoOn;
}

// ---- the driver --------------------------------------------------------------------------------
template <class K>
int fused_chunk_once(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, K* ka, uint64_t ka_slots, K* kb, uint64_t kb_slots)
{
    constexpr bool kOne = FusedChunk<K>::kOne;
    const uint32_t keybits = 2 * c->len;
    if (src.records() && !kOne && c->mode == GOSS_MODE_GRAPH && !c->knobs.graph_rep) return kFusedDeclined;          // (the record form extracts one key per window)
    FusedChunk<K> ch{c, src, nstarts, navail, ka, ka_slots, kb, kb_slots, keybits};
    ch.rep_graph = c->mode == GOSS_MODE_GRAPH && c->knobs.graph_rep;
    ch.rep_kmer = c->mode != GOSS_MODE_GRAPH && kOne;
    ch.use_rep = ch.rep_graph || ch.rep_kmer;
    ch.graph_mode = c->mode == GOSS_MODE_GRAPH && !ch.rep_graph;
    ch.reduced = ka_slots < nstarts * (ch.graph_mode ? 2 : 1) || kb_slots < nstarts * (ch.graph_mode ? 2 : 1);
    if (!c->knobs.fused || c->path != 0 || !c->knobs.lookback || c->knobs.ordered_tiles || nstarts < c->knobs.fused_min || keybits < (uint32_t)kSegBits + 8)
        return kFusedDeclined;
    ArenaScope scope(c->arena);
    ch.t_begin = std::chrono::steady_clock::now();

    // 1. a sample of the keys, the distinct keys it promises, and the key space the chunk is counted in
    FusedSample sm;
    if (const int rc = plan_sample(ch, &sm); rc != kFusedGoOn) return rc;
    sm.ns = extract_sample(ch, sm, true);
    if (sm.ns < (1u << 20)) return ch.decline("mostly non-bases");
    ch.lap("sample extracted");
    sm.n_exp = (uint64_t)((double)sm.ns * sm.scale);
    uint64_t m_rare = 0;
    uint64_t m_est = spectrum_estimate<K>(c, ka, sm.ns, (double)sm.n_exp, &m_rare);
    if (c->knobs.est_scale != 1.0) m_est = (uint64_t)((double)m_est * c->knobs.est_scale);      // tests: a wrong estimate on purpose
    m_rare = std::min(m_rare, m_est);
    ch.lap("distinct keys estimated");
    if (m_est == 0 || m_est > sm.n_exp / 3) return ch.decline("too little duplication for the segment path");
    const bool canon_l1 = choose_key_space(c, ch.rep_kmer, m_est, m_rare, sm.n_exp);
    if (canon_l1)
    {
        // (the regions are sized from the sample: it must be in the key space the first level writes)
        if (extract_sample(ch, sm, false) != sm.ns) throw StatusError{GOSS_ERR_HIP, "fused path: the sample changed between two extractions"};
        ch.lap("sample extracted again (canonical forms)");
    }
    // buffers sized from the estimated share of valid windows must hold what the sample promises
    if (ch.reduced && ((double)sm.n_exp * 1.035 + 262144.0 > (double)ka_slots || (double)sm.n_exp * 1.02 + 6.0e6 > (double)kb_slots))
    {
        if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: fused path: %llu keys expected, buffers of %llu / %llu slots too small\n",
                                   (unsigned long long)sm.n_exp, (unsigned long long)ka_slots, (unsigned long long)kb_slots);
        return (int)kFusedNeedFull;
    }

    // the form: how many segment bits, which table, which second level
    const uint64_t limit = SegCfg<K>::kLimit;
    FusedForm form = choose_form<K>(c, keybits, m_est, ch.graph_mode, canon_l1);
    if ((form.table == FusedForm::kSmall && (m_est >> form.segbits) > limit) || form.segbits + 8 > keybits)
        return ch.decline("too many distinct keys per segment");

    // 2. histograms of the sample, and the regions sized from them: sub-regions of the second buffer (two-level form;
    //    they must fit, else the next simpler form is used), then bucket regions of the first
    SampleHist hist = sample_histograms(ch, form, sm.ns);
    Sub32Regions sub32;
    Sub8Regions sub8;
    if (form.msd && form.rem32())
    {
        sub32 = size_sub32_regions(hist.joint17, form, sm, c->knobs.fused_capscale, ka_slots, kb_slots);
        if (sub32.misfit)
        {
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: 32-bit sub-regions need %llu slots of %llu: 8-byte form\n",
                                       (unsigned long long)sub32.slots, (unsigned long long)(2 * kb_slots));
            form = form.eight_byte();
            if ((m_est >> form.segbits) > limit) return ch.decline("too many distinct keys per segment");
        }
    }
    if (form.msd && !form.rem32())
    {
        sub8 = size_sub8_regions(hist.joint, sm, c->knobs.fused_capscale);
        if (sub8.slots > kb_slots && ch.reduced)
        {
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: sub-regions need %llu slots of %llu\n", (unsigned long long)sub8.slots, (unsigned long long)kb_slots);
            return (int)kFusedNeedFull;
        }
        if (sub8.slots > kb_slots)
        {
            if (c->knobs.debug) std::fprintf(stderr, "libgossgpu: sub-regions need %llu slots of %llu: one-level form\n",
                                       (unsigned long long)sub8.slots, (unsigned long long)kb_slots);
            if (form.table != FusedForm::kSmall) return ch.decline("sub-regions do not fit and the big table needs them");
            form = form.one_level();
            // the one-level form partitions on the LOW digit: its marginal histogram
            std::fill(hist.hh.begin(), hist.hh.end(), 0ULL);
            for (uint32_t i = 0; i < 65536; ++i) hist.hh[i & 255u] += hist.joint[i];
        }
    }
    ch.lap("sample histograms");
    BucketRegions br;
    size_bucket_regions<K>(hist.hh, sm, nstarts, ch.graph_mode, ka_slots, c->knobs.fused_capscale, c->knobs.blk_log2_max, &br);
    // (buffers sized from the share of valid windows: the caller retries with one slot per window start)
    if (!br.fits) return ch.reduced ? (int)kFusedNeedFull : ch.decline("bucket regions do not fit the key buffer");

    // 3. extraction that partitions
    GapTable* dgt = (GapTable*)c->arena.temp(sizeof(GapTable));
    PartCounters* pc = (PartCounters*)c->arena.temp(sizeof(PartCounters));
    HIP_TRY(hipMemcpyAsync(dgt, &br.gt, sizeof(GapTable), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(pc, 0, sizeof(PartCounters), c->stream));
    launch_first_level(ch, form, canon_l1, br, dgt, pc);
    FirstLevelResult fl;
    if (const int rc = read_first_level(ch, form, br, pc, &br.gt, dgt, &fl); rc != kFusedGoOn) return rc;

    // 4. the second level and the counting
    FusedLookback lb{(LookbackCtl*)c->arena.temp(sizeof(LookbackCtl)), (LookbackCtl*)((uint8_t*)c->h_pinned + 128)};
    HIP_TRY(hipMemsetAsync(lb.ctl, 0, sizeof(LookbackCtl), c->stream));
    Run r{nullptr, nullptr, 0};
    int rc = kFusedDeclined;
    if (form.msd && form.rem32()) { if constexpr (kOne) rc = count_rem32(ch, form, sub32, fl, dgt, lb, &r); }          // (one-word keys only: choose_form)
    else if (form.msd) rc = count_sub8(ch, form, sub8, fl, dgt, lb, &r);
    else rc = count_dense(ch, form, fl, dgt, pc, lb, scope, &r);
    if (rc != kFusedGoOn) return rc;
    ch.lap("segments counted");

    // 5. the run
    if (canon_l1) c->stats.canon_chunks++;
    if (ch.use_rep && !canon_l1)
    {
        // the run stays in representative space: it is mapped to gossamer's canonical forms when it meets a run
        // that is not, or at finish -- a build of several chunks pays for the re-ordering once, on the merged run
        r.rep = true;
        c->stats.rep_chunks++;
    }
    c->build.runs.push_back(r);
    c->build.windows += fl.windows;
    c->build.keys_total += ch.rep_graph ? 2 * fl.n : fl.n;          // (the adapter's key stream: two keys per window of a graph)
    c->stats.fused_chunks++;
    if (src.records()) c->stats.rec_chunks++;
    return kFusedDone;
}

// A 32-bit-remainder form that overflowed has adjusted the context (more sub-segments, or never that form): the chunk again.
template <class K>
int process_chunk_fused(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nstarts, uint64_t navail, K* ka, uint64_t ka_slots,
                        K* kb, uint64_t kb_slots)
{
    for (;;)
    {
        const int rc = fused_chunk_once<K>(c, src, nstarts, navail, ka, ka_slots, kb, kb_slots);
        if (rc != kFusedAgain) return rc;
    }
}
