// reads_path.hpp -- reads against an object (goss_gpu_object_match_reads, _classify_reads, _taxo_*, _colour_reads): one
// pass over the reads whatever it is asked for (kernels_match.hpp), the batch the _host forms stage, the classify
// bitmaps, a taxonomy over a KmerSet's k-mers (kernels_taxo.hpp), and the colour words (kernels_elect.hpp).
// Part of goss_gpu.hip, which includes it at file scope behind the objects' query entry points and keeps the entry
// points of everything here.

namespace {

// exclusive scan of a[0..n) in place; `partial` holds the chunk sums of every level
void exclusive_scan_partials(hipStream_t st, uint64_t* a, uint64_t n, uint64_t* partial)
{
    const uint64_t nchunks = (n + kScanChunk - 1) / kScanChunk;
    if (nchunks <= 1)
    {
        hipLaunchKernelGGL(scan_apply_kernel, dim3(1), dim3(kTB), 0, st, a, n, (const uint64_t*)nullptr);
        return;
    }
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(grid_for(n, kScanChunk)), dim3(kTB), 0, st, (const uint64_t*)a, n, partial);
    exclusive_scan_partials(st, partial, nchunks, partial + nchunks);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(grid_for(n, kScanChunk)), dim3(kTB), 0, st, a, n, (const uint64_t*)partial);
}

// ---- the taxonomy's tables ----------------------------------------------------------------------------------------------

inline dim3 taxo_grid(uint64_t n) { return dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 2048)); }

struct TaxoTables {
    const uint32_t *parent, *last, *id, *sorted_id, *sorted_class;
};
TaxoTables taxo_tables(const goss_gpu_object* o)
{
    const uint32_t* t = o->taxo_tree;
    const uint64_t n = o->taxo_n;
    return TaxoTables{t, t + n, t + 2 * n, t + 3 * n, t + 4 * n};
}

// what the two taxonomy modes of a pass read and write, but for the annotate mode's classes per read
TaxoView taxo_view(const goss_gpu_object* o)
{
    const TaxoTables t = taxo_tables(o);
    TaxoView tx;
    tx.parent = t.parent; tx.last = t.last; tx.ann = o->taxo_ann;
    return tx;
}

// the checks every taxo call but the tree's begins with; *empty: the set has no k-mers, and the call has nothing to do
int taxo_ready(goss_gpu_object* o, const char* what, bool need_ann, bool* empty)
{
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = std::string(what) + " needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    *empty = o->q.s.count == 0;
    if (*empty) return GOSS_OK;
    if (!o->taxo_n) { o->last_error = std::string(what) + ": no tree (goss_gpu_object_taxo_tree_host)"; return GOSS_ERR_STATE; }
    if (need_ann && !o->taxo_ann_kept) { o->last_error = std::string(what) + ": no annotation (goss_gpu_object_taxo_annotation_host)"; return GOSS_ERR_STATE; }
    return GOSS_OK;
}

// out[0..z) = the classes of the node ids in[0..z) (device arrays); an id the tree lacks throws, `item` naming what i counts
void taxo_dense(goss_gpu_object* o, const char* what, const char* item, const uint32_t* in, uint64_t z, uint32_t allow, uint32_t* out)
{
    if (!z) return;
    const TaxoTables t = taxo_tables(o);
    HIP_TRY(hipMemsetAsync(o->d_bad, 0xFF, 8, o->stream));
    hipLaunchKernelGGL(taxo_dense_kernel, taxo_grid(z), dim3(kTB), 0, o->stream, in, z, t.sorted_id, t.sorted_class, o->taxo_n, allow, out, o->d_bad);
    HIP_TRY(hipMemcpyAsync(o->h_bad, o->d_bad, 8, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    check_launch(what);
    const unsigned long long bad = *o->h_bad;
    if (bad == ~0ULL) return;
    uint32_t id = 0;
    HIP_TRY(hipMemcpy(&id, in + bad, 4, hipMemcpyDeviceToHost));
    throw StatusError{GOSS_ERR_INVALID_ARG, std::string(what) + ": " + item + " " + std::to_string(bad) + " has node id " + std::to_string(id) + ", which the tree lacks"};
}

// bins (device, n + 2) = the tally of z classes
void taxo_tally(goss_gpu_object* o, const uint32_t* classes, uint64_t z)
{
    HIP_TRY(hipMemsetAsync(o->taxo_bins, 0, ((uint64_t)o->taxo_n + 2) * 8, o->stream));
    if (z) hipLaunchKernelGGL(taxo_tally_kernel, taxo_grid(z), dim3(kTB), 0, o->stream, classes, z, o->taxo_n, o->taxo_bins);
}

// counts[i] = the bin of the i-th node as given, then none and many
void taxo_bins_out(goss_gpu_object* o, uint64_t* counts)
{
    std::vector<unsigned long long> bins((uint64_t)o->taxo_n + 2);
    HIP_TRY(hipMemcpyAsync(bins.data(), o->taxo_bins, bins.size() * 8, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    for (uint32_t i = 0; i < o->taxo_n; ++i) counts[i] = bins[o->taxo_pre[i]];
    counts[o->taxo_n] = bins[o->taxo_n];
    counts[o->taxo_n + 1] = bins[o->taxo_n + 1];
}

// ---- the pass over the reads -----------------------------------------------------------------------------------------------

// what a pass is asked to do
struct ReadsJob {
    const char* what;                       // names the call in messages
    int mode;                               // kModeCount / kModeAny / kModeClassify / kModeAnnotate / kModeTaxon / kModeColour (kernels_match.hpp)
    const void* d_bases;
    uint64_t nbytes;
    uint32_t flags;
    uint64_t max_reads;                     // what each per-read array holds
    uint32_t* d_windows;                    // per read, on the device; each may be NULL
    uint32_t* d_hits;                       // by mode: hits, 1 / 0, the 4-bit mask, (annotate: unused), the node id;
                                            // kModeColour: 8 bytes per read, the word
    uint64_t* d_read_starts;                // reads + 1 values
    bool must_fit = false;                  // more reads than max_reads are refused even where no array is given (annotate:
                                            // aux.tx.read_class holds max_reads classes)
    MatchAux aux{};                         // kModeClassify: the bitmaps; kModeAnnotate / kModeTaxon: the taxonomy; kModeColour: the words
};

// what one pass over the reads leaves on the host
struct ReadsPass {
    uint64_t reads = 0;
    unsigned long long sums[4] = {0, 0, 0, 0};  // windows, hits, reads with a hit; kModeTaxon: hits at a rank without a class
    unsigned long long counts[16] = {};         // kModeClassify: reads per mask; kModeTaxon: [0] reads without a class, [1] with many
    unsigned long long by_count[65] = {};       // kModeColour: reads per number of bits in their word
    float ms = 0;
};

// One pass, past the entry point's own argument checks.  Two waits: for the number of reads, which sizes the rest, and
// for the sums; nothing is allocated once the object's buffers have grown.
int reads_pass(goss_gpu_object* o, const ReadsJob& job, ReadsPass* res)
{
    const uint64_t nbytes = job.nbytes;
    uint64_t* const d_read_starts = job.d_read_starts;
    if (nbytes == 0)
    {
        if (!d_read_starts) return GOSS_OK;
        return obj_guarded(o->device, o->last_error, [&]() {
            HIP_TRY(hipMemsetAsync(d_read_starts, 0, 8, o->stream));
            HIP_TRY(hipStreamSynchronize(o->stream));
        });
    }
    return obj_guarded(o->device, o->last_error, [&]() {
        const std::string what = job.what;
        const uint8_t* bases = (const uint8_t*)job.d_bases;
        const uint64_t ntiles = (nbytes + kMatchTile - 1) / kMatchTile;
        // working memory: [0, 256) sums[4], bad[2] at word 4, the classes' counts[16] at word 8; then the tiles' newline
        // counts (+ 1: the total) and the scan's partial sums, then the colour mode's by_count[65]
        const uint64_t npartial = 2 * ((ntiles + 1 + kScanChunk - 1) / kScanChunk) + 64;
        const bool colour = job.mode == kModeColour;
        const uint64_t hit_bytes = colour ? 8 : 4;
        uint8_t* mem = o->scan_sums.room(256 + (ntiles + 1 + npartial + 65) * 8);
        unsigned long long* sums = (unsigned long long*)mem;
        unsigned long long* bad = sums + 4;
        unsigned long long* counts = sums + 8;
        uint64_t* tiles = (uint64_t*)(mem + 256);
        uint64_t* partial = tiles + ntiles + 1;
        unsigned long long* by_count = (unsigned long long*)(partial + npartial);
        if (!o->h_pass) HIP_TRY(hipHostMalloc((void**)&o->h_pass, 1024, hipHostMallocDefault));      // (words 32 .. 96: by_count)
        for (hipEvent_t& e : o->pass_ev) if (!e) HIP_TRY(hipEventCreate(&e));
        const uint32_t aligned = ((uintptr_t)bases & 7u) == 0;

        // reads: one '\n' count per tile, scanned; the last byte decides whether a read is left open
        HIP_TRY(hipMemsetAsync(mem, 0, 256, o->stream));
        HIP_TRY(hipMemsetAsync(bad, 0xFF, 16, o->stream));
        HIP_TRY(hipMemsetAsync(tiles + ntiles, 0, 8, o->stream));
        HIP_TRY(hipEventRecord(o->pass_ev[0], o->stream));
        hipLaunchKernelGGL(match_count_newlines_kernel, unit_grid((ntiles + kWaves - 1) / kWaves), dim3(kTB), 0, o->stream, bases, nbytes, ntiles, tiles, aligned);
        exclusive_scan_partials(o->stream, tiles, ntiles + 1, partial);
        HIP_TRY(hipEventRecord(o->pass_ev[1], o->stream));
        HIP_TRY(hipMemcpyAsync(&o->h_pass[0], tiles + ntiles, 8, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipMemcpyAsync(&o->h_pass[1], bases + nbytes - 1, 1, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        check_launch((what + ": counting the reads").c_str());
        const bool open_end = (uint8_t)(o->h_pass[1] & 0xFF) != (uint8_t)'\n';
        const uint64_t reads = o->h_pass[0] + (open_end ? 1 : 0);
        res->reads = reads;
        if ((job.d_windows || job.d_hits || d_read_starts || job.must_fit) && reads > job.max_reads)
            throw StatusError{GOSS_ERR_BUFFER, what + ": the input holds " + std::to_string(reads) + " reads, the output arrays " + std::to_string(job.max_reads)};

        // outputs the caller left out are still the kernel's counters
        uint32_t* w = job.d_windows;
        uint32_t* h = job.d_hits;
        if (!w || !h)
        {
            const uint64_t each = (reads * 4 + 255) & ~255ULL;
            uint8_t* tmp = o->spare_out.room(3 * each + 256);
            if (!w) w = (uint32_t*)tmp;
            if (!h) h = (uint32_t*)(tmp + each);
        }
        if (reads)
        {
            HIP_TRY(hipMemsetAsync(w, 0, reads * 4, o->stream));
            HIP_TRY(hipMemsetAsync(h, 0, reads * hit_bytes, o->stream));
        }
        if (colour) HIP_TRY(hipMemsetAsync(by_count, 0, 65 * 8, o->stream));
        HIP_TRY(hipEventRecord(o->pass_ev[2], o->stream));
        MatchAux aux = job.aux;
        aux.tx.unann = sums + 3;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, unit_grid(ntiles), dim3(kTB), 0, o->stream, o->q, bases, nbytes, ntiles, (const uint64_t*)tiles, job.flags, aligned,
                               w, h, d_read_starts, bad, aux);
        };
        auto by_mode = [&](auto key) {
            typedef decltype(key) K;
            switch (job.mode)
            {
            case kModeAny: return launch(match_reads_kernel<K, kModeAny>);
            case kModeClassify: return launch(match_reads_kernel<K, kModeClassify>);
            case kModeAnnotate: return launch(match_reads_kernel<K, kModeAnnotate>);
            case kModeTaxon: return launch(match_reads_kernel<K, kModeTaxon>);
            case kModeColour: return launch(match_reads_kernel<K, kModeColour>);
            default: return launch(match_reads_kernel<K, kModeCount>);
            }
        };
        if (o->key_words == 1) by_mode(Key1{});
        else by_mode(Key2{});
        // what a mode adds behind the kernel, inside the timed stretch
        if (job.mode == kModeClassify && reads)
            hipLaunchKernelGGL(classify_sums_kernel, dim3((uint32_t)std::min<uint64_t>((reads + 255) / 256, 2048)), dim3(kTB), 0, o->stream,
                               (const uint32_t*)h, reads, counts);
        if (colour && reads)
            hipLaunchKernelGGL(elect_sums_kernel, dim3((uint32_t)std::min<uint64_t>((reads + 255) / 256, 2048)), dim3(kTB), 0, o->stream,
                               (const uint64_t*)h, reads, by_count);
        // (the colour mode's words are no sums: its hit sums stay 0)
        hipLaunchKernelGGL(match_sums_kernel, dim3((uint32_t)std::min<uint64_t>((reads + 255) / 256 + 1, 2048)), dim3(kTB), 0, o->stream,
                           (const uint32_t*)w, colour ? (const uint32_t*)nullptr : (const uint32_t*)h, reads, sums, d_read_starts, nbytes - (open_end ? 0 : 1));
        if (job.mode == kModeTaxon && reads)
        {
            // the figures from the classes, then the classes become node ids where they lie
            taxo_tally(o, h, reads);
            hipLaunchKernelGGL(taxo_ids_kernel, taxo_grid(reads), dim3(kTB), 0, o->stream, (const uint32_t*)h, reads, taxo_tables(o).id, h);
            HIP_TRY(hipMemcpyAsync(counts, o->taxo_bins + o->taxo_n, 16, hipMemcpyDeviceToDevice, o->stream));
        }
        HIP_TRY(hipEventRecord(o->pass_ev[3], o->stream));
        HIP_TRY(hipMemcpyAsync(o->h_pass, mem, 192, hipMemcpyDeviceToHost, o->stream));
        if (colour) HIP_TRY(hipMemcpyAsync(o->h_pass + 32, by_count, 65 * 8, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        check_launch((what + ": matching").c_str());
        if (o->h_pass[4] != ~0ULL)
            throw StatusError{GOSS_ERR_INVALID_ARG, what + ": the window at byte " + std::to_string(o->h_pass[4] >> 2) + ": the index walk cannot answer (damaged object)"};
        if (o->h_pass[5] != ~0ULL)
            throw StatusError{GOSS_ERR_INVALID_ARG, what + ": read " + std::to_string(o->h_pass[5]) + " has 2^32 - 1 windows or more"};
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, o->pass_ev[0], o->pass_ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, o->pass_ev[2], o->pass_ev[3]));
        for (int i = 0; i < 4; ++i) res->sums[i] = o->h_pass[i];
        for (int i = 0; i < 16; ++i) res->counts[i] = o->h_pass[8 + i];
        if (colour) for (int i = 0; i < 65; ++i) res->by_count[i] = o->h_pass[32 + i];
        res->ms = a + b;
    });
}

// The tail of every device form: the pass's status goes on; `info` receives the reads always and, from a pass that
// succeeded, the time and the figures `fill` picks.
template <class Info, class Fill>
int pass_report(int rc, const ReadsPass& res, Info* info, Fill fill)
{
    if (info)
    {
        info->reads = res.reads;
        if (rc == GOSS_OK) { fill(*info); info->ms = res.ms; }
    }
    return rc;
}

// ---- the host forms' batch -------------------------------------------------------------------------------------------------

// a batch on the device, in the buffer the object keeps: the bases, 4 bytes per read in a, b and extra (NULL where the
// caller has no such array), the read starts (NULL likewise)
struct StagedBatch {
    const uint8_t* bases = nullptr;
    uint32_t* a = nullptr;
    uint32_t* b = nullptr;
    uint64_t* starts = nullptr;
    uint32_t* extra = nullptr;
};

// The host forms: the batch goes to the device, and with it `extra`, max_reads values where the caller has some;
// `device_form(batch, &mine)` answers it there, its info is passed on, and 4 bytes per read and array come back (a:
// windows, b: hits / classes; b_bytes = 8: b holds 64-bit words, the colour mode's).  No bytes: the device form on no
// batch.  The only place that lays the staged buffer out.
template <class Info, class Call>
int reads_staged(goss_gpu_object* o, const void* bases, uint64_t nbytes, uint64_t max_reads, uint32_t* a, uint32_t* b, uint64_t* read_starts,
                 const uint32_t* extra, Info* info, Call device_form, uint64_t b_bytes = 4)
{
    StagedBatch s;
    if (nbytes == 0)
    {
        if (read_starts) read_starts[0] = 0;
        return device_form(s, info);
    }
    int rc = obj_guarded(o->device, o->last_error, [&]() {
        const uint64_t b0 = (nbytes + 255) & ~255ULL, each = (max_reads * 4 + 255) & ~255ULL, narrays = (extra ? 3 : 2) + (b_bytes == 8 ? 1 : 0);
        uint8_t* mem = o->staged.room(b0 + narrays * each + (max_reads + 1) * 8);
        s.bases = mem;
        if (a) s.a = (uint32_t*)(mem + b0);
        if (b) s.b = (uint32_t*)(mem + b0 + each);
        if (extra) s.extra = (uint32_t*)(mem + b0 + (narrays - 1) * each);
        if (read_starts) s.starts = (uint64_t*)(mem + b0 + narrays * each);
        HIP_TRY(hipMemcpyAsync(mem, bases, nbytes, hipMemcpyHostToDevice, o->stream));
        if (extra && max_reads) HIP_TRY(hipMemcpyAsync(s.extra, extra, max_reads * 4, hipMemcpyHostToDevice, o->stream));
    });
    if (rc != GOSS_OK) return rc;
    Info mine;
    rc = device_form(s, &mine);
    if (info) *info = mine;
    if (rc != GOSS_OK) return rc;
    const uint64_t reads = mine.reads;
    return obj_guarded(o->device, o->last_error, [&]() {
        if (a && reads) HIP_TRY(hipMemcpyAsync(a, s.a, reads * 4, hipMemcpyDeviceToHost, o->stream));
        if (b && reads) HIP_TRY(hipMemcpyAsync(b, s.b, reads * b_bytes, hipMemcpyDeviceToHost, o->stream));
        if (read_starts) HIP_TRY(hipMemcpyAsync(read_starts, s.starts, (reads + 1) * 8, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
    });
}

// n values per array staged to the device and `call`ed there: ins host arrays in, then `out` back
template <class Call>
int taxo_staged(goss_gpu_object* o, std::initializer_list<const uint32_t*> ins, uint64_t n, uint32_t* out, Call call)
{
    uint32_t* d[3] = {nullptr, nullptr, nullptr};
    int rc = obj_guarded(o->device, o->last_error, [&]() {
        const uint64_t each = (n * 4 + 255) & ~255ULL;
        uint8_t* mem = o->staged.room(3 * each + 256);
        uint32_t k = 0;
        for (const uint32_t* p : ins)
        {
            d[k] = (uint32_t*)(mem + k * each);
            if (n) HIP_TRY(hipMemcpyAsync(d[k], p, n * 4, hipMemcpyHostToDevice, o->stream));
            ++k;
        }
        d[2] = (uint32_t*)(mem + 2 * each);
        HIP_TRY(hipStreamSynchronize(o->stream));
    });
    if (rc != GOSS_OK) return rc;
    rc = call(d[0], d[1], d[2]);
    if (rc != GOSS_OK || !out || !n) return rc;
    return obj_guarded(o->device, o->last_error, [&]() { HIP_TRY(hipMemcpy(out, d[2], n * 4, hipMemcpyDeviceToHost)); });
}

// ---- the classify bitmaps ---------------------------------------------------------------------------------------------------

// goss_gpu_object_classify_bits_host: the pair kept on the device, lhs then rhs
void classify_keep_bits(goss_gpu_object* o, const uint64_t* lhs, const uint64_t* rhs)
{
    const uint64_t nwords = (o->q.s.count + 63) / 64, bytes = nwords * 8;
    if (nwords && !o->classify_bits) HIP_TRY(hipMalloc((void**)&o->classify_bits, 2 * bytes));      // (count never changes)
    if (nwords)
    {
        HIP_TRY(hipMemcpyAsync(o->classify_bits, lhs, bytes, hipMemcpyHostToDevice, o->stream));
        HIP_TRY(hipMemcpyAsync(o->classify_bits + nwords, rhs, bytes, hipMemcpyHostToDevice, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
    }
    o->classify_kept = true;
}

// ---- the colour words -------------------------------------------------------------------------------------------------------

// count words on the device, not yet the object's: freed unless adopt() makes them the kept ones, so a call that
// fails on the way leaves the old words, and the object never holds a second copy
struct FreshColours {
    goss_gpu_object* o;
    unsigned long long* p = nullptr;
    explicit FreshColours(goss_gpu_object* obj) : o(obj)
    {
        const uint64_t z = o->q.s.count;
        if (z && hipMalloc((void**)&p, z * 8) != hipSuccess) { (void)hipGetLastError(); p = nullptr; throw StatusError{GOSS_ERR_OOM, "colours: no device memory for the words"}; }
    }
    FreshColours(const FreshColours&) = delete;
    FreshColours& operator=(const FreshColours&) = delete;
    ~FreshColours() { if (p) (void)hipFree(p); }
    // (the stream is idle: every call on the object is synchronous, so nothing still reads the old words)
    void adopt(uint32_t ncolours)
    {
        HIP_TRY(hipStreamSynchronize(o->stream));
        if (o->colours) (void)hipFree(o->colours);
        o->colours = (uint64_t*)p;
        p = nullptr;
        o->ncolours = ncolours;
        o->colours_kept = true;
    }
};

// goss_gpu_object_colours_host past its argument checks
void colours_keep_host(goss_gpu_object* o, const uint64_t* colours, uint32_t ncolours)
{
    const uint64_t z = o->q.s.count;
    if (ncolours < 64)
        for (uint64_t r = 0; r < z; ++r)
            if (colours[r] >> ncolours)
                throw StatusError{GOSS_ERR_INVALID_ARG, "colours: the word of rank " + std::to_string(r) + " has a bit at or above ncolours = " + std::to_string(ncolours)};
    FreshColours fresh(o);
    if (z) HIP_TRY(hipMemcpyAsync(fresh.p, colours, z * 8, hipMemcpyHostToDevice, o->stream));
    fresh.adopt(ncolours);
}

// goss_gpu_object_colours_from_index past its argument checks: S = N / z words' worth of positions ORed into place
uint32_t colours_keep_index(goss_gpu_object* o, goss_gpu_object* index)
{
    const uint64_t z = o->q.s.count;
    const RdSparse& idx = index->q.s;
    if (!z) throw StatusError{GOSS_ERR_INVALID_ARG, "colours_from_index: the set is empty, so the index's universe cannot be S * count"};
    if (idx.size_hi || idx.size_lo % z) throw StatusError{GOSS_ERR_INVALID_ARG, "colours_from_index: the index's universe is not S * count (count = " + std::to_string(z) + ")"};
    const uint64_t S = idx.size_lo / z;
    if (S < 1 || S > GOSS_ELECT_MAX_COLOURS)
        throw StatusError{GOSS_ERR_INVALID_ARG, "colours_from_index: the index speaks of S = " + std::to_string(S) + " references; S must be 1 .. 64"};
    HIP_TRY(hipStreamSynchronize(index->stream));
    FreshColours fresh(o);
    HIP_TRY(hipMemsetAsync(fresh.p, 0, z * 8, o->stream));
    HIP_TRY(hipMemsetAsync(o->d_bad, 0xFF, 8, o->stream));
    if (idx.count) hipLaunchKernelGGL(elect_colours_from_index_kernel, query_grid(idx.count), dim3(kTB), 0, o->stream, idx, z, (uint32_t)S, fresh.p, o->d_bad);
    HIP_TRY(hipMemcpyAsync(o->h_bad, o->d_bad, 8, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    check_launch("colours_from_index");
    if (*o->h_bad != ~0ULL)
        throw StatusError{GOSS_ERR_INVALID_ARG, "colours_from_index: stored position " + std::to_string(*o->h_bad >> 2) + " of the index cannot be read, or lies at or past S * count (damaged object)"};
    fresh.adopt((uint32_t)S);
    return (uint32_t)S;
}

// ---- the taxonomy: the tree, the annotation, the empty set -------------------------------------------------------------------

// goss_gpu_object_taxo_tree_host past its NULL checks: the n nodes checked, numbered in pre-order and kept on the device
void taxo_build_tree(goss_gpu_object* o, uint32_t n, const uint32_t* ids, const uint32_t* parent_index)
{
    auto refuse = [](const std::string& msg) { throw StatusError{GOSS_ERR_INVALID_ARG, "taxo_tree: " + msg}; };
    // one root, parents in range, ids usable and distinct
    uint32_t root = n;
    for (uint32_t i = 0; i < n; ++i)
    {
        if (parent_index[i] >= n) refuse("node " + std::to_string(i) + " names parent " + std::to_string(parent_index[i]) + " of " + std::to_string(n));
        if (ids[i] == GOSS_TAXO_NONE || ids[i] == GOSS_TAXO_MANY) refuse("node " + std::to_string(i) + " has the reserved id " + std::to_string(ids[i]));
        if (parent_index[i] != i) continue;
        if (root != n) refuse("nodes " + std::to_string(root) + " and " + std::to_string(i) + " are both their own parent");
        root = i;
    }
    if (root == n) refuse("no node is its own parent");
    std::vector<uint32_t> by_id(n);
    for (uint32_t i = 0; i < n; ++i) by_id[i] = i;
    std::sort(by_id.begin(), by_id.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
    for (uint32_t i = 1; i < n; ++i)
        if (ids[by_id[i]] == ids[by_id[i - 1]]) refuse("node id " + std::to_string(ids[by_id[i]]) + " occurs twice");
    // children in the order given (a counting sort by parent), then pre-order numbers without recursion
    std::vector<uint32_t> first(n + 1, 0), kids(n ? n - 1 : 0);
    for (uint32_t i = 0; i < n; ++i) if (i != root) ++first[parent_index[i] + 1];
    for (uint32_t i = 0; i < n; ++i) first[i + 1] += first[i];
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        for (uint32_t i = 0; i < n; ++i) if (i != root) kids[at[parent_index[i]]++] = i;
    }
    std::vector<uint32_t> pre(n, 0xFFFFFFFFu), tab(5 * (uint64_t)n), next(n, 0), stack;
    uint32_t* parent = tab.data(); uint32_t* last = parent + n; uint32_t* id = last + n; uint32_t* sid = id + n; uint32_t* scl = sid + n;
    uint32_t seen = 0;
    pre[root] = seen++;
    parent[0] = 0;
    id[0] = ids[root];
    stack.push_back(root);
    while (!stack.empty())
    {
        const uint32_t v = stack.back();
        if (next[v] < first[v + 1] - first[v])
        {
            const uint32_t c = kids[first[v] + next[v]++];
            pre[c] = seen++;
            parent[pre[c]] = pre[v];
            id[pre[c]] = ids[c];
            stack.push_back(c);
        }
        else
        {
            last[pre[v]] = seen - 1;
            stack.pop_back();
        }
    }
    if (seen != n)
        for (uint32_t i = 0; i < n; ++i)
            if (pre[i] == 0xFFFFFFFFu) refuse("node " + std::to_string(i) + " does not hang under the root");
    for (uint32_t i = 0; i < n; ++i) { sid[i] = ids[by_id[i]]; scl[i] = pre[by_id[i]] + 1; }

    const uint64_t tab_bytes = (5 * (uint64_t)n * 4 + 7) & ~7ULL;
    uint32_t* mem = nullptr;
    if (hipMalloc((void**)&mem, tab_bytes + ((uint64_t)n + 2) * 8) != hipSuccess) { (void)hipGetLastError(); throw StatusError{GOSS_ERR_OOM, "taxo_tree: no device memory for the tree"}; }
    if (hipMemcpy(mem, tab.data(), 5 * (uint64_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(mem); throw StatusError{GOSS_ERR_HIP, "taxo_tree: the copy of the tree failed"}; }
    HIP_TRY(hipStreamSynchronize(o->stream));
    if (o->taxo_tree) (void)hipFree(o->taxo_tree);
    o->taxo_tree = mem;
    o->taxo_bins = (unsigned long long*)((uint8_t*)mem + tab_bytes);
    o->taxo_n = n;
    o->taxo_pre.swap(pre);
    o->taxo_ann_kept = false;                // (its classes were the old tree's numbers)
}

// goss_gpu_object_taxo_annotation_host on a set with k-mers: `ann` as classes (none everywhere without one) becomes the kept one
void taxo_keep_annotation(goss_gpu_object* o, const uint32_t* ann)
{
    const uint64_t z = o->q.s.count;
    if (!o->taxo_ann && hipMalloc((void**)&o->taxo_ann, z * 4) != hipSuccess) { (void)hipGetLastError(); o->taxo_ann = nullptr; throw StatusError{GOSS_ERR_OOM, "taxo_annotation: no device memory for the annotation"}; }
    if (!ann) HIP_TRY(hipMemsetAsync(o->taxo_ann, 0, z * 4, o->stream));
    else
    {
        // converted beside the kept one, which an unknown id leaves as it was
        const uint64_t each = (z * 4 + 255) & ~255ULL;
        uint8_t* tmp = o->taxo_scratch.room(2 * each);
        HIP_TRY(hipMemcpyAsync(tmp, ann, z * 4, hipMemcpyHostToDevice, o->stream));
        taxo_dense(o, "taxo_annotation", "rank", (const uint32_t*)tmp, z, kTaxoAllowNone, (uint32_t*)(tmp + each));
        HIP_TRY(hipMemcpyAsync(o->taxo_ann, tmp + each, z * 4, hipMemcpyDeviceToDevice, o->stream));
    }
    HIP_TRY(hipStreamSynchronize(o->stream));
    o->taxo_ann_kept = true;
}

// goss_gpu_object_taxo_annotation_read on a set with k-mers: the kept annotation as node ids, the ranks per node
void taxo_read_annotation(goss_gpu_object* o, uint32_t* ann_out, uint64_t* counts_out)
{
    const uint64_t z = o->q.s.count;
    if (counts_out)
    {
        taxo_tally(o, o->taxo_ann, z);
        std::vector<uint64_t> counts((uint64_t)o->taxo_n + 2);
        taxo_bins_out(o, counts.data());
        std::copy(counts.begin(), counts.end() - 2, counts_out);
    }
    if (ann_out)
    {
        uint32_t* tmp = (uint32_t*)o->taxo_scratch.room(z * 4);
        hipLaunchKernelGGL(taxo_ids_kernel, taxo_grid(z), dim3(kTB), 0, o->stream, (const uint32_t*)o->taxo_ann, z, taxo_tables(o).id, tmp);
        HIP_TRY(hipMemcpyAsync(ann_out, tmp, z * 4, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        check_launch("taxo_annotation_read");
    }
}

// the result of a taxo call on an empty set: the reads counted and their windows, no hit anywhere (must_fit: annotate,
// whose node ids are per read; the pass itself refuses a batch that does not fit)
int taxo_empty_pass(goss_gpu_object* o, const char* what, const void* d_bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads, uint32_t* d_result,
                    uint32_t* d_windows, uint64_t* d_read_starts, bool must_fit, goss_gpu_taxo_info* info)
{
    ReadsPass res;
    int rc = reads_pass(o, ReadsJob{what, kModeCount, d_bases, nbytes, flags, max_reads, d_windows, nullptr, d_read_starts, must_fit}, &res);
    if (rc == GOSS_OK && d_result && res.reads)
        rc = obj_guarded(o->device, o->last_error, [&]() {
            HIP_TRY(hipMemsetAsync(d_result, 0xFF, res.reads * 4, o->stream));       // (GOSS_TAXO_NONE)
            HIP_TRY(hipStreamSynchronize(o->stream));
        });
    return pass_report(rc, res, info, [&](goss_gpu_taxo_info& i) { i.windows = res.sums[0]; i.none = must_fit ? 0 : res.reads; });
}

// goss_gpu_object_taxo_pair past its checks: out[i] = the lca of the node ids a[i] and b[i] (device arrays)
void taxo_pair(goss_gpu_object* o, const uint32_t* d_a, const uint32_t* d_b, uint64_t n, uint32_t* d_out)
{
    const TaxoTables t = taxo_tables(o);
    HIP_TRY(hipMemsetAsync(o->d_bad, 0xFF, 8, o->stream));
    hipLaunchKernelGGL(taxo_pair_kernel, taxo_grid(n), dim3(kTB), 0, o->stream, d_a, d_b, n, t.sorted_id, t.sorted_class, t.last, t.id, o->taxo_n, d_out, o->d_bad);
    HIP_TRY(hipMemcpyAsync(o->h_bad, o->d_bad, 8, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    check_launch("taxo_pair");
    if (*o->h_bad != ~0ULL) throw StatusError{GOSS_ERR_INVALID_ARG, "taxo_pair: pair " + std::to_string(*o->h_bad) + " holds a node id the tree lacks"};
}

}  // namespace
