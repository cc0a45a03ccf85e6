// emit_path.hpp -- from a finished result to the files of gossamer's on-disk objects.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, after chunk_loop.hpp and ahead of graph_passes.hpp,
// which writes its own objects through the same arrays): the IntegerArray column layout, DenseSelect (whole, per range,
// composed), SparseArray (header, index, low bits), VariableByteArray and the counts histogram, and the three ways to
// an object -- emit_object on one device, emit_part on a range's owner and emit_assemble where the parts meet.
// The entry points (goss_gpu_emit*, goss_gpu_emit_sparse_array, ...) stay in goss_gpu.hip and only call in here.
// Every function takes its temporaries under an ArenaScope of its own; what it leaves -- the file images -- is
// permanent room, listed in build.files by add_dev_file / add_host_file.
#pragma once

void add_host_file(goss_gpu_ctx* c, const std::string& suffix, const void* p, size_t n)
{
    OutFile f; f.suffix = suffix; f.size = n;
    f.host.assign((const uint8_t*)p, (const uint8_t*)p + n);
    c->build.files.push_back(std::move(f));
}
// ... and a file whose image lies on the device (permanent room of the arena)
void add_dev_file(goss_gpu_ctx* c, const std::string& suffix, const void* dev, uint64_t size)
{
    OutFile f; f.suffix = suffix; f.size = size; f.dev = (const uint8_t*)dev;
    c->build.files.push_back(std::move(f));
}

struct IaCol { std::string suffix; uint32_t bytes; uint32_t shift; };

// IntegerArray::builder column layout (IntegerArray.cc:259-357, StackedArray.hh:152-178).
bool ia_layout(uint32_t bits, const std::string& prefix, uint32_t shift, std::vector<IaCol>& out)
{
    uint32_t ub = 0, lb = 0;
    switch (bits)
    {
        case 8: case 16: case 32: case 64: out.push_back({prefix, bits / 8, shift}); return true;
        case 24: ub = 8; lb = 16; break;
        case 40: ub = 8; lb = 32; break;
        case 48: ub = 16; lb = 32; break;
        case 56: ub = 8; lb = 48; break;
        case 72: ub = 8; lb = 64; break;
        case 80: ub = 16; lb = 64; break;
        case 88: ub = 8; lb = 80; break;
        case 96: ub = 32; lb = 64; break;
        case 104: ub = 8; lb = 96; break;
        case 112: ub = 16; lb = 96; break;
        case 120: ub = 24; lb = 96; break;
        case 128: ub = 64; lb = 64; break;
        default: return false;
    }
    return ia_layout(ub, prefix + ".upr", shift + lb, out) && ia_layout(lb, prefix + ".lwr", shift, out);
}

// SparseArray::Builder::d (SparseArray.cc:47-72).
uint64_t sparse_d(uint64_t n_lo, uint64_t n_hi, uint64_t M)
{
    double scale = 18446744073709551616.0;
    double n = (double)n_hi * scale + (double)n_lo;
    double m = (double)M;
    double d0 = std::log2(n / ((1 + m) * 1.4426950408889634));
    uint64_t d = (uint64_t)std::ceil(d0);
    if (d < 8) d = 8; else if (d > 128) d = 128;
    return d;
}

struct DsHeader {
    uint64_t version, flags, indexArrayOffset, rankArrayOffset;
    uint64_t logBlockSize, blockSize, logSampleRate, sampleRate;
    uint64_t numBlocks, indexSize, smallBlocks, smallBlocksSize;
    uint64_t intermediateBlocks, intermediateBlocksSize, largeBlocks, largeBlocksSize;
};
static_assert(sizeof(DsHeader) == 128, "DenseSelect header is 128 bytes");

// DenseSelect file image over the virtual position sequence (DenseArray.cc:446-694).
template <class K>
void emit_dense_select(goss_gpu_ctx* c, const K* keys, uint64_t m, uint32_t D, int invert, uint64_t count,
                       const std::string& suffix)
{
    const uint64_t nblocks = (count + 8191) >> 13;
    DsHeader h{};
    h.version = 2012092701ULL;
    h.flags = invert ? 1 : 0;
    h.logBlockSize = 13; h.blockSize = 8192; h.logSampleRate = 6; h.sampleRate = 64;
    std::vector<uint32_t> btype(nblocks);
    std::vector<uint64_t> bbytes(nblocks), boff(nblocks);
    ArenaScope scope(c->arena);
    uint32_t* d_btype = nullptr; uint64_t* d_bbytes = nullptr; uint64_t* d_brank = nullptr; uint64_t* d_boff = nullptr;
    if (nblocks)
    {
        d_btype = (uint32_t*)c->arena.temp(nblocks * 4);
        d_bbytes = (uint64_t*)c->arena.temp(nblocks * 8);
        d_brank = (uint64_t*)c->arena.temp(nblocks * 8);
        d_boff = (uint64_t*)c->arena.temp(nblocks * 8);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ds_classify_kernel<K>), dim3(grid_for(nblocks, 64)), dim3(64), 0, c->stream,
                           DsSrc<K>{keys, m, D, invert, 0, nullptr, 0}, count, (uint64_t)0, nblocks, d_btype, d_bbytes, d_brank);
        HIP_TRY(hipMemcpyAsync(btype.data(), d_btype, nblocks * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(bbytes.data(), d_bbytes, nblocks * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    uint64_t pos = 4096;
    for (uint64_t b = 0; b < nblocks; ++b)
    {
        boff[b] = pos;
        uint64_t cnt = std::min<uint64_t>(8192, count - (b << 13));
        switch (btype[b])
        {
            case kDsSmall: h.smallBlocks++; h.smallBlocksSize += 256; break;
            case kDsIntermediate: h.intermediateBlocks++; h.intermediateBlocksSize += bbytes[b]; break;
            case kDsSpill32: h.largeBlocks++; h.largeBlocksSize += cnt * 4; break;
            default: h.largeBlocks++; h.largeBlocksSize += cnt * 8; break;
        }
        pos += bbytes[b];
    }
    h.numBlocks = nblocks;
    pos = (pos + 15) & ~15ULL;
    h.indexArrayOffset = pos;
    h.rankArrayOffset = pos + nblocks * 8;
    h.indexSize = nblocks * 16;
    const uint64_t size = pos + nblocks * 16;
    uint8_t* image = (uint8_t*)c->arena.perm(size);
    HIP_TRY(hipMemsetAsync(image, 0, size, c->stream));
    HIP_TRY(hipMemcpyAsync(image, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    if (nblocks)
    {
        HIP_TRY(hipMemcpyAsync(d_boff, boff.data(), nblocks * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ds_fill_kernel<K>), dim3((uint32_t)nblocks), dim3(128), 0, c->stream,
                           DsSrc<K>{keys, m, D, invert, 0, nullptr, 0}, count, (uint64_t)0, (const uint32_t*)d_btype, (const uint64_t*)d_boff,
                           (const uint64_t*)d_brank, image, (uint64_t*)(image + h.indexArrayOffset));
        HIP_TRY(hipMemcpyAsync(image + h.rankArrayOffset, d_brank, nblocks * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));    // host vectors / header go out of scope
    add_dev_file(c, suffix, image, size);
}

// ---- DenseSelect blocks per range (round 5) ---------------------------------------------------------------------------
// A block of 8192 indexed positions is a function of those positions alone (DenseArray.cc:446-647): type, bytes and body.
// A range's owner builds the blocks that lie wholly inside its share of the ones (or zeros); the assembler builds the few
// that straddle two ranges from the bitmap, adds up the sizes, copies the bodies to their offsets and writes the master
// index and the rank array.  A range's blocks travel as ONE record: {nb, payload bytes, 0, 0}, bytes[nb], rank[nb],
// type[nb] (u32, padded to 8), the bodies back to back.
constexpr uint64_t kPartSpan = 1, kPartDs = 2;          // kinds of the records of a ".part.span" file: {kind, a, b, body bytes}, the body
struct DsPlan { uint64_t b0 = 0, nb = 0, payload = 0; std::vector<uint32_t> type; std::vector<uint64_t> bytes, rank; uint32_t* d_type = nullptr; uint64_t* d_rank = nullptr; };
static inline uint64_t ds_record_bytes(const DsPlan& p) { return 32 + p.nb * 16 + ((p.nb * 4 + 7) & ~7ULL) + p.payload; }

// types, sizes and first positions of blocks b0 .. b0 + nb - 1 (temporaries of the arena stay for ds_fill_record)
template <class K>
DsPlan ds_plan(goss_gpu_ctx* c, const DsSrc<K>& src, uint64_t count, uint64_t b0, uint64_t nb)
{
    DsPlan p; p.b0 = b0; p.nb = nb;
    if (!nb) return p;
    p.type.resize(nb); p.bytes.resize(nb); p.rank.resize(nb);
    p.d_type = (uint32_t*)c->arena.temp(nb * 4);
    uint64_t* d_bytes = (uint64_t*)c->arena.temp(nb * 8);
    p.d_rank = (uint64_t*)c->arena.temp(nb * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ds_classify_kernel<K>), dim3(grid_for(nb, 64)), dim3(64), 0, c->stream, src, count, b0, nb, p.d_type, d_bytes, p.d_rank);
    HIP_TRY(hipMemcpyAsync(p.type.data(), p.d_type, nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(p.bytes.data(), d_bytes, nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(p.rank.data(), p.d_rank, nb * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint64_t b = 0; b < nb; ++b) p.payload += p.bytes[b];
    return p;
}
// the record of a plan at `at` (ds_record_bytes(p) bytes, zeroed by the caller)
template <class K>
void ds_fill_record(goss_gpu_ctx* c, const DsSrc<K>& src, uint64_t count, const DsPlan& p, uint8_t* at)
{
    const uint64_t head[4] = {p.nb, p.payload, 0, 0};
    HIP_TRY(hipMemcpyAsync(at, head, 32, hipMemcpyHostToDevice, c->stream));
    if (p.nb)
    {
        uint8_t* a_bytes = at + 32; uint8_t* a_rank = a_bytes + p.nb * 8; uint8_t* a_type = a_rank + p.nb * 8;
        uint8_t* body = a_type + ((p.nb * 4 + 7) & ~7ULL);
        std::vector<uint64_t> boff(p.nb);
        uint64_t pos = 0;
        for (uint64_t b = 0; b < p.nb; ++b) { boff[b] = pos; pos += p.bytes[b]; }
        uint64_t* d_boff = (uint64_t*)c->arena.temp(p.nb * 8);
        HIP_TRY(hipMemcpyAsync(d_boff, boff.data(), p.nb * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(a_bytes, p.bytes.data(), p.nb * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(a_rank, p.d_rank, p.nb * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(a_type, p.d_type, p.nb * 4, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ds_fill_kernel<K>), dim3((uint32_t)p.nb), dim3(128), 0, c->stream, src, count, p.b0, (const uint32_t*)p.d_type,
                           (const uint64_t*)d_boff, (const uint64_t*)p.d_rank, body, (uint64_t*)nullptr);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));          // (host vectors go out of scope)
}

// A DenseSelect file from the records of the ranges (device addresses on this context's device: `recs` = {first block, the
// record}) and, for every block none of them holds, from the assembled bitmap (words, nwords, ones before every word).
void ds_compose(goss_gpu_ctx* c, int invert, uint64_t count, const std::vector<std::pair<uint64_t, const uint8_t*>>& recs,
                const unsigned long long* words, uint64_t nwords, const uint64_t* before, const std::string& suffix)
{
    const uint64_t NB = (count + 8191) >> 13;
    std::vector<uint32_t> type(NB);
    std::vector<uint64_t> bytes(NB), rank(NB), boff(NB);
    std::vector<uint8_t> have(NB, 0);
    struct Seg { uint64_t b0, nb; const uint8_t* body; uint64_t payload; };
    std::vector<Seg> segs;
    ArenaScope scope(c->arena);
    for (auto& r : recs)
    {
        uint64_t head[4];
        HIP_TRY(hipMemcpyAsync(head, r.second, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint64_t b0 = r.first, nb = head[0];
        if (!nb) continue;
        if (b0 + nb > NB) throw StatusError{GOSS_ERR_INVALID_ARG, "emit_assemble: a range's blocks lie beyond the array"};
        const uint8_t* a_bytes = r.second + 32; const uint8_t* a_rank = a_bytes + nb * 8; const uint8_t* a_type = a_rank + nb * 8;
        HIP_TRY(hipMemcpyAsync(bytes.data() + b0, a_bytes, nb * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rank.data() + b0, a_rank, nb * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(type.data() + b0, a_type, nb * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint64_t b = b0; b < b0 + nb; ++b) { if (have[b]) throw StatusError{GOSS_ERR_INVALID_ARG, "emit_assemble: a block built twice"}; have[b] = 1; }
        c->stats.ds_blocks_ranges += nb;
        segs.push_back({b0, nb, a_type + ((nb * 4 + 7) & ~7ULL), head[1]});
    }
    // the blocks nobody built (they straddle two ranges, or their range gave no record): runs of them, from the bitmap
    struct Own { DsPlan plan; uint64_t* pos; uint64_t first; uint8_t* rec; };
    std::vector<Own> own;
    for (uint64_t b = 0; b < NB;)
    {
        if (have[b]) { ++b; continue; }
        uint64_t e = b;
        while (e < NB && !have[e] && e - b < 4096) ++e;          // (at most 32 M positions at a time)
        const uint64_t first = b << 13, n = std::min<uint64_t>(count, e << 13) - first;
        uint64_t* pos = (uint64_t*)c->arena.temp(n * 8);
        hipLaunchKernelGGL(ef_select_range_kernel, dim3(grid_for(n, kTB)), dim3(kTB), 0, c->stream, words, nwords, before, first, n, invert, pos);
        const DsSrc<Key1> src{nullptr, 0, 0, invert, 0, pos, first};
        Own o; o.pos = pos; o.first = first;
        o.plan = ds_plan<Key1>(c, src, count, b, e - b);
        const uint64_t rb = ds_record_bytes(o.plan);
        o.rec = (uint8_t*)c->arena.temp(rb);
        HIP_TRY(hipMemsetAsync(o.rec, 0, rb, c->stream));
        ds_fill_record<Key1>(c, src, count, o.plan, o.rec);
        for (uint64_t x = b; x < e; ++x) { type[x] = o.plan.type[x - b]; bytes[x] = o.plan.bytes[x - b]; rank[x] = o.plan.rank[x - b]; have[x] = 1; }
        segs.push_back({b, e - b, o.rec + 32 + (e - b) * 16 + (((e - b) * 4 + 7) & ~7ULL), o.plan.payload});
        own.push_back(std::move(o));
        c->stats.ds_blocks_own += e - b;
        b = e;
    }
    DsHeader h{};
    h.version = 2012092701ULL;
    h.flags = invert ? 1 : 0;
    h.logBlockSize = 13; h.blockSize = 8192; h.logSampleRate = 6; h.sampleRate = 64;
    uint64_t pos = 4096;
    for (uint64_t b = 0; b < NB; ++b)
    {
        boff[b] = pos;
        const uint64_t cnt = std::min<uint64_t>(8192, count - (b << 13));
        switch (type[b])
        {
            case kDsSmall: h.smallBlocks++; h.smallBlocksSize += 256; break;
            case kDsIntermediate: h.intermediateBlocks++; h.intermediateBlocksSize += bytes[b]; break;
            case kDsSpill32: h.largeBlocks++; h.largeBlocksSize += cnt * 4; break;
            default: h.largeBlocks++; h.largeBlocksSize += cnt * 8; break;
        }
        pos += bytes[b];
    }
    h.numBlocks = NB;
    pos = (pos + 15) & ~15ULL;
    h.indexArrayOffset = pos;
    h.rankArrayOffset = pos + NB * 8;
    h.indexSize = NB * 16;
    const uint64_t size = pos + NB * 16;
    // (the image is permanent, the temporaries above it go with the scope: it goes first in the arena's order -- taken
    // from the permanent end, which grows from the other side)
    uint8_t* image = (uint8_t*)c->arena.perm(size);
    HIP_TRY(hipMemsetAsync(image, 0, size, c->stream));
    HIP_TRY(hipMemcpyAsync(image, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    for (auto& sg : segs)
        if (sg.payload) HIP_TRY(hipMemcpyAsync(image + boff[sg.b0], sg.body, sg.payload, hipMemcpyDeviceToDevice, c->stream));
    for (uint64_t b = 0; b < NB; ++b) boff[b] |= type[b];          // the master index entries
    if (NB)
    {
        HIP_TRY(hipMemcpyAsync(image + h.indexArrayOffset, boff.data(), NB * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(image + h.rankArrayOffset, rank.data(), NB * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    add_dev_file(c, suffix, image, size);
}

struct SaHeader { uint64_t version, D, quantizedD, mask_lo, mask_hi, size_lo, size_hi, count; };
static_assert(sizeof(SaHeader) == 64, "SparseArray header is 64 bytes");

// nd = Nend >> D, which must fit 64 bits (SparseArray.cc:79-86)
uint64_t sparse_nd(uint32_t D, uint64_t Nend_lo, uint64_t Nend_hi)
{
    if (D >= 128) return 0;
    if (D >= 64) return Nend_hi >> (D - 64);
    if (D > 0 && (Nend_hi >> D) != 0) throw StatusError{GOSS_ERR_TOO_LARGE, "Internal error in SparseArray; nd does not fit 64 bits"};
    if (D == 0 && Nend_hi) throw StatusError{GOSS_ERR_TOO_LARGE, "Internal error in SparseArray; nd does not fit 64 bits"};
    return D == 0 ? Nend_lo : ((Nend_lo >> D) | (Nend_hi << (64 - D)));
}

// SparseArray::Header (SparseArray.hh:60-72) as the ".header" file
void emit_sparse_header(goss_gpu_ctx* c, uint32_t D, uint64_t Nend_lo, uint64_t Nend_hi, uint64_t count, const std::string& base)
{
    SaHeader h{};
    h.version = 2012030501ULL; h.D = D; h.quantizedD = 8 * ((D + 7) / 8);
    if (D >= 128) { h.mask_lo = ~0ULL; h.mask_hi = ~0ULL; }
    else if (D >= 64) { h.mask_lo = ~0ULL; h.mask_hi = D == 64 ? 0 : ((1ULL << (D - 64)) - 1); }
    else { h.mask_lo = (1ULL << D) - 1; h.mask_hi = 0; }
    h.size_lo = Nend_lo; h.size_hi = Nend_hi; h.count = count;
    add_host_file(c, base + ".header", &h, sizeof h);
}

// The index part of a SparseArray: high-bits bitmap, -d0 (zeros), -d1 (ones), from keys whose high part
// is key >> D -- or from the high parts themselves with D = 0 (distributed emission).
template <class K>
void emit_sparse_index(goss_gpu_ctx* c, const K* keys, uint64_t m, uint32_t D, uint64_t nd, const std::string& base, uint64_t* built = nullptr)
{
    const uint64_t nwords = (nd + m + 3) / 64 + 1;
    uint64_t* words = built ? built : (uint64_t*)c->arena.perm(nwords * 8);
    if (built) {}                                // (assembled from the ranges' spans: emit_assemble)
    else if (m >= (1u << 16))
    {
        // from the keys' side: one coalesced pass over the keys (below 65 536 keys: the per-word binary search)
        HIP_TRY(hipMemsetAsync(words, 0, nwords * 8, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_high_bits_keys_kernel<K>), dim3(grid_for(m, kEfChunk)), dim3(kTB), 0, c->stream,
                           keys, m, D, (uint64_t)0, nwords, (unsigned long long*)words, (uint64_t)0);
    }
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_high_bits_kernel<K>), dim3(grid_for(nwords, 256)), dim3(256), 0, c->stream,
                           keys, m, D, nwords, words);
    add_dev_file(c, base + ".high-bits", words, nwords * 8);
    emit_dense_select<K>(c, keys, m, D, 1, nd + 2, base + "-d0");
    emit_dense_select<K>(c, keys, m, D, 0, m, base + "-d1");
}

// The low-bits column files of m keys (IntegerArray / StackedArray columns of quantizedD bits)
template <class K>
void emit_sparse_low_bits(goss_gpu_ctx* c, const K* keys, uint64_t m, uint32_t D, const std::string& base)
{
    const uint32_t qD = 8 * ((D + 7) / 8);
    std::vector<IaCol> cols;
    if (!ia_layout(qD, "", 0, cols)) throw StatusError{GOSS_ERR_INVALID_ARG, "IntegerArray::builder: unsupported integer width"};
    EfColumns ec{};
    ec.n = (uint32_t)cols.size();
    for (size_t i = 0; i < cols.size(); ++i)
    {
        uint8_t* dst = (uint8_t*)c->arena.perm(std::max<uint64_t>(m * cols[i].bytes, 8));
        ec.c[i] = EfColumn{dst, cols[i].bytes, cols[i].shift};
        add_dev_file(c, base + ".low-bits" + cols[i].suffix, dst, m * cols[i].bytes);
    }
    if (m)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_low_bits_kernel<K>), dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                           keys, m, D, ec);
}

// Every key's high part (key >> D) must fit 64 bits too (SparseArray.hh:91-95).  begin queues the check ahead of the
// kernels that write the files; end, behind them, reads its flag and refuses.
template <class K>
void high_bits_check_begin(goss_gpu_ctx* c, const K* keys, uint64_t m, uint32_t D)
{
    HIP_TRY(hipMemsetAsync(c->d_flags + 1, 0, 4, c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_check_kernel<K>), dim3(1), dim3(64), 0, c->stream, keys, m, D, c->d_flags + 1);
}
void high_bits_check_end(goss_gpu_ctx* c)
{
    uint32_t* hf = (uint32_t*)c->h_pinned;
    HIP_TRY(hipMemcpyAsync(hf, c->d_flags + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hf[0]) throw StatusError{GOSS_ERR_TOO_LARGE, "SparseArray::push_back: high bits do not fit 64 bits"};
}

// SparseArray at suffix `base` (SparseArray::Builder ctor + push_back* + end).
template <class K>
void emit_sparse_array(goss_gpu_ctx* c, const K* keys, uint64_t m, uint64_t N_lo, uint64_t N_hi, uint64_t Mest,
                       uint64_t Nend_lo, uint64_t Nend_hi, const std::string& base)
{
    const uint32_t D = (uint32_t)sparse_d(N_lo, N_hi, Mest);
    const uint64_t nd = sparse_nd(D, Nend_lo, Nend_hi);
    high_bits_check_begin<K>(c, keys, m, D);
    emit_sparse_header(c, D, Nend_lo, Nend_hi, m, base);
    emit_sparse_index<K>(c, keys, m, D, nd, base);
    emit_sparse_low_bits<K>(c, keys, m, D, base);
    high_bits_check_end(c);
}

// The first step of a VariableByteArray (VariableByteArray.hh:76-118): ord0, the low byte of every count, and in
// slot[0, m] the rank of every entry above 255 among those.  Returns how many there are.
uint64_t vba_ord0(goss_gpu_ctx* c, const uint32_t* counts, uint64_t m, uint8_t* ord0, uint64_t* slot)
{
    hipLaunchKernelGGL(vba_ord0_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m, ord0, slot);
    return scan_total(c, slot, m);
}

// Histogram of a u32 count column (m > 0) as (count, frequency), ascending: the counts sorted as keys and run-length
// encoded.  mute_sort: the sort's passes stay out of the per-kernel timing.
std::map<uint64_t, uint64_t> count_histogram(goss_gpu_ctx* c, const uint32_t* counts, uint64_t m, bool mute_sort)
{
    ArenaScope scope(c->arena);
    Key1* ka = (Key1*)c->arena.temp(m * 8);
    Key1* kb = (Key1*)c->arena.temp(m * 8);
    hipLaunchKernelGGL(widen_counts_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m, ka);
    const bool in_b = [&]() { Scoped<bool> mute(&c->mute_timing, c->mute_timing || mute_sort); return radix_sort<Key1, false>(c, ka, kb, nullptr, nullptr, m, 4); }();
    const Key1* sorted = in_b ? kb : ka;
    Key1* distinct = in_b ? ka : kb;
    const uint64_t ntiles = (m + kRedTile - 1) / kRedTile;
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(heads_count_kernel<Key1>), dim3(grid_for(m, kRedTile)), dim3(kTB), 0, c->stream,
                       sorted, m, tile_counts);
    const uint64_t nv = scan_total(c, tile_counts, ntiles);
    uint64_t* starts = (uint64_t*)c->arena.temp(std::max<uint64_t>(nv, 1) * 8);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(heads_write_kernel<Key1>), dim3(grid_for(m, kRedTile)), dim3(kTB), 0, c->stream,
                       sorted, m, (const uint64_t*)tile_counts, distinct, starts);
    std::vector<uint64_t> hv(nv), hs(nv);
    HIP_TRY(hipMemcpyAsync(hv.data(), distinct, nv * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hs.data(), starts, nv * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::map<uint64_t, uint64_t> hist;
    for (uint64_t i = 0; i < nv; ++i) hist[hv[i]] = (i + 1 < nv ? hs[i + 1] : m) - hs[i];
    // the result's counts beyond 32 bits sit in the array modulo 2^32; the histogram is keyed by the count
    // itself (Graph.hh:101-106: mHist[count]++ on the u64 before it is narrowed)
    if (counts == c->build.res_counts)
        for (auto& kv : c->build.res_big)
        {
            auto it = hist.find(kv.second & 0xFFFFFFFFULL);
            if (it != hist.end() && --it->second == 0) hist.erase(it);
            hist[kv.second] += 1;
        }
    return hist;
}
// ... and as the text of a "-counts-hist.txt" (Graph.cc:131-150)
std::string histogram_text(const std::map<uint64_t, uint64_t>& hist)
{
    std::string text;
    char line[64];
    for (auto& kv : hist)
    {
        int l = snprintf(line, sizeof line, "%llu\t%llu\n", (unsigned long long)kv.first, (unsigned long long)kv.second);
        text.append(line, (size_t)l);
    }
    return text;
}

// VariableByteArray + counts histogram (VariableByteArray.hh:76-118, Graph.cc:115-134) of any u32 column on the
// device.  out_hist empty: no histogram file; hist_lines: the number of distinct values the histogram lists.
void emit_counts(goss_gpu_ctx* c, const uint32_t* counts, uint64_t m, uint64_t num_items, const std::string& out_counts, const std::string& out_hist,
                 uint64_t* hist_lines = nullptr)
{
    ArenaScope scope(c->arena);
    uint8_t* ord0 = (uint8_t*)c->arena.perm(std::max<uint64_t>(m, 8));
    uint64_t n1 = 0, n2 = 0;
    Key1* pos1 = nullptr; uint8_t* ord1 = nullptr; Key1* pos2 = nullptr; uint16_t* ord2 = nullptr;
    if (m)
    {
        uint64_t* slot = (uint64_t*)c->arena.temp((m + 1) * 8);
        n1 = vba_ord0(c, counts, m, ord0, slot);
        pos1 = (Key1*)c->arena.perm(std::max<uint64_t>(n1 * 8, 8));
        ord1 = (uint8_t*)c->arena.perm(std::max<uint64_t>(n1, 8));
        if (n1)
        {
            uint32_t* hi16 = (uint32_t*)c->arena.temp(n1 * 4);
            uint64_t* slot2 = (uint64_t*)c->arena.temp((n1 + 1) * 8);
            hipLaunchKernelGGL(vba_ord1_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m,
                               (const uint64_t*)slot, n1, (uint64_t*)pos1, ord1, hi16);
            hipLaunchKernelGGL(vba_flag2_kernel, dim3(grid_for(n1, 256)), dim3(256), 0, c->stream, (const uint32_t*)hi16, n1, slot2);
            n2 = scan_total(c, slot2, n1);
            pos2 = (Key1*)c->arena.perm(std::max<uint64_t>(n2 * 8, 8));
            ord2 = (uint16_t*)c->arena.perm(std::max<uint64_t>(n2 * 2, 8));
            if (n2)
                hipLaunchKernelGGL(vba_ord2_kernel, dim3(grid_for(n1, 256)), dim3(256), 0, c->stream, (const uint32_t*)hi16, n1,
                                   (const uint64_t*)slot2, (uint64_t*)pos2, ord2);
        }
    }
    if (!pos1) pos1 = (Key1*)c->arena.perm(8);
    if (!pos2) pos2 = (Key1*)c->arena.perm(8);
    if (!ord1) ord1 = (uint8_t*)c->arena.perm(8);
    if (!ord2) ord2 = (uint16_t*)c->arena.perm(8);
    add_dev_file(c, out_counts + ".ord0", ord0, m);
    const uint64_t mest = (uint64_t)((double)num_items * 0.001);
    emit_sparse_array<Key1>(c, pos1, n1, num_items, 0, mest, m, 0, out_counts + ".ord1p");
    add_dev_file(c, out_counts + ".ord1", ord1, n1);
    emit_sparse_array<Key1>(c, pos2, n2, num_items, 0, mest, n1, 0, out_counts + ".ord2p");
    add_dev_file(c, out_counts + ".ord2", ord2, n2 * 2);

    std::map<uint64_t, uint64_t> hist;
    if (m && !out_hist.empty()) hist = count_histogram(c, counts, m, false);
    if (hist_lines) *hist_lines = hist.size();
    const std::string text = histogram_text(hist);
    if (!out_hist.empty()) add_host_file(c, out_hist, text.data(), text.size());
    HIP_TRY(hipStreamSynchronize(c->stream));
}

// N = 4^len of the object's SparseArray (KmerSet.hh:84,72, Graph.cc:120-124) and its file name base
void object_universe(const goss_gpu_ctx* c, uint64_t* nlo, uint64_t* nhi, std::string* base)
{
    const uint32_t bits = c->mode == GOSS_MODE_KMER_SET ? 2 * c->k : 2 * c->k + 2;
    *nlo = bits < 64 ? (1ULL << bits) : 0;
    *nhi = bits >= 64 ? (1ULL << (bits - 64)) : 0;
    *base = c->mode == GOSS_MODE_KMER_SET ? ".kmers" : "-edges";
}
// the object's ".header": {version, k, m} -- a graph's says 0, its arrays know
void add_object_header(goss_gpu_ctx* c, uint64_t m)
{
    const bool set = c->mode == GOSS_MODE_KMER_SET;
    const uint64_t hdr[3] = {set ? kKmerSetVersion : kGraphVersion, c->k, set ? m : 0};
    add_host_file(c, ".header", hdr, sizeof hdr);
}

template <class K>
void emit_object(goss_gpu_ctx* c, const uint64_t* m_estimate)
{
    const K* keys = (const K*)c->build.res_keys;
    const uint64_t m = c->build.M;
    // the SparseArray estimate: the exact distinct count (single-pass build) unless the caller
    // gave one (merges use the sum of the inputs' counts, GossCmdMerge.tcc:256-258,296)
    const uint64_t est = m_estimate ? *m_estimate : m;
    PhaseTimer t(c, GOSS_T_EMIT, m);
    uint64_t nlo, nhi; std::string base;
    object_universe(c, &nlo, &nhi, &base);
    // (the order of the file list: a k-mer set's header behind its array, a graph's ahead of its arrays)
    const bool set = c->mode == GOSS_MODE_KMER_SET;
    if (!set) add_object_header(c, m);
    emit_sparse_array<K>(c, keys, m, nlo, nhi, est, nlo, nhi, base);
    if (set) add_object_header(c, m);
    else emit_counts(c, c->build.res_counts, m, est, "-counts", "-counts-hist.txt");
    t.stop();
}

// Distributed emission, the part a range's owner builds from its own keys (goss_gpu_emit_part).
// prev_high: the high part (key >> D) of the last key of the ranges below this one (0 when there is none) -- what tells a
// range which zeros of the bitmap are its own; have_prev: it was given (else the range builds no blocks of "-d0").
template <class K>
void emit_part(goss_gpu_ctx* c, uint64_t first_index, uint64_t total, uint64_t estimate, uint64_t prev_high = 0, bool have_prev = false)
{
    const K* keys = (const K*)c->build.res_keys;
    const uint64_t m = c->build.M;
    PhaseTimer t(c, GOSS_T_EMIT, m);
    uint64_t nlo, nhi; std::string base;
    object_universe(c, &nlo, &nhi, &base);
    const uint32_t D = (uint32_t)sparse_d(nlo, nhi, estimate);
    const uint64_t nd = sparse_nd(D, nlo, nhi);
    high_bits_check_begin<K>(c, keys, m, D);
    emit_sparse_low_bits<K>(c, keys, m, D, base);
    // This range's SPAN of the high-bits bitmap for the assembling rank: the words its ones fall into (one i of the
    // whole array sits at bit (key_i >> D) + i), built from the range's own keys -- about 2.4 bits per key on the wire
    // where the first form of this path sent key >> D of every key (4 or 8 bytes) -- and, behind it, the DenseSelect blocks
    // that lie wholly inside the range's share of the ones ("-d1") and of the zeros ("-d0": with prev_high).  Records
    // {kind, a, b, body bytes} + body: the span {kPartSpan, first word, words} + the words; blocks {kPartDs, sense (0 ones,
    // 1 zeros), first block} + ds_fill_record's record.
    {
        const uint64_t nwords = (nd + total + 3) / 64 + 1;
        uint64_t w0 = 0, nspan = 0, last_high = prev_high;
        if (m)
        {
            K ends[2];
            HIP_TRY(hipMemcpyAsync(&ends[0], keys, sizeof(K), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(&ends[1], keys + (m - 1), sizeof(K), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const uint64_t h0 = (D >= 128 ? 0 : key_shr64(ends[0], D)) + first_index;
            last_high = D >= 128 ? 0 : key_shr64(ends[1], D);
            const uint64_t h1 = last_high + first_index + (m - 1);
            w0 = h0 >> 6;
            nspan = std::min((h1 >> 6) + 1, nwords) - w0;
        }
        ArenaScope scope(c->arena);
        // whole blocks of ones [first_index, first_index + m) -- the array's last, partial block is the last range's --
        // and of zeros [prev_high, last_high) (the last range: up to the array's nd + 2 zeros)
        // (the LAST NON-EMPTY range owns the tails: an empty range behind it -- first_index == total, m == 0 -- would satisfy
        // first_index + m == total as well and build the same tail blocks a second time; an empty range builds no block,
        // and when every range is empty the assembler builds them all from the bitmap)
        const bool last_range = m > 0 && first_index + m == total;
        const uint64_t count1 = total, count0 = nd + 2;
        DsPlan p1, p0;
        const DsSrc<K> src1{keys, m, D, 0, first_index, nullptr, 0}, src0{keys, m, D, 1, first_index, nullptr, 0};
        if (m)
        {
            const uint64_t b0 = (first_index + 8191) >> 13;
            const uint64_t e = last_range ? (count1 + 8191) >> 13 : (first_index + m) >> 13;
            if (e > b0) p1 = ds_plan<K>(c, src1, count1, b0, e - b0);
        }
        if (have_prev && m)
        {
            const uint64_t z0 = prev_high, z1 = last_range ? count0 : last_high;
            const uint64_t b0 = (z0 + 8191) >> 13;
            const uint64_t e = last_range ? (count0 + 8191) >> 13 : z1 >> 13;
            if (e > b0) p0 = ds_plan<K>(c, src0, count0, b0, e - b0);
        }
        const uint64_t r1 = p1.nb ? 32 + ds_record_bytes(p1) : 0, r0 = p0.nb ? 32 + ds_record_bytes(p0) : 0;
        const uint64_t bytes = 32 + nspan * 8 + r1 + r0;
        uint8_t* blob = (uint8_t*)c->arena.perm(bytes);
        HIP_TRY(hipMemsetAsync(blob, 0, bytes, c->stream));
        const uint64_t hdr[4] = {kPartSpan, w0, nspan, nspan * 8};
        HIP_TRY(hipMemcpyAsync(blob, hdr, 32, hipMemcpyHostToDevice, c->stream));
        if (m)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_high_bits_keys_kernel<K>), dim3(grid_for(m, kEfChunk)), dim3(kTB), 0, c->stream,
                               keys, m, D, first_index, nwords, (unsigned long long*)(blob + 32), w0);
        uint8_t* at = blob + 32 + nspan * 8;
        const uint64_t h1[4] = {kPartDs, 0, p1.b0, ds_record_bytes(p1)}, h0[4] = {kPartDs, 1, p0.b0, ds_record_bytes(p0)};
        if (p1.nb)
        {
            HIP_TRY(hipMemcpyAsync(at, h1, 32, hipMemcpyHostToDevice, c->stream));
            ds_fill_record<K>(c, src1, count1, p1, at + 32);
            at += r1;
        }
        if (p0.nb)
        {
            HIP_TRY(hipMemcpyAsync(at, h0, 32, hipMemcpyHostToDevice, c->stream));
            ds_fill_record<K>(c, src0, count0, p0, at + 32);
            at += r0;
        }
        HIP_TRY(hipStreamSynchronize(c->stream));            // (the headers go out of scope)
        add_dev_file(c, ".part.span", blob, bytes);
    }
    if (c->mode == GOSS_MODE_GRAPH)
    {
        const uint32_t* counts = c->build.res_counts;
        ArenaScope scope(c->arena);
        uint8_t* ord0 = (uint8_t*)c->arena.perm(std::max<uint64_t>(m, 8));
        uint64_t nbig = 0;
        BigCount* big = nullptr;
        std::vector<uint64_t> hist;                      // (count, frequency) pairs, ascending
        if (m)
        {
            uint64_t* slot = (uint64_t*)c->arena.temp((m + 1) * 8);
            nbig = vba_ord0(c, counts, m, ord0, slot);
            big = (BigCount*)c->arena.perm(std::max<uint64_t>(nbig * sizeof(BigCount), 16));
            if (nbig)
                hipLaunchKernelGGL(vba_big_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m, (const uint64_t*)slot,
                                   first_index, big);
            for (auto& kv : count_histogram(c, counts, m, true)) { hist.push_back(kv.first); hist.push_back(kv.second); }
        }
        add_dev_file(c, "-counts.ord0", ord0, m);
        add_dev_file(c, ".part.big", big, nbig * sizeof(BigCount));
        add_host_file(c, ".part.hist", hist.data(), hist.size() * 8);
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    t.stop();
    high_bits_check_end(c);
}

// Distributed emission, the assembling side (goss_gpu_emit_assemble): everything that needs all ranges.
void emit_assemble(goss_gpu_ctx* c, const void* d_spans, uint64_t span_bytes, uint64_t total, uint64_t estimate,
                   const BigCount* big, uint64_t nbig, const uint64_t* hist, uint64_t nhist)
{
    PhaseTimer t(c, GOSS_T_EMIT, total);
    uint64_t nlo, nhi; std::string base;
    object_universe(c, &nlo, &nhi, &base);
    const uint32_t D = (uint32_t)sparse_d(nlo, nhi, estimate);
    const uint64_t nd = sparse_nd(D, nlo, nhi);
    c->stats.ds_blocks_ranges = c->stats.ds_blocks_own = 0;
    // the bitmap: the ranges' spans ORed together (neighbours share their boundary words); the ranges' DenseSelect blocks
    // noted for the composition below
    const uint64_t nwords = (nd + total + 3) / 64 + 1;
    uint64_t* words = (uint64_t*)c->arena.perm(nwords * 8);
    HIP_TRY(hipMemsetAsync(words, 0, nwords * 8, c->stream));
    std::vector<std::pair<uint64_t, const uint8_t*>> ds_recs[2];          // [sense]: {first block, record}
    for (uint64_t at = 0; at + 32 <= span_bytes;)
    {
        uint64_t hdr[4];
        HIP_TRY(hipMemcpyAsync(hdr, (const uint8_t*)d_spans + at, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint8_t* body = (const uint8_t*)d_spans + at + 32;
        if (at + 32 + hdr[3] > span_bytes) throw StatusError{GOSS_ERR_INVALID_ARG, "emit_assemble: a record runs past the parts"};
        if (hdr[0] == kPartSpan)
        {
            if (hdr[1] + hdr[2] > nwords || hdr[3] != hdr[2] * 8) throw StatusError{GOSS_ERR_INVALID_ARG, "emit_assemble: a span does not fit the bitmap"};
            if (hdr[2])
                hipLaunchKernelGGL(ef_or_span_kernel, dim3(grid_for(hdr[2], kTB)), dim3(kTB), 0, c->stream, (unsigned long long*)words + hdr[1],
                                   (const unsigned long long*)body, hdr[2]);
        }
        else if (hdr[0] == kPartDs && hdr[1] < 2) ds_recs[hdr[1]].push_back({hdr[2], body});
        else throw StatusError{GOSS_ERR_INVALID_ARG, "emit_assemble: not a part's record"};
        at += 32 + hdr[3];
    }
    // ones in the words below every word: what finds the positions of the blocks no range could build alone
    ArenaScope scope(c->arena);
    uint64_t* ones = (uint64_t*)c->arena.temp(nwords * 8);
    hipLaunchKernelGGL(ef_word_ones_kernel, dim3(grid_for(nwords, kTB)), dim3(kTB), 0, c->stream, (const unsigned long long*)words, nwords, ones);
    exclusive_scan_u64(c, ones, nwords);
    auto index_files = [&]() {
        add_dev_file(c, base + ".high-bits", words, nwords * 8);
        ds_compose(c, 1, nd + 2, ds_recs[1], (const unsigned long long*)words, nwords, ones, base + "-d0");
        ds_compose(c, 0, total, ds_recs[0], (const unsigned long long*)words, nwords, ones, base + "-d1");
    };
    if (c->mode == GOSS_MODE_KMER_SET)
    {
        emit_sparse_header(c, D, nlo, nhi, total, base);
        index_files();
        add_object_header(c, total);
    }
    else
    {
        add_object_header(c, total);
        emit_sparse_header(c, D, nlo, nhi, total, base);
        index_files();
        // VariableByteArray continuation arrays from the entries with count > 255 (VariableByteArray.hh:76-118):
        // ord1p marks their global positions, ord1 holds bits 8..15; ord2p marks, among those, the ones with
        // count > 65535 by their index in ord1, ord2 holds bits 16..31
        std::vector<uint64_t> pos1(nbig), pos2;
        std::vector<uint8_t> ord1(nbig);
        std::vector<uint16_t> ord2;
        for (uint64_t i = 0; i < nbig; ++i)
        {
            pos1[i] = big[i].index;
            ord1[i] = (uint8_t)((big[i].count >> 8) & 0xFF);
            if (big[i].count >> 16) { pos2.push_back(i); ord2.push_back((uint16_t)(big[i].count >> 16)); }
        }
        const uint64_t mest = (uint64_t)((double)estimate * 0.001);
        Key1* d1 = (Key1*)c->arena.temp(std::max<uint64_t>(nbig, 1) * 8);
        Key1* d2 = (Key1*)c->arena.temp(std::max<uint64_t>(pos2.size(), 1) * 8);
        if (nbig) HIP_TRY(hipMemcpyAsync(d1, pos1.data(), nbig * 8, hipMemcpyHostToDevice, c->stream));
        if (!pos2.empty()) HIP_TRY(hipMemcpyAsync(d2, pos2.data(), pos2.size() * 8, hipMemcpyHostToDevice, c->stream));
        emit_sparse_array<Key1>(c, d1, nbig, estimate, 0, mest, total, 0, "-counts.ord1p");
        add_host_file(c, "-counts.ord1", ord1.data(), ord1.size());
        emit_sparse_array<Key1>(c, d2, pos2.size(), estimate, 0, mest, nbig, 0, "-counts.ord2p");
        add_host_file(c, "-counts.ord2", ord2.data(), ord2.size() * 2);
        // histogram: the ranges' (count, frequency) pairs added up (Graph.cc:131-150 writes them ascending)
        std::map<uint64_t, uint64_t> all;
        for (uint64_t i = 0; i < nhist; ++i) all[hist[2 * i]] += hist[2 * i + 1];
        const std::string text = histogram_text(all);
        add_host_file(c, "-counts-hist.txt", text.data(), text.size());
    }
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
}
