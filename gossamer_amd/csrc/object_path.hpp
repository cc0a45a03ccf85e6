// object_path.hpp -- a KmerSet, Graph, SparseArray or EntryEdgeSet opened for queries (goss_gpu_object_*): the object,
// how its images are planned, checked and brought into its one allocation, and the batched query every entry point
// goes through.  What runs reads against an object is reads_path.hpp.
// Part of goss_gpu.hip, which includes it at file scope behind the context's entry points.

// Device memory that only grows.  room() leaves at least `bytes` (a quarter more when it has to grow, the old block
// freed first: the contents are not kept); the memory goes with the buffer.
namespace {

struct DevBuf {
    uint8_t* p = nullptr;
    uint64_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }

    uint8_t* room(uint64_t bytes)
    {
        if (bytes > cap)
        {
            if (p) { HIP_TRY(hipFree(p)); p = nullptr; cap = 0; }
            const uint64_t want = (bytes + (bytes >> 2) + 4095) & ~4095ULL;
            if (hipMalloc((void**)&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; throw StatusError{GOSS_ERR_OOM, "no device memory for the working arrays of match_reads"}; }
            cap = want;
        }
        return p;
    }
};

}  // namespace

struct goss_gpu_object {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int kind = 0;
    uint32_t K = 0, key_words = 1, node_words = 1;
    bool asymmetric = false;
    uint8_t* mem = nullptr;                 // every image, then the query's failure word
    uint64_t bytes = 0;
    unsigned long long* d_bad = nullptr;    // [0] the failure word, [1] near_kmers' gray total
    unsigned long long* h_bad = nullptr;    // (page-locked, two words)
    QueryObj q{};
    QueryEntries qe{};                      // an EntryEdgeSet's lengths and ends
    std::string last_error;
    // a pass over reads (reads_path.hpp): grow-only working memory, a page-locked block for what comes back, the
    // events that time the kernels
    DevBuf scan_sums;                       // the pass's sums and failure words, the tiles' newline counts and their scan
    DevBuf spare_out;                       // the per-read outputs the caller left out
    DevBuf staged;                          // the _host forms: the batch and its answers on the device
    unsigned long long* h_pass = nullptr;
    hipEvent_t pass_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // goss_gpu_object_classify_bits_host: the kept pair, lhs then rhs, (count + 63) / 64 words each
    uint64_t* classify_bits = nullptr;
    bool classify_kept = false;
    // goss_gpu_object_taxo_*: the tree in one allocation -- parent, last, id by pre-order number, then the sorted ids and
    // their classes, then n + 2 bins --, the annotation (a class per rank), working memory that only grows
    uint32_t taxo_n = 0;
    uint32_t* taxo_tree = nullptr;
    unsigned long long* taxo_bins = nullptr;
    std::vector<uint32_t> taxo_pre;         // the pre-order number of the i-th node as given
    uint32_t* taxo_ann = nullptr;
    bool taxo_ann_kept = false;
    DevBuf taxo_scratch;                    // ids on their way to classes and back
    // goss_gpu_object_colours_host / _from_index: the kept word per rank, how many references it speaks of (new words
    // are filled in an allocation of their own, which replaces this one only once they are complete)
    uint64_t* colours = nullptr;
    uint32_t ncolours = 0;
    bool colours_kept = false;

    // (object_free has set the device and waited for the stream; the buffers above go after this body)
    ~goss_gpu_object()
    {
        if (mem) (void)hipFree(mem);
        if (h_bad) (void)hipHostFree(h_bad);
        if (h_pass) (void)hipHostFree(h_pass);
        if (classify_bits) (void)hipFree(classify_bits);
        if (taxo_tree) (void)hipFree(taxo_tree);
        if (taxo_ann) (void)hipFree(taxo_ann);
        if (colours) (void)hipFree(colours);
        for (hipEvent_t e : pass_ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

thread_local std::string t_open_error;      // why the calling thread's last open failed (goss_gpu_object_last_error(NULL))

struct ObjSrc { const uint8_t* p = nullptr; uint64_t n = 0; bool dev = false; };
typedef std::map<std::string, ObjSrc> ObjFiles;

// The images an object needs, laid out in its one allocation: what is read from where, and which device
// pointer of the object's view points at it.
struct ObjPlan {
    const ObjFiles& files;
    struct Piece { ObjSrc src; uint64_t bytes, off; const void** dst; };
    std::vector<Piece> pieces;
    uint64_t total = 0;

    const ObjSrc& need(const std::string& name) const
    {
        auto it = files.find(name);
        if (it == files.end()) throw StatusError{GOSS_ERR_INVALID_ARG, "missing file " + name};
        if (!it->second.p && it->second.n) throw StatusError{GOSS_ERR_INVALID_ARG, "no data for file " + name};
        return it->second;
    }
    // the first n bytes of a file on the host
    std::vector<uint8_t> head(const ObjSrc& s, uint64_t n) const
    {
        std::vector<uint8_t> v(n);
        if (!n) return v;
        if (s.dev) HIP_TRY(hipMemcpy(v.data(), s.p, n, hipMemcpyDeviceToHost));
        else std::memcpy(v.data(), s.p, n);
        return v;
    }
    void place(const ObjSrc& s, uint64_t bytes, const void** dst)
    {
        pieces.push_back(Piece{s, bytes, total, dst});
        total = (total + bytes + 16 + 255) & ~255ULL;            // (16: the walkers never read past an image; slack only)
    }
};

uint64_t pow4(uint32_t n, uint64_t* hi) { *hi = 2 * n >= 64 ? 1ULL << (2 * n - 64) : 0; return 2 * n < 64 ? 1ULL << (2 * n) : 0; }

// SparseArray(base, fac) (SparseArray.hh:60-72, SparseArray.cc:133-170): header, high-bits, -d0, -d1 and the low-bits
// columns of quantizedD bits (IntegerArray.cc:259-357), every size checked against the header
void plan_sparse(ObjPlan& pl, const std::string& sa, RdSparse& s)
{
    const ObjSrc& hs = pl.need(sa + ".header");
    if (hs.n < sizeof(SaHeader)) throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".header is too short"};
    SaHeader h;
    std::memcpy(&h, pl.head(hs, sizeof h).data(), sizeof h);
    if (h.version != 2012030501ULL) throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".header: SparseArray version mismatch"};
    std::vector<IaCol> cols;
    if (h.D == 0 || h.D > 128 || h.quantizedD != 8 * ((h.D + 7) / 8) || !ia_layout((uint32_t)h.quantizedD, "", 0, cols) || cols.size() > 4)
        throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".header: corrupt SparseArray header"};
    s = RdSparse{};
    s.D = h.D; s.count = h.count; s.size_lo = h.size_lo; s.size_hi = h.size_hi;
    // N >> D bits of zeros and count ones (SparseArray.cc:79-86)
    uint64_t nd = 0;
    if (h.D < 64)
    {
        if (h.size_hi >> h.D) throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".header: N >> D does not fit 64 bits"};
        nd = (h.size_lo >> h.D) | (h.size_hi << (64 - h.D));
    }
    else if (h.D < 128) nd = h.size_hi >> (h.D - 64);
    const ObjSrc& hb = pl.need(sa + ".high-bits");
    const uint64_t words = hb.n / 8;
    if (nd > (~0ULL >> 2) || h.count > (~0ULL >> 2) || words < (nd + h.count + 63) / 64)
        throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".high-bits is shorter than its header says"};
    s.hi.nwords = words;
    pl.place(hb, words * 8, (const void**)&s.hi.w);
    const ObjSrc& d0 = pl.need(sa + "-d0");
    const ObjSrc& d1 = pl.need(sa + "-d1");
    s.d0 = parse_dense_select(pl.head(d0, std::min<uint64_t>(d0.n, sizeof(DsHeader))).data(), d0.n, 1, sa + "-d0");
    s.d1 = parse_dense_select(pl.head(d1, std::min<uint64_t>(d1.n, sizeof(DsHeader))).data(), d1.n, 0, sa + "-d1");
    pl.place(d0, d0.n, (const void**)&s.d0.data);
    pl.place(d1, d1.n, (const void**)&s.d1.data);
    s.ncols = (uint32_t)cols.size();
    for (size_t i = 0; i < cols.size(); ++i)
    {
        const std::string name = sa + ".low-bits" + cols[i].suffix;
        const ObjSrc& c = pl.need(name);
        if (h.count > c.n / cols[i].bytes) throw StatusError{GOSS_ERR_INVALID_ARG, name + " is shorter than its header's count"};
        s.col_bytes[i] = cols[i].bytes; s.col_shift[i] = cols[i].shift;
        pl.place(c, h.count * cols[i].bytes, (const void**)&s.col[i]);
    }
}

// Graph::open / Graph::Graph (Graph.cc:366-410), KmerSet's constructor (KmerSet.hh:170-190), SparseArray(base, fac)
void open_object(goss_gpu_object* o, int kind, const std::string& base, const ObjFiles& files)
{
    ObjPlan pl{files};
    QueryObj& q = o->q;
    o->kind = kind;
    // VariableByteArray(base, fac) (VariableByteArray.hh:120-160) of `items` values
    auto plan_vba = [&](const std::string& vb, RdVba& v, uint64_t items) {
        const ObjSrc& o0 = pl.need(vb + ".ord0");
        if (o0.n < items) throw StatusError{GOSS_ERR_INVALID_ARG, vb + ".ord0 is shorter than the item count"};
        pl.place(o0, items, (const void**)&v.ord0);
        plan_sparse(pl, vb + ".ord1p", v.p1);
        plan_sparse(pl, vb + ".ord2p", v.p2);
        if (v.p1.size_hi || v.p2.size_hi) throw StatusError{GOSS_ERR_INVALID_ARG, vb + ": presence arrays wider than 64 bits"};
        const ObjSrc& o1 = pl.need(vb + ".ord1");
        const ObjSrc& o2 = pl.need(vb + ".ord2");
        if (o1.n < v.p1.count) throw StatusError{GOSS_ERR_INVALID_ARG, vb + ".ord1 is shorter than the ord1p count"};
        if (o2.n / 2 < v.p2.count) throw StatusError{GOSS_ERR_INVALID_ARG, vb + ".ord2 is shorter than the ord2p count"};
        pl.place(o1, v.p1.count, (const void**)&v.ord1);
        pl.place(o2, v.p2.count * 2, (const void**)&v.ord2);
    };
    if (kind == GOSS_OBJECT_SPARSE_ARRAY)
    {
        plan_sparse(pl, base, q.s);
        o->key_words = q.s.size_hi ? 2 : 1;
    }
    else if (kind == GOSS_OBJECT_ENTRY_EDGE_SET)
    {
        // EntryEdgeSet(baseName, fac) (EntryEdgeSet.cc:139-152, 299-306): header, .edges, .counts, .lengths, .ends
        const ObjSrc& hs = pl.need(base + ".header");
        if (hs.n < 16) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header is too short"};
        uint64_t h[2];
        std::memcpy(h, pl.head(hs, 16).data(), 16);
        if (h[0] != 2011041901ULL) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header: EntryEdgeSet version mismatch"};
        if (h[1] == 0 || h[1] > 62u) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header: K out of range"};
        o->K = (uint32_t)h[1];
        q.len = o->K + 1;
        q.graph = 1;                                              // (a count per element: lookup answers it)
        o->key_words = 2 * q.len <= 62 ? 1 : 2;
        o->node_words = 2 * o->K <= 62 ? 1 : 2;
        plan_sparse(pl, base + ".edges", q.s);
        uint64_t nhi, nlo = pow4(q.len, &nhi);
        if (q.s.size_lo != nlo || q.s.size_hi != nhi) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".edges.header: the universe is not 4^len"};
        plan_vba(base + ".counts", q.v, q.s.count);
        plan_vba(base + ".lengths", o->qe.lengths, q.s.count);
        o->qe.count = q.s.count;
        const ObjSrc& up = pl.need(base + ".ends.upr");
        const ObjSrc& lw = pl.need(base + ".ends.lwr");
        if (up.n < q.s.count) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".ends.upr is shorter than the entry count"};
        if (lw.n / 4 < q.s.count) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".ends.lwr is shorter than the entry count"};
        pl.place(up, q.s.count, (const void**)&o->qe.ends_upr);
        pl.place(lw, q.s.count * 4, (const void**)&o->qe.ends_lwr);
    }
    else
    {
        const ObjSrc& hs = pl.need(base + ".header");
        if (hs.n < 24) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header is too short"};
        uint64_t h[3];
        std::memcpy(h, pl.head(hs, 24).data(), 24);
        const bool graph = kind == GOSS_OBJECT_GRAPH;
        if (h[0] != (graph ? kGraphVersion : kKmerSetVersion))
            throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header: " + (graph ? "Graph" : "KmerSet") + " version mismatch"};
        if (h[1] == 0 || h[1] > (graph ? 62u : 63u)) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header: K out of range"};
        o->K = (uint32_t)h[1];
        q.len = graph ? o->K + 1 : o->K;
        q.graph = graph;
        o->key_words = 2 * q.len <= 62 ? 1 : 2;
        o->node_words = 2 * o->K <= 62 ? 1 : 2;
        o->asymmetric = graph && (h[2] & 1);
        const std::string sa = base + (graph ? "-edges" : ".kmers");
        plan_sparse(pl, sa, q.s);
        uint64_t nhi, nlo = pow4(q.len, &nhi);
        if (q.s.size_lo != nlo || q.s.size_hi != nhi) throw StatusError{GOSS_ERR_INVALID_ARG, sa + ".header: the universe is not 4^len"};
        if (!graph && h[2] != q.s.count) throw StatusError{GOSS_ERR_INVALID_ARG, base + ".header: count differs from " + sa};
        if (graph)
        {
            plan_vba(base + "-counts", q.v, q.s.count);
        }
    }
    // one allocation: the images, then the failure word
    const uint64_t bad_off = pl.total;
    o->bytes = pl.total + 256;
    HIP_TRY(hipMalloc((void**)&o->mem, o->bytes));
    o->d_bad = (unsigned long long*)(o->mem + bad_off);
    for (auto& pc : pl.pieces)
    {
        *pc.dst = o->mem + pc.off;
        if (pc.bytes)
            HIP_TRY(hipMemcpyAsync(o->mem + pc.off, pc.src.p, pc.bytes, pc.src.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, o->stream));
    }
    HIP_TRY(hipStreamSynchronize(o->stream));
}

int usable_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return GOSS_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GOSS_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GOSS_ERR_NO_DEVICE;
    return GOSS_OK;
}

// guarded() for objects: no exception crosses the ABI; the message goes to `err`
template <class F>
int obj_guarded(int device, std::string& err, F&& f)
{
    try
    {
        HIP_TRY(hipSetDevice(device));
        (void)hipGetLastError();
        f();
        check_launch("a kernel launch was refused");
        return GOSS_OK;
    }
    catch (const HipError& e) { err = std::string(e.what) + ": " + hipGetErrorString(e.e); return GOSS_ERR_HIP; }
    catch (const StatusError& e) { err = e.msg; return e.status; }
    catch (const std::bad_alloc&) { err = "host allocation failed"; return GOSS_ERR_OOM; }
    catch (const std::exception& e) { err = std::string("unexpected failure: ") + e.what(); return GOSS_ERR_STATE; }
}

void object_free(goss_gpu_object* o)
{
    if (!o) return;
    (void)hipSetDevice(o->device);
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    const hipStream_t owned = o->own_stream ? o->stream : nullptr;
    delete o;                                                    // everything it holds; an owned stream goes last
    if (owned) (void)hipStreamDestroy(owned);
}

int object_open(goss_gpu_object** out, int device, void* stream, int kind, const std::string& base, const ObjFiles& files)
{
    goss_gpu_object* o = new (std::nothrow) goss_gpu_object();
    if (!o) return GOSS_ERR_OOM;
    o->device = device;
    int rc = obj_guarded(device, t_open_error, [&]() {
        if (stream) o->stream = (hipStream_t)stream;
        else { HIP_TRY(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking)); o->own_stream = true; }
        HIP_TRY(hipHostMalloc((void**)&o->h_bad, 16, hipHostMallocDefault));    // (the failure word; near_kmers: the gray total)
        open_object(o, kind, base, files);
    });
    if (rc != GOSS_OK) { object_free(o); return rc; }
    *out = o;
    return GOSS_OK;
}

inline dim3 query_grid(uint64_t n) { return dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 8192)); }

// one batched query: launch, then the lowest failing query index, if any, becomes the call's error
template <class L>
int object_query(goss_gpu_object* o, uint64_t n, L&& launch)
{
    if (n == 0) return GOSS_OK;
    return obj_guarded(o->device, o->last_error, [&]() {
        HIP_TRY(hipMemsetAsync(o->d_bad, 0xFF, 8, o->stream));
        launch(query_grid(n));
        HIP_TRY(hipMemcpyAsync(o->h_bad, o->d_bad, 8, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        const unsigned long long bad = *o->h_bad;
        if (bad != ~0ULL)
        {
            static const char* const why[4] = {"", "a key has bits at or above 2*len (or lies at or past N)",
                                               "a rank is not below the count", "the index walk cannot answer (damaged object)"};
            throw StatusError{GOSS_ERR_INVALID_ARG, "query " + std::to_string(bad >> 2) + ": " + why[bad & 3]};
        }
    });
}

}  // namespace
