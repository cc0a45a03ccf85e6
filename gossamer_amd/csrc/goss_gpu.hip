// goss_gpu.hip -- implementation of the C ABI in include/goss_gpu.h on top of the HIP
// kernels in goss_kernels.hpp.  gfx950 only; no CPU fallback: every entry point that needs
// the device fails with GOSS_ERR_NO_DEVICE / GOSS_ERR_HIP when it is not usable.
#include "../../include/goss_gpu.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "goss_kernels.hpp"
#include "goss_reader.hpp"
#include "goss_read_src.hpp"
#include "goss_knobs.hpp"
#include "goss_arena.hpp"

using namespace goss;

namespace { constexpr uint32_t kAbiVersion = 1; }

// ---- the context: its records, the arena, the phase timer, guarded() ----------------------------------
#include "goss_ctx.hpp"

namespace {

// ---- counting a chunk of keys and merging runs; the fused path; the chunk loop over a push ----------
#include "count_path.hpp"
#include "fused_path.hpp"
#include "chunk_loop.hpp"

// ---- on-disk arrays: the files of an object, of a range's part and of the assembled whole --------
#include "emit_path.hpp"

// ---- prune-tips, print-contigs, build-entry-edge-set: the passes over a finished graph ---------
#include "graph_passes.hpp"

// ---- pool-samples: bit rows, pair counts, the index ---------------------------------------------
#include "pool_path.hpp"

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================
static const char* const kBrokenMsg = "an exchange round of this context's group failed half way: reads staged before it may be lost (goss_gpu_reset starts over)";

extern "C" {

const char* goss_gpu_strerror(int status)
{
    switch (status)
    {
        case GOSS_OK: return "ok";
        case GOSS_ERR_INVALID_ARG: return "invalid argument";
        case GOSS_ERR_NO_DEVICE: return "no usable gfx950 HIP device";
        case GOSS_ERR_OOM: return "out of memory (HBM budget)";
        case GOSS_ERR_HIP: return "HIP runtime error";
        case GOSS_ERR_STATE: return "call out of order";
        case GOSS_ERR_K_RANGE: return "unable to build a graph with that k";
        case GOSS_ERR_COUNT_OVERFLOW: return "a key count does not fit 32 bits";
        case GOSS_ERR_TOO_LARGE: return "SparseArray high bits do not fit 64 bits";
        case GOSS_ERR_BUFFER: return "a buffer of the caller is too small";
        default: return "unknown status";
    }
}

const char* goss_gpu_last_error(const goss_gpu_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

uint32_t goss_gpu_abi_version(void) { return kAbiVersion; }

int goss_gpu_create(goss_gpu_ctx** out, int device, uint32_t k, int mode, uint64_t hbm_budget, void* stream)
{
    if (!out) return GOSS_ERR_INVALID_ARG;
    *out = nullptr;
    if (mode != GOSS_MODE_KMER_SET && mode != GOSS_MODE_GRAPH) return GOSS_ERR_INVALID_ARG;
    if (k == 0) return GOSS_ERR_K_RANGE;
    if (mode == GOSS_MODE_KMER_SET && k > 63) return GOSS_ERR_K_RANGE;   // KmerSet::MaxK
    if (mode == GOSS_MODE_GRAPH && k > 62) return GOSS_ERR_K_RANGE;      // Graph::MaxK
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return GOSS_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GOSS_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GOSS_ERR_NO_DEVICE;
    goss_gpu_ctx* c = new (std::nothrow) goss_gpu_ctx();
    if (!c) return GOSS_ERR_OOM;
    c->device = device; c->k = k; c->mode = mode;
    c->len = mode == GOSS_MODE_GRAPH ? k + 1 : k;
    c->words = (2 * c->len <= 62) ? 1 : 2;
    c->budget = hbm_budget;
    c->knobs = knobs_from_env();
    int rc = guarded(c, [&]() {
        if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
        else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
        HIP_TRY(hipMalloc((void**)&c->d_ctr, sizeof(ExtractCounters)));
        HIP_TRY(hipMalloc((void**)&c->d_flags, 16));
        HIP_TRY(hipMemsetAsync(c->d_flags, 0, 16, c->stream));
        HIP_TRY(hipHostMalloc(&c->h_pinned, 256, hipHostMallocDefault));
    });
    if (rc != GOSS_OK) { goss_gpu_destroy(c); return rc == GOSS_ERR_HIP ? GOSS_ERR_NO_DEVICE : rc; }
    *out = c;
    return GOSS_OK;
}

int goss_gpu_prepare(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->arena.base || c->arena_thread.joinable()) return GOSS_OK;
    c->arena_status = GOSS_OK;
    c->arena_thread = std::thread([c]() {
        try
        {
            HIP_TRY(hipSetDevice(c->device));
            map_arena(c);
        }
        catch (const HipError& e) { c->arena_status = GOSS_ERR_HIP; c->arena_error = std::string(e.what) + ": " + hipGetErrorString(e.e); }
        catch (const StatusError& e) { c->arena_status = e.status; c->arena_error = e.msg; }
    });
    return GOSS_OK;
}

void goss_gpu_destroy(goss_gpu_ctx* c)
{
    if (!c) return;
    if (c->arena_thread.joinable()) c->arena_thread.join();
    (void)hipSetDevice(c->device);
    if (c->bg.joinable()) c->bg.join();
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& pd : c->pending) { if (pd.fn) pd.fn(pd.user); (void)hipEventDestroy(pd.ev); }
    for (auto e : c->pend_pool) (void)hipEventDestroy(e);
    for (auto*& b : c->stage_buf) if (b) (void)hipFree(b);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (auto& pe : c->events) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->arena.base) (void)hipFree(c->arena.base);
    if (c->d_ctr) (void)hipFree(c->d_ctr);
    if (c->d_flags) (void)hipFree(c->d_flags);
    if (c->d_route) (void)hipFree(c->d_route);
    if (c->grp_send) (void)hipFree(c->grp_send);
    if (c->grp_inbox) (void)hipFree(c->grp_inbox);
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Host pushes are gathered in a staging buffer in HBM and counted together: every counted chunk
// becomes a sorted run that has to be merged later, so many small chunks are far more expensive
// than one large one.  Pushes are separated by one non-base byte (windows never span pushes).
// The counting thread's outcome, taken over by the caller's thread (every entry point but the host pushes does this
// first: one thread at a time works on the context's arena and runs).
static void wait_background(goss_gpu_ctx* c);
namespace { void wait_background_thread(goss_gpu_ctx* c) { wait_background(c); } }
static void wait_background(goss_gpu_ctx* c)
{
    if (!c->bg.joinable()) return;
    c->bg.join();
    if (c->bg_status != GOSS_OK)
    {
        const int st = c->bg_status;
        c->bg_status = GOSS_OK;
        throw StatusError{st, c->bg_error};
    }
}

// what a staging buffer holds, as a source: bytes, or -- packed -- its two arrays from position 0
static ReadSrc staged_src(const goss_gpu_ctx* c, const uint8_t* buf, bool packed)
{
    return packed ? ReadSrc::of_packed(pk_codes_of((uint8_t*)buf), pk_bad_of((uint8_t*)buf, c->stage_cap)) : ReadSrc::of_bytes(buf);
}
static void count_staged(goss_gpu_ctx* c, const uint8_t* buf, uint64_t n, bool packed = false)
{
    const auto t1 = std::chrono::steady_clock::now();
    push_source(c, staged_src(c, buf, packed), n);
    c->stats.flush_count_us += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
    c->stats.flushes++;
}

// What is staged is counted now, on the caller's thread (finish, a device push, anything that needs the runs).
static void flush_staging(goss_gpu_ctx* c)
{
    wait_background(c);
    if (!c->stage || c->stage_fill == 0) return;
    const uint64_t n = c->stage_fill;
    c->stage_fill = 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipStreamSynchronize(c->copy_stream));      // (the copies queued so far: counted apart from the chunk's own time)
    c->stats.flush_wait_us += (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    count_staged(c, c->stage, n, c->stage_pk[c->stage_cur]);
}

// A staging buffer is full while the caller keeps pushing: a thread of the library counts it -- its kernels wait on
// the device for the copies that filled it -- and the caller goes on with the other buffer.
static void flush_staging_background(goss_gpu_ctx* c)
{
    if (c->deferred && c->stage && c->stage_fill)
        throw StatusError{GOSS_ERR_BUFFER, "the staging buffer is full and counting is deferred: goss_gpu_group_route_exchange first (goss_gpu_stage_room says how much fits)"};
    wait_background(c);                                  // (one buffer is counted at a time: this is where a producer that outruns the device waits)
    if (!c->stage || c->stage_fill == 0) return;
    const uint64_t n = c->stage_fill;
    uint8_t* buf = c->stage;
    hipEvent_t e;
    if (!c->pend_pool.empty()) { e = c->pend_pool.back(); c->pend_pool.pop_back(); }
    else HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(e, c->copy_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, e, 0));
    c->pend_pool.push_back(e);                           // (the wait has been queued: the event may be recorded again)
    // (the caller's next copies go to the other buffer: the background run below reads this one.  The buffer being
    // switched to is free: wait_background above returned only after the run that read it had synchronised its stream)
    const int cur0 = c->stage_cur;
    const bool packed = c->stage_pk[cur0];
    c->stage_cur ^= 1;
    c->stage = c->stage_buf[c->stage_cur];
    c->stage_fill = 0;
    c->bg_status = GOSS_OK;
    try {
    c->bg = std::thread([c, buf, n, packed]() {
        try
        {
            HIP_TRY(hipSetDevice(c->device));
            (void)hipGetLastError();
            // (the buffer filled up under a caller that goes on pushing: this chunk is one of several)
            Scoped<bool> more(&c->more_follows, true);
            count_staged(c, buf, n, packed);
            check_launch("a kernel launch was refused");
        }
        catch (const HipError& e) { c->bg_status = GOSS_ERR_HIP; c->bg_error = std::string(e.what) + ": " + hipGetErrorString(e.e); }
        catch (const StatusError& e) { c->bg_status = e.status; c->bg_error = e.msg; }
        catch (const std::bad_alloc&) { c->bg_status = GOSS_ERR_OOM; c->bg_error = "host allocation failed"; }
    });
    }
    catch (const std::system_error& e)
    {
        // no thread to be had: nothing was counted and nothing may be lost -- the staged bases are the current buffer's again
        c->stage_cur = cur0;
        c->stage = c->stage_buf[cur0];
        c->stage_fill = n;
        throw StatusError{GOSS_ERR_OOM, std::string("no thread for the counting of a staging buffer: ") + e.what()};
    }
}

int goss_gpu_push_bases_device(goss_gpu_ctx* c, const void* d_bases, uint64_t nbytes)
{
    if (!c || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        flush_staging(c);
        push_source(c, ReadSrc::of_bytes(d_bases), nbytes);
    });
}

// What the caller means to push in all (the `goss` commands know their files' sizes): lets the first chunks of a build
// of many choose the key space they count in for the whole build rather than for themselves.
int goss_gpu_expect_bases(goss_gpu_ctx* c, uint64_t total_bases)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    c->build.expect_bases = total_bases;
    return GOSS_OK;
}

// Packed bases that are already resident in HBM: counted where they lie, like goss_gpu_push_bases_device's bytes.
int goss_gpu_push_packed_device(goss_gpu_ctx* c, const uint32_t* d_codes, const uint16_t* d_nonbase, uint64_t nbases)
{
    if (!c || (nbases && (!d_codes || !d_nonbase))) return GOSS_ERR_INVALID_ARG;
    if (((uintptr_t)d_codes & 3u) || ((uintptr_t)d_nonbase & 1u)) { c->last_error = "packed arrays must be aligned to their elements"; return GOSS_ERR_INVALID_ARG; }
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (c->deferred) { c->last_error = "a deferred context takes host pushes only (its staging buffer is what the group routes)"; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        flush_staging(c);
        push_source(c, ReadSrc::of_packed(d_codes, d_nonbase), nbases);
    });
}

// The byte form of a base string in HBM -> the packed form in the caller's two arrays (ceil(nbytes / 16) elements
// each), on the context's stream; returns when the arrays are written.
int goss_gpu_pack_bases_device(goss_gpu_ctx* c, const void* d_bases, uint64_t nbytes, uint32_t* d_codes, uint16_t* d_nonbase)
{
    if (!c || (nbytes && (!d_bases || !d_codes || !d_nonbase))) return GOSS_ERR_INVALID_ARG;
    if (((uintptr_t)d_codes & 3u) || ((uintptr_t)d_nonbase & 1u)) { c->last_error = "packed arrays must be aligned to their elements"; return GOSS_ERR_INVALID_ARG; }
    return guarded(c, [&]() {
        if (!nbytes) return;
        const uintptr_t addr = (uintptr_t)d_bases;
        const uint32_t mis = (uint32_t)(addr & 15u);
        const uint64_t groups = (nbytes + 15) / 16;
        hipLaunchKernelGGL(pack_bases_kernel, dim3(grid_for(groups, kTB)), dim3(kTB), 0, c->stream, (const uint8_t*)(addr - mis), mis, nbytes,
                           d_codes, d_nonbase, groups);
        check_launch("a kernel launch was refused");
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

// Buffers of asynchronous pushes whose copies have completed go back to the caller (from the caller's own
// thread, inside this call); wait = all of them.
static void release_pending(goss_gpu_ctx* c, bool wait)
{
    size_t done = 0;
    for (; done < c->pending.size(); ++done)
    {
        auto& pd = c->pending[done];
        if (wait) HIP_TRY(hipEventSynchronize(pd.ev));
        else
        {
            const hipError_t e = hipEventQuery(pd.ev);
            if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }          // (the stream is in order: the rest is not ready either)
            if (e != hipSuccess) throw HipError{e, "hipEventQuery(pending push)"};
        }
        if (pd.fn) pd.fn(pd.user);
        c->pend_pool.push_back(pd.ev);
    }
    c->pending.erase(c->pending.begin(), c->pending.begin() + done);
}

static void note_pending(goss_gpu_ctx* c, void (*fn)(void*), void* user)
{
    hipEvent_t e;
    if (!c->pend_pool.empty()) { e = c->pend_pool.back(); c->pend_pool.pop_back(); }
    else HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(e, c->copy_stream));
    c->pending.push_back({e, fn, user});
}

// An asynchronous push registers its buffer and hands back the buffers of earlier pushes whose copies are done.  The
// contract of a failed push (include/goss_gpu.h): the library does NOT call release for it -- the buffer is the
// caller's again on return -- so when handing back fails, the entry just registered is taken out again, after the
// copies queued from the buffer have run (the caller may free it at once).
static void note_pending_checked(goss_gpu_ctx* c, void (*fn)(void*), void* user)
{
    note_pending(c, fn, user);
    try { release_pending(c, false); }
    catch (...)
    {
        (void)hipStreamSynchronize(c->copy_stream);
        if (!c->pending.empty() && c->pending.back().fn == fn && c->pending.back().user == user)
        {
            c->pend_pool.push_back(c->pending.back().ev);
            c->pending.pop_back();
        }
        throw;
    }
}

static void ensure_stage(goss_gpu_ctx* c)
{
    if (c->stage) return;
    wait_background(c);
    ensure_arena(c);
    // 1/24 of the arena each: with ~17 bytes of key workspace per base the staged bases then
    // fill about three quarters of the arena when they are counted
    c->stage_cap = std::max<uint64_t>(c->arena.avail() / 24, 1u << 20) & ~4095ULL;
    {
        // (an arena that was given nearly all of the device leaves less than that beside it: smaller buffers then)
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        // (a deferred context -- a member of a group that exchanges records -- also keeps its routed records and its
        // inbox beside the arena: 0.27 records per staged byte to send and a ninth more to receive, 12 or 20 bytes each --
        // 3.2 + 3.6 staging buffers' worth for one-word keys, 5.3 + 6 for two-word keys; they are allocated at the first
        // exchange and must still find room then)
        const uint64_t units = !c->deferred ? 2u : c->words == 1 ? 9u : 14u;
        const uint64_t room = free_b > (768ULL << 20) ? (free_b - (512ULL << 20)) / units : (128ULL << 20) / units;
        const uint64_t fits = room > (48ULL << 20) ? (room - (32ULL << 20)) : (1ULL << 20);
        if (c->stage_cap > fits) c->stage_cap = std::max<uint64_t>(fits, 1u << 20) & ~4095ULL;
    }
    // (tests: a small staging buffer makes a small input take several flushes / exchange rounds)
    if (const char* e = std::getenv("GOSS_GPU_STAGE_CAP"))
    {
        const uint64_t v = std::strtoull(e, nullptr, 10);
        if (v) c->stage_cap = std::min<uint64_t>(c->stage_cap, std::max<uint64_t>(v, 1u << 16) & ~4095ULL);
    }
    if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    // (one block each: stage_cap bytes, or -- packed -- 6 bytes per sixteen positions of them: codes, then flags)
    const uint64_t bytes = c->stage_cap + 16 + 256 + 64;
    for (auto*& b : c->stage_buf)
        if (!b && hipMalloc((void**)&b, bytes) != hipSuccess) { (void)hipGetLastError(); b = nullptr; throw StatusError{GOSS_ERR_OOM, "no device memory for the staging buffers"}; }
    c->stage_cur = 0;
    c->stage = c->stage_buf[0];
    c->stage_fill = 0;
}

static inline bool is_base_byte(char ch) { const char l = (char)(ch | 0x20); return l == 'a' || l == 'c' || l == 'g' || l == 't'; }

// bases -> staging buffer.  release == nullptr && !async: the copy has completed on return (the caller may
// reuse its buffer); else the buffer comes back through release(user) once its copy has.
static void push_bases_host(goss_gpu_ctx* c, const char* bases, uint64_t nbytes, bool async, void (*release)(void*), void* user)
{
    if (nbytes < c->len) { if (release) release(user); return; }
    ensure_stage(c);
    if (nbytes + 1 > c->stage_cap)
    {
        if (c->deferred) throw StatusError{GOSS_ERR_BUFFER, "a push larger than the staging buffer while counting is deferred"};
        // larger than the staging buffer: count it on its own, in pieces that overlap by
        // len-1 bytes so that no window is lost at a cut
        flush_staging(c);
        uint64_t done = 0;
        const uint64_t nstarts_total = nbytes - c->len + 1;
        while (done < nstarts_total)
        {
            uint64_t ns = std::min<uint64_t>(c->stage_cap - c->len, nstarts_total - done);
            uint64_t nb = ns + c->len - 1;
            c->stage_pk[c->stage_cur] = false;
            HIP_TRY(hipMemcpyAsync(c->stage, bases + done, nb, hipMemcpyHostToDevice, c->copy_stream));
            HIP_TRY(hipStreamSynchronize(c->copy_stream));
            Scoped<uint64_t> more(&c->more_starts, nstarts_total - done - ns);          // (the pieces behind this one: the chunks choose their key space for all of them)
            count_staged(c, c->stage, nb);
            HIP_TRY(hipStreamSynchronize(c->stream));
            done += ns;
        }
        if (release) release(user);
        return;
    }
    // (a buffer holds bytes or packed groups: what is staged in the other form is counted first -- or, when counting is
    // deferred, is the exchange round's to take)
    if (c->stage_fill && c->stage_pk[c->stage_cur])
    {
        if (c->deferred) throw StatusError{GOSS_ERR_BUFFER, "the staging buffer holds packed bases and counting is deferred: goss_gpu_group_route_exchange first"};
        flush_staging_background(c);
    }
    if (c->stage_fill + nbytes + 1 > c->stage_cap) flush_staging_background(c);
    c->stage_pk[c->stage_cur] = false;
    HIP_TRY(hipMemcpyAsync(c->stage + c->stage_fill, bases, nbytes, hipMemcpyHostToDevice, c->copy_stream));
    // reads of two pushes must not join: a separator unless the caller's bytes end with one already
    const bool sep = is_base_byte(bases[nbytes - 1]);
    if (sep) HIP_TRY(hipMemsetAsync(c->stage + c->stage_fill + nbytes, '\n', 1, c->copy_stream));
    c->stage_fill += nbytes + (sep ? 1 : 0);
    if (async) { note_pending_checked(c, release, user); }
    else { HIP_TRY(hipStreamSynchronize(c->copy_stream)); release_pending(c, false); if (release) release(user); }
}

// packed bases -> the staging buffer, as they are: codes to the buffer's code array, flags to its flag array, sixteen
// positions per group (round 5: no landing area, no unpacking kernel -- the kernels that read bases take the groups)
static void push_packed_host(goss_gpu_ctx* c, const uint32_t* codes, const uint16_t* nonbase, uint64_t nbases, bool async,
                             void (*release)(void*), void* user)
{
    if (nbases < c->len) { if (release) release(user); return; }
    ensure_stage(c);
    // The pieces of one push are staged back to back without separators (all but the last are whole groups), so no
    // window is lost where one piece ends.  When the staging buffer must be counted in between, the last len - 1
    // positions are staged again in front of the rest -- their groups from the start, the positions whose windows
    // have been counted flagged as no bases.
    // (the staged string always ends on a group boundary behind a group of separators: the flag array of a buffer is
    // all ones when it starts to fill, and a push sets the flags behind its own last group back to that)
    uint64_t pos = 0, kill = 0;
    bool cont = false;
    if (c->deferred)
    {
        // (goss_gpu.h: a deferred push that does not fit is refused with NOTHING of it taken -- the caller runs the
        // group's exchange round and pushes the same batch again, so a piece staged before the refusal would be
        // counted twice.  The whole push must fit behind what is staged, or the state is not touched.)
        const uint64_t at0 = (c->stage_fill + 15) & ~15ULL;
        const uint64_t need = ((nbases + 15) / 16 + 1) * 16;
        if (at0 + need + 32 > c->stage_cap)
            throw StatusError{GOSS_ERR_BUFFER, c->stage_fill ? "the staging buffer is full and counting is deferred: goss_gpu_group_route_exchange first (goss_gpu_stage_room says how much fits)"
                                                             : "a push larger than the staging buffer while counting is deferred"};
        if (c->stage_fill && !c->stage_pk[c->stage_cur])
            throw StatusError{GOSS_ERR_BUFFER, "the staging buffer holds bytes and counting is deferred: goss_gpu_group_route_exchange first"};
    }
    // (bytes staged by the byte form: counted first -- a buffer holds one form)
    if (c->stage_fill && !c->stage_pk[c->stage_cur]) flush_staging_background(c);
    const uint16_t ones = 0xFFFFu;
    while (pos < nbases)
    {
        if (c->stage_fill == 0)
        {
            // a buffer that starts to fill: packed from here on, every flag set
            c->stage_pk[c->stage_cur] = true;
            HIP_TRY(hipMemsetAsync(pk_bad_of(c->stage, c->stage_cap), 0xFF, pk_groups(c->stage_cap) * 2, c->copy_stream));
        }
        // continuing a push: over the separator group of the piece before (whole groups but for the last piece)
        uint64_t at = cont ? c->stage_fill - 16 : c->stage_fill;
        uint64_t room = at + 64 < c->stage_cap ? (c->stage_cap - 32 - at) & ~15ULL : 0;
        if (room < std::min<uint64_t>((nbases - pos + 15) & ~15ULL, 65536))
        {
            c->stage_fill = at;
            flush_staging_background(c);
            if (cont)
            {
                const uint64_t keep = pos >= c->len - 1 ? pos - (c->len - 1) : 0;      // first position whose window is still to be counted
                const uint64_t from = keep & ~15ULL;
                kill = keep - from;
                pos = from;
            }
            cont = false;
            continue;          // (the other buffer, from its start)
        }
        const uint64_t n = std::min<uint64_t>(nbases - pos, room);
        const uint64_t groups = (n + 15) / 16;
        uint32_t* dcodes = pk_codes_of(c->stage) + at / 16;
        uint16_t* dbad = pk_bad_of(c->stage, c->stage_cap) + at / 16;
        const uint32_t* hc = codes + pos / 16;
        const uint16_t* hb = nonbase + pos / 16;
        HIP_TRY(hipMemcpyAsync(dcodes, hc, groups * 4, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(hipMemcpyAsync(dbad, hb, groups * 2, hipMemcpyHostToDevice, c->copy_stream));
        // positions behind the piece's last in its last group are no bases (the caller's flags need not say so), and the
        // positions of a continued push whose windows were counted with the buffer before are none any more: the two
        // flag words concerned are set once more, corrected -- by a 16-bit memset behind the copies on their stream: the
        // value travels in the command, no host memory has to outlive the call
        if ((n & 15ULL) && (uint16_t)(hb[groups - 1] | (ones << (n & 15ULL))) != hb[groups - 1])
        {
            const uint16_t w = (uint16_t)(hb[groups - 1] | (ones << (n & 15ULL)));
            HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)(dbad + (groups - 1)), w, 1, c->copy_stream));
        }
        if (kill)
        {
            const uint16_t w = (uint16_t)(hb[0] | ((1u << kill) - 1u) | ((groups == 1 && (n & 15ULL)) ? (ones << (n & 15ULL)) : 0u));
            HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)dbad, w, 1, c->copy_stream));
            kill = 0;
        }
        // (the group behind the piece is a group of separators as it stands: a buffer fills from its start, nothing has
        // been written at or behind that group since the flags were set to ones)
        c->stage_fill = at + (groups + 1) * 16;
        pos += n;
        cont = true;
    }
    if (async) { note_pending_checked(c, release, user); }
    else { HIP_TRY(hipStreamSynchronize(c->copy_stream)); release_pending(c, false); if (release) release(user); }
}

int goss_gpu_push_bases_host(goss_gpu_ctx* c, const char* bases, uint64_t nbytes)
{
    if (!c || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    return guarded(c, [&]() { push_bases_host(c, bases, nbytes, false, nullptr, nullptr); }, false);
}

int goss_gpu_push_bases_host_async(goss_gpu_ctx* c, const char* bases, uint64_t nbytes, goss_gpu_release_fn release, void* user)
{
    if (!c || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        // (a failed push hands the buffer back to the caller on return: what was queued from it must have run)
        try { push_bases_host(c, bases, nbytes, true, release, user); }
        catch (...) { if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream); throw; }
    }, false);
}

int goss_gpu_push_packed_host(goss_gpu_ctx* c, const uint32_t* codes, const uint16_t* nonbase, uint64_t nbases)
{
    if (!c || (nbases && (!codes || !nonbase))) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    return guarded(c, [&]() { push_packed_host(c, codes, nonbase, nbases, false, nullptr, nullptr); }, false);
}

int goss_gpu_push_packed_host_async(goss_gpu_ctx* c, const uint32_t* codes, const uint16_t* nonbase, uint64_t nbases,
                                    goss_gpu_release_fn release, void* user)
{
    if (!c || (nbases && (!codes || !nonbase))) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        try { push_packed_host(c, codes, nonbase, nbases, true, release, user); }
        catch (...) { if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream); throw; }
    }, false);
}

int goss_gpu_flush(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    return guarded(c, [&]() { if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream)); release_pending(c, true); }, false);
}

int goss_gpu_finish(goss_gpu_ctx* c, goss_gpu_counts* out)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "finish called twice"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    int rc = guarded(c, [&]() {
        ensure_arena(c);
        flush_staging(c);
        release_pending(c, true);          // (every asynchronous push has been copied by now: the buffers go back)
        const bool unmerged = c->build.runs.size() == 1;          // (a merge resolves its own counts: resolve_big_counts)
        if (c->words == 1) merge_runs<Key1>(c); else merge_runs<Key2>(c);
        if (unmerged && c->build.pushed_counts)
        {
            if (c->words == 1) adopt_literal_counts<Key1>(c, c->build.runs[0]); else adopt_literal_counts<Key2>(c, c->build.runs[0]);
        }
        if (!c->build.runs.empty() && c->build.runs[0].rep)
        {
            if (c->mode == GOSS_MODE_GRAPH)
            {
                // strand pairs -> both strands: the reverse complements as a second run, merged with the first
                if (c->words == 1) { expand_graph_run<Key1>(c, 0); merge_runs<Key1>(c); }
                else { expand_graph_run<Key2>(c, 0); merge_runs<Key2>(c); }
            }
            else
            {
                if (c->words != 1) throw StatusError{GOSS_ERR_STATE, "a two-word run in representative space"};
                canonicalize_run<Key1>(c, c->build.runs[0]);
            }
        }
        if (!c->build.runs.empty()) { c->build.res_keys = c->build.runs[0].keys; c->build.res_counts = c->build.runs[0].counts; c->build.M = c->build.runs[0].m; }
        else { c->build.res_keys = c->arena.perm(16); c->build.res_counts = (uint32_t*)c->arena.perm(16); c->build.M = 0; }
        uint32_t* hf = (uint32_t*)c->h_pinned;
        HIP_TRY(hipMemcpyAsync(hf, c->d_flags, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        // u32 counts saturate at 2^32-1.  A k-mer set does not store counts.  A graph keeps the exact u64 counts
        // of such keys beside the run (resolve_big_counts); its u32 count becomes the value modulo 2^32, which is
        // what the reference stores (Graph::Builder::push_back hands a u64 to VariableByteArray's u32 value_type,
        // Graph.hh:101-106, VariableByteArray.hh:72,81), and its histogram is keyed by the exact count.
        c->build.res_big.clear();
        if (c->mode == GOSS_MODE_GRAPH)
        {
            if (hf[0]) throw StatusError{GOSS_ERR_COUNT_OVERFLOW, "a key occurred 2^32 times or more (unresolved)"};
            if (!c->build.runs.empty() && c->build.runs[0].big >= 0 && !c->build.big_maps[c->build.runs[0].big].empty())
            {
                c->build.res_big = c->build.big_maps[c->build.runs[0].big];
                ArenaScope scope(c->arena);
                const Saturated sat = find_saturated(c, c->build.res_keys, c->build.res_counts, c->build.M);
                const uint32_t nq = (uint32_t)sat.at.size();
                std::vector<uint32_t> vals(nq);
                for (uint32_t q = 0; q < nq; ++q)
                {
                    auto it = c->build.res_big.find(sat.key[q]);
                    if (it == c->build.res_big.end()) throw StatusError{GOSS_ERR_HIP, "count bookkeeping: a saturated result entry without its exact count"};
                    vals[q] = (uint32_t)(it->second & 0xFFFFFFFFULL);
                }
                if (nq)
                {
                    uint32_t* dv = (uint32_t*)c->arena.temp(nq * 4);
                    unsigned long long* dat = (unsigned long long*)c->arena.temp(nq * 8);
                    HIP_TRY(hipMemcpyAsync(dv, vals.data(), nq * 4, hipMemcpyHostToDevice, c->stream));
                    HIP_TRY(hipMemcpyAsync(dat, sat.at.data(), nq * 8, hipMemcpyHostToDevice, c->stream));
                    hipLaunchKernelGGL(patch_counts_kernel, dim3(grid_for(nq, 64)), dim3(64), 0, c->stream, c->build.res_counts,
                                       (const unsigned long long*)dat, (const uint32_t*)dv, nq);
                    HIP_TRY(hipStreamSynchronize(c->stream));
                }
            }
        }
        c->build.finished = true;
    });
    if (rc == GOSS_OK && out)
    {
        out->windows = c->build.windows; out->keys = c->build.keys_total; out->distinct = c->build.M;
        out->key_words = (uint32_t)c->words; out->reserved = 0;
    }
    return rc;
}

int goss_gpu_result(goss_gpu_ctx* c, const void** d_keys, const uint32_t** d_counts, uint64_t* distinct)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished) { c->last_error = "result before finish"; return GOSS_ERR_STATE; }
    if (d_keys) *d_keys = c->build.res_keys;
    if (d_counts) *d_counts = c->build.res_counts;
    if (distinct) *distinct = c->build.M;
    return GOSS_OK;
}

int goss_gpu_result_copy(goss_gpu_ctx* c, uint64_t first, uint64_t n, uint64_t* h_keys, uint32_t* h_counts)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished) { c->last_error = "result before finish"; return GOSS_ERR_STATE; }
    if (first > c->build.M || n > c->build.M - first) return GOSS_ERR_INVALID_ARG;
    return guarded_reading(c, [&]() {
        const uint64_t ksz = c->words * 8;
        if (h_keys && n) HIP_TRY(hipMemcpyAsync(h_keys, (const uint8_t*)c->build.res_keys + first * ksz, n * ksz, hipMemcpyDeviceToHost, c->stream));
        if (h_counts && n) HIP_TRY(hipMemcpyAsync(h_counts, c->build.res_counts + first, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

// goss_gpu_emit and goss_gpu_emit_estimate: m_estimate is the SparseArray estimate the caller gave, or null
static int emit_result(goss_gpu_ctx* c, const uint64_t* m_estimate)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished || c->build.emitted) { c->last_error = "emit needs exactly one finish before it"; return GOSS_ERR_STATE; }
    int rc = guarded(c, [&]() {
        c->build.files.clear();
        {
            // file images: low bits (up to 16 B), bitmap, DenseSelect blocks, counts per element
            const uint64_t need = c->build.M * 40 + (256ULL << 20);
            if (c->arena.avail() < need) grow_arena(c, need);
        }
        if (c->words == 1) emit_object<Key1>(c, m_estimate); else emit_object<Key2>(c, m_estimate);
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
    if (rc == GOSS_OK) c->build.emitted = true;
    return rc;
}

int goss_gpu_emit(goss_gpu_ctx* c) { return emit_result(c, nullptr); }

int goss_gpu_emit_estimate(goss_gpu_ctx* c, uint64_t m_estimate) { return emit_result(c, &m_estimate); }

int goss_gpu_big_counts(goss_gpu_ctx* c, uint64_t* keys, uint64_t* counts, uint32_t cap, uint32_t* n)
{
    if (!c || !n) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished) { c->last_error = "big_counts before finish"; return GOSS_ERR_STATE; }
    *n = (uint32_t)c->build.res_big.size();
    uint32_t i = 0;
    for (auto& kv : c->build.res_big)
    {
        if (i >= cap) break;
        if (keys) { keys[2 * i] = kv.first.second; keys[2 * i + 1] = kv.first.first; }
        if (counts) counts[i] = kv.second;
        ++i;
    }
    return GOSS_OK;
}

static int emit_part_entry(goss_gpu_ctx* c, uint64_t first_index, uint64_t total, uint64_t estimate, uint64_t prev_high, bool have_prev)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished || c->build.emitted) { c->last_error = "emit_part needs exactly one finish before it"; return GOSS_ERR_STATE; }
    if (first_index + c->build.M > total) { c->last_error = "emit_part: the range does not fit the total"; return GOSS_ERR_INVALID_ARG; }
    int rc = guarded(c, [&]() {
        c->build.files.clear();
        {
            const uint64_t need = c->build.M * 48 + (256ULL << 20);
            if (c->arena.avail() < need) grow_arena(c, need);
        }
        const uint64_t est = estimate ? estimate : total;
        if (c->words == 1) emit_part<Key1>(c, first_index, total, est, prev_high, have_prev);
        else emit_part<Key2>(c, first_index, total, est, prev_high, have_prev);
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
    if (rc == GOSS_OK) c->build.emitted = true;
    return rc;
}
int goss_gpu_emit_part(goss_gpu_ctx* c, uint64_t first_index, uint64_t total, uint64_t estimate)
{
    return emit_part_entry(c, first_index, total, estimate, 0, false);
}
int goss_gpu_emit_part_ranges(goss_gpu_ctx* c, uint64_t first_index, uint64_t total, uint64_t estimate, uint64_t prev_last_high)
{
    return emit_part_entry(c, first_index, total, estimate, prev_last_high, true);
}
int goss_gpu_emit_last_high(goss_gpu_ctx* c, uint64_t total, uint64_t estimate, uint64_t* high, int* nonempty)
{
    if (!c || !high || !nonempty) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished) { c->last_error = "emit_last_high needs a finished range"; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        *high = 0; *nonempty = c->build.M ? 1 : 0;
        if (!c->build.M) return;
        uint64_t nlo, nhi; std::string base;
        object_universe(c, &nlo, &nhi, &base);
        const uint32_t D = (uint32_t)sparse_d(nlo, nhi, estimate ? estimate : total);
        if (c->words == 1)
        {
            Key1 k;
            HIP_TRY(hipMemcpyAsync(&k, (const Key1*)c->build.res_keys + (c->build.M - 1), sizeof k, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            *high = D >= 128 ? 0 : key_shr64(k, D);
        }
        else
        {
            Key2 k;
            HIP_TRY(hipMemcpyAsync(&k, (const Key2*)c->build.res_keys + (c->build.M - 1), sizeof k, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            *high = D >= 128 ? 0 : key_shr64(k, D);
        }
    });
}

int goss_gpu_emit_assemble(goss_gpu_ctx* c, const void* d_spans, uint64_t span_bytes, uint64_t total, uint64_t estimate,
                           const void* h_big, uint64_t nbig, const uint64_t* h_hist, uint64_t nhist)
{
    if (!c || (span_bytes & 7u) || (span_bytes && !d_spans) || (total && !span_bytes) || (nbig && !h_big) || (nhist && !h_hist))
        return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished && (!c->build.runs.empty() || c->stage_fill))
    {
        c->last_error = "emit_assemble while a count is in progress";
        return GOSS_ERR_STATE;
    }
    return guarded(c, [&]() {
        ensure_arena(c);
        {
            const uint64_t need = total * 12 + (256ULL << 20);
            if (c->arena.avail() < need) grow_arena(c, need);
        }
        const auto t0 = std::chrono::steady_clock::now();
        emit_assemble(c, d_spans, span_bytes, total, estimate ? estimate : total, (const BigCount*)h_big, nbig, h_hist, nhist);
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->stats.assemble_us = (uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    });
}

// ---- several contexts in one process (one per GPU): the exchange and the emission of gossamer_amd/dist.py
// ---- without a process group -- device-to-device copies instead of collectives ---------------------------

extern "C++" {
namespace {

template <class K>
void group_exchange(goss_gpu_ctx* const* ctxs, uint32_t n, uint32_t sample)
{
    const uint64_t ksz = sizeof(K);
    // 1. splitters: quantiles of a pooled sample of every context's sorted distinct keys
    std::vector<K> pool;
    for (uint32_t i = 0; i < n; ++i)
    {
        goss_gpu_ctx* c = ctxs[i];
        const uint64_t m = c->build.M;
        if (m == 0) continue;
        HIP_TRY(hipSetDevice(c->device));
        const uint64_t take = std::min<uint64_t>(m, sample);
        const uint64_t stride = m / take;
        std::vector<K> h(take);
        HIP_TRY(hipMemcpy2DAsync(h.data(), ksz, (const uint8_t*)c->build.res_keys + (stride / 2) * ksz, stride * ksz, ksz, take,
                                 hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        pool.insert(pool.end(), h.begin(), h.end());
    }
    std::sort(pool.begin(), pool.end(), [](const K& a, const K& b) { return a < b; });
    std::vector<K> split(n > 1 ? n - 1 : 0);
    for (uint32_t p = 1; p < n; ++p)
        split[p - 1] = pool.empty() ? K{} : pool[std::min<uint64_t>(pool.size() - 1, (uint64_t)p * pool.size() / n)];
    // 2. where every context's run is cut
    std::vector<std::vector<uint64_t>> cut(n, std::vector<uint64_t>(n + 1, 0));
    for (uint32_t i = 0; i < n; ++i)
    {
        goss_gpu_ctx* c = ctxs[i];
        cut[i][n] = c->build.M;
        if (n == 1 || c->build.M == 0) { for (uint32_t p = 1; p < n; ++p) cut[i][p] = 0; if (c->build.M == 0) continue; }
        if (n == 1) continue;
        HIP_TRY(hipSetDevice(c->device));
        ArenaScope scope(c->arena);
        K* dq = (K*)c->arena.temp((n - 1) * ksz);
        uint64_t* dout = (uint64_t*)c->arena.temp((n - 1) * 8);
        HIP_TRY(hipMemcpyAsync(dq, split.data(), (n - 1) * ksz, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(lower_bound_keys_kernel<K>), dim3((n - 1 + 63) / 64), dim3(64), 0, c->stream,
                           (const K*)c->build.res_keys, c->build.M, (const K*)dq, n - 1, dout);
        HIP_TRY(hipMemcpyAsync(&cut[i][1], dout, (n - 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // 3. range j of every run -> buffers on context j's device: at the top of context j's own arena where it has the
    //    room (the arenas of a build without --hbm-budget may have grown to nearly all of HBM: device memory outside
    //    them is then scarce), else memory of their own.  The top of an arena is temporary space: it is fenced off
    //    while the context is reset and takes the runs in.
    struct Inbox { uint8_t* keys = nullptr; uint32_t* counts = nullptr; std::vector<uint64_t> off; bool in_arena = false; uint64_t fence = 0; };
    std::vector<Inbox> inbox(n);
    auto free_all = [&]() {
        for (uint32_t j = 0; j < n; ++j)
        {
            if (inbox[j].in_arena) continue;
            (void)hipSetDevice(ctxs[j]->device);
            if (inbox[j].keys) (void)hipFree(inbox[j].keys);
            if (inbox[j].counts) (void)hipFree(inbox[j].counts);
        }
    };
    try
    {
        for (uint32_t j = 0; j < n; ++j)
        {
            goss_gpu_ctx* d = ctxs[j];
            Inbox& in = inbox[j];
            in.off.assign(n + 1, 0);
            for (uint32_t i = 0; i < n; ++i) in.off[i + 1] = in.off[i] + (cut[i][j + 1] - cut[i][j]);
            const uint64_t tot = in.off[n];
            if (tot == 0) continue;
            HIP_TRY(hipSetDevice(d->device));
            // (room for the inbox above the result, and for the runs it becomes plus their merge below it)
            if (d->arena.avail() >= 3 * tot * (ksz + 4) + (512ULL << 20))
            {
                in.counts = (uint32_t*)d->arena.temp(tot * 4);
                in.keys = (uint8_t*)d->arena.temp(tot * ksz);
                in.in_arena = true;
                in.fence = d->arena.hi;
            }
            else
            {
                HIP_TRY(hipMalloc((void**)&in.keys, tot * ksz));
                HIP_TRY(hipMalloc((void**)&in.counts, tot * 4));
            }
            for (uint32_t i = 0; i < n; ++i)
            {
                const uint64_t cnt = cut[i][j + 1] - cut[i][j];
                if (!cnt) continue;
                goss_gpu_ctx* s = ctxs[i];
                HIP_TRY(hipMemcpyPeerAsync(in.keys + in.off[i] * ksz, d->device, (const uint8_t*)s->build.res_keys + cut[i][j] * ksz, s->device,
                                           cnt * ksz, d->stream));
                HIP_TRY(hipMemcpyPeerAsync(in.counts + in.off[i], d->device, s->build.res_counts + cut[i][j], s->device, cnt * 4, d->stream));
            }
        }
        for (uint32_t j = 0; j < n; ++j)
        {
            HIP_TRY(hipSetDevice(ctxs[j]->device));
            HIP_TRY(hipStreamSynchronize(ctxs[j]->stream));
        }
        // 4. every context merges what it received (one host thread per device: the merges run side by side)
        std::vector<int> status(n, GOSS_OK);
        std::vector<std::thread> pool_t;
        for (uint32_t j = 0; j < n; ++j)
            pool_t.emplace_back([&, j]() {
                goss_gpu_ctx* d = ctxs[j];
                const uint64_t windows = d->build.windows, keys_total = d->build.keys_total;
                int rc = goss_gpu_reset(d);
                if (inbox[j].in_arena) d->arena.hi = inbox[j].fence;          // (the reset has given the whole arena back: the inbox lives on)
                for (uint32_t i = 0; i < n && rc == GOSS_OK; ++i)
                {
                    const uint64_t cnt = inbox[j].off[i + 1] - inbox[j].off[i];
                    if (cnt) rc = goss_gpu_push_run_device(d, inbox[j].keys + inbox[j].off[i] * ksz, inbox[j].counts + inbox[j].off[i], cnt);
                }
                if (inbox[j].in_arena) d->arena.hi = d->arena.size;           // (the runs are copies: the inbox is done)
                d->build.windows = windows; d->build.keys_total = keys_total;
                goss_gpu_counts cts;
                if (rc == GOSS_OK) rc = goss_gpu_finish(d, &cts);
                status[j] = rc;
            });
        for (auto& t : pool_t) t.join();
        for (uint32_t j = 0; j < n; ++j)
            if (status[j] != GOSS_OK) throw StatusError{status[j], "merging the received ranges: " + ctxs[j]->last_error};
    }
    catch (...)
    {
        free_all();
        throw;
    }
    free_all();
}

}  // namespace
}  // extern "C++"

int goss_gpu_group_exchange(goss_gpu_ctx* const* ctxs, uint32_t n, uint32_t sample_per_context, uint64_t* range_sizes)
{
    if (!ctxs || n == 0 || n > 64) return GOSS_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) if (!ctxs[i]) return GOSS_ERR_INVALID_ARG;
    goss_gpu_ctx* c0 = ctxs[0];
    for (uint32_t i = 0; i < n; ++i)
    {
        goss_gpu_ctx* c = ctxs[i];
        if (c->k != c0->k || c->mode != c0->mode) { c0->last_error = "group: contexts of different k or mode"; return GOSS_ERR_INVALID_ARG; }
        if (!c->build.finished || c->build.emitted) { c0->last_error = "group exchange needs every context finished and not emitted"; return GOSS_ERR_STATE; }
        for (uint32_t j = 0; j < i; ++j) if (ctxs[j] == c) { c0->last_error = "group: the same context twice"; return GOSS_ERR_INVALID_ARG; }
        if (!c->build.res_big.empty())
        {
            c0->last_error = "group exchange: a multiplicity of 2^32 - 1 or more (exact counts do not travel between contexts)";
            return GOSS_ERR_COUNT_OVERFLOW;
        }
    }
    int rc = guarded(c0, [&]() {
        const uint32_t sample = sample_per_context ? sample_per_context : 1024u;
        if (c0->words == 1) group_exchange<Key1>(ctxs, n, sample); else group_exchange<Key2>(ctxs, n, sample);
    });
    if (rc == GOSS_OK && range_sizes) for (uint32_t i = 0; i < n; ++i) range_sizes[i] = ctxs[i]->build.M;
    return rc;
}

int goss_gpu_group_emit(goss_gpu_ctx* const* ctxs, uint32_t n, uint64_t estimate)
{
    if (!ctxs || n == 0 || n > 64) return GOSS_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) if (!ctxs[i]) return GOSS_ERR_INVALID_ARG;
    goss_gpu_ctx* c0 = ctxs[0];
    for (uint32_t i = 0; i < n; ++i)
        if (ctxs[i]->k != c0->k || ctxs[i]->mode != c0->mode) { c0->last_error = "group: contexts of different k or mode"; return GOSS_ERR_INVALID_ARG; }
    uint64_t total = 0;
    std::vector<uint64_t> first(n);
    for (uint32_t i = 0; i < n; ++i) { first[i] = total; total += ctxs[i]->build.M; }
    // the high part of the last key of the ranges below every range: which zeros of the bitmap a range owns
    std::vector<uint64_t> prev(n, 0);
    {
        uint64_t run = 0;
        for (uint32_t i = 0; i < n; ++i)
        {
            prev[i] = run;
            uint64_t h = 0; int ne = 0;
            const int rc = goss_gpu_emit_last_high(ctxs[i], total, estimate, &h, &ne);
            if (rc != GOSS_OK) { if (i) c0->last_error = ctxs[i]->last_error; return rc; }
            if (ne) run = h;
        }
    }
    // every context's own span and blocks, side by side
    {
        // (a thread that cannot be started -- std::system_error out of std::thread's constructor -- must neither cross the
        // C boundary nor leave joinable threads behind: that member's part is then built on the caller's thread, the parts
        // being independent of one another)
        std::vector<int> status(n, GOSS_OK);
        std::vector<std::thread> pool;
        pool.reserve(n);
        for (uint32_t i = 0; i < n; ++i)
        {
            auto work = [&status, ctxs, &first, total, estimate, &prev, i]() {
                status[i] = goss_gpu_emit_part_ranges(ctxs[i], first[i], total, estimate, prev[i]);
            };
            try { pool.emplace_back(work); }
            catch (const std::system_error&) { work(); }
        }
        for (auto& t : pool) if (t.joinable()) t.join();
        for (uint32_t i = 0; i < n; ++i)
            if (status[i] != GOSS_OK) { if (i) c0->last_error = ctxs[i]->last_error; return status[i]; }
    }
    // the compact parts -> context 0
    uint8_t* d_high = nullptr;
    int rc = guarded(c0, [&]() {
        std::vector<uint8_t> big;
        std::vector<uint64_t> hist;
        std::vector<std::pair<const OutFile*, goss_gpu_ctx*>> highs;
        uint64_t high_total = 0;
        for (uint32_t i = 0; i < n; ++i)
        {
            goss_gpu_ctx* c = ctxs[i];
            HIP_TRY(hipSetDevice(c->device));
            for (const OutFile& f : c->build.files)
            {
                if (f.suffix == ".part.span")
                {
                    highs.push_back({&f, c});
                    high_total += f.size;
                }
                else if (f.suffix == ".part.big" || f.suffix == ".part.hist")
                {
                    std::vector<uint8_t> h(f.size);
                    if (f.size)
                    {
                        if (f.dev)
                        {
                            HIP_TRY(hipMemcpyAsync(h.data(), f.dev, f.size, hipMemcpyDeviceToHost, c->stream));
                            HIP_TRY(hipStreamSynchronize(c->stream));
                        }
                        else std::memcpy(h.data(), f.host.data(), f.size);
                    }
                    if (f.suffix == ".part.big") big.insert(big.end(), h.begin(), h.end());
                    else { const size_t o = hist.size(); hist.resize(o + f.size / 8); if (f.size) std::memcpy(hist.data() + o, h.data(), f.size); }
                }
            }
        }
        if (highs.size() != n) throw StatusError{GOSS_ERR_STATE, "group emit: a context without its span of the bitmap"};
        HIP_TRY(hipSetDevice(c0->device));
        if (high_total)
        {
            HIP_TRY(hipMalloc((void**)&d_high, high_total));
            uint64_t at = 0;
            for (auto& hp : highs)
            {
                if (hp.first->size)
                    HIP_TRY(hipMemcpyPeerAsync(d_high + at, c0->device, hp.first->dev, hp.second->device, hp.first->size, c0->stream));
                at += hp.first->size;
            }
            HIP_TRY(hipStreamSynchronize(c0->stream));
        }
        const int arc = goss_gpu_emit_assemble(c0, d_high, high_total, total, estimate, big.empty() ? nullptr : big.data(),
                                               big.size() / 16, hist.empty() ? nullptr : hist.data(), hist.size() / 2);
        if (arc != GOSS_OK) throw StatusError{arc, c0->last_error};
    });
    if (d_high) { (void)hipSetDevice(c0->device); (void)hipFree(d_high); }
    return rc;
}

// ---- the exchange BEFORE counting for one process that owns several GPUs ---------------------------------
// (gossamer_amd/dist.py: route_and_exchange_records does the same between processes)

extern "C++" {
namespace {

// Bases -> super-k-mer records in nparts parts (goss_gpu_route_records_device; the group's exchange round routes its
// staging buffers through here).  part_records comes back with what every part holds -- or, when a part's room was too
// small (GOSS_ERR_BUFFER), needs.
void route_records(goss_gpu_ctx* c, const ReadSrc& src, uint64_t nbytes, uint32_t nparts, void* d_records, const uint64_t* part_first,
                   const uint64_t* part_cap, uint64_t* part_records, uint64_t* part_windows)
{
    if (c->len > 63) throw StatusError{GOSS_ERR_INVALID_ARG, "records carry windows of at most 63 bases"};
    for (uint32_t p = 0; p < nparts; ++p) { part_records[p] = 0; if (part_windows) part_windows[p] = 0; }
    if (nbytes < c->len) return;
    // counters and the parts' places: a small device block of its own (the arena may not be mapped yet, and need not
    // be), kept for the context's life -- hipFree waits for the whole device, also for a collective of the caller
    // that is still moving the records of the piece before
    const size_t tab = (size_t)kRouteMaxParts * 8;
    if (!c->d_route) HIP_TRY(hipMalloc(&c->d_route, sizeof(RouteCounters) + 2 * tab));
    RouteCounters* rc = (RouteCounters*)c->d_route;
    unsigned long long* dfirst = (unsigned long long*)((uint8_t*)c->d_route + sizeof(RouteCounters));
    unsigned long long* dcap = dfirst + kRouteMaxParts;
    HIP_TRY(hipMemsetAsync(rc, 0, sizeof(RouteCounters), c->stream));
    HIP_TRY(hipMemcpyAsync(dfirst, part_first, nparts * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dcap, part_cap, nparts * 8, hipMemcpyHostToDevice, c->stream));
    const uint64_t nstarts = nbytes - c->len + 1;
    const uint64_t ntiles = (nstarts + kTB * 16 - 1) / (kTB * 16);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, 256 * GOSS_ROUTE_OCC);
    const ReadSrc::Launch in = src.launch();          // (bytes, or a packed staging buffer routed as it is)
    const uint32_t maxwin = 16;          // (the counting side takes records of any length in both modes)
    // slots a workgroup takes ahead per part: ~8 tiles' worth (a tile cuts ~550 records); what it does not use ends as pads
    const uint32_t block = std::max<uint32_t>(32, std::min<uint32_t>(GOSS_ROUTE_BLOCK, 8 * GOSS_ROUTE_BLOCK / nparts));
    {
        PhaseTimer t(c, GOSS_T_EXTRACT, nstarts);
        with_bool(in.kind == ReadSrc::Packed, [&](auto pk) {
            constexpr bool PK = decltype(pk)::value;
            auto route1 = [&](auto w) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(route_records_kernel<decltype(w)::value, PK>), dim3(grid), dim3(kTB), 0, c->stream, in.base, in.mis, nstarts,
                                   nbytes, c->len, maxwin, nparts, block, (SkRec*)d_records, (const unsigned long long*)dfirst,
                                   (const unsigned long long*)dcap, rc, ntiles, in.bad);
            };
            if (c->words == 2)
                // two-word keys: 20-byte records, the minimizer taken over the central 31 / 30 bases of a window (17 positions)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(route_records2_kernel<17, PK>), dim3((uint32_t)std::min<uint64_t>(ntiles, 256 * 4)), dim3(kTB), 0,
                                   c->stream, in.base, in.mis, nstarts, nbytes, c->len, nparts, block, (SkRec2*)d_records,
                                   (const unsigned long long*)dfirst, (const unsigned long long*)dcap, rc, ntiles, in.bad);
            else
                switch (route_positions(c->len))
                {
                    case 17: route1(int_c<17>{}); break;
                    case 13: route1(int_c<13>{}); break;
                    case 9: route1(int_c<9>{}); break;
                    case 5: route1(int_c<5>{}); break;
                    default: route1(int_c<1>{}); break;
                }
        });
        t.stop();
    }
    std::vector<unsigned long long> h(sizeof(RouteCounters) / 8);
    HIP_TRY(hipMemcpyAsync(h.data(), rc, sizeof(RouteCounters), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const RouteCounters* hr = (const RouteCounters*)h.data();
    for (uint32_t p = 0; p < nparts; ++p) { part_records[p] = hr->records[p]; if (part_windows) part_windows[p] = hr->windows[p]; }
#if defined(GOSS_STAMPS)
    if (nparts <= 128 && hr->records[128 + 7])
    {
        const double n = (double)hr->records[128 + 7];
        std::fprintf(stderr, "libgossgpu: routing stamps per tile (ticks of wave 0): A %.0f  B %.0f  barrier %.0f  runs+scan %.0f  C %.0f  room %.0f  D %.0f   (%.0f tiles)\n",
                     hr->records[128] / n, hr->records[129] / n, hr->records[130] / n, hr->records[131] / n, hr->records[132] / n, hr->records[133] / n, hr->records[134] / n, n);
    }
#endif
    if (hr->overflow) throw StatusError{GOSS_ERR_BUFFER, "a part's record buffer is too small (part_records holds what every part needs)"};
}

// RCCL, loaded at run time (the library links against nothing but HIP): point-to-point sends and receives inside one
// group call are an all-to-all at full xGMI bandwidth.  Absent library, communicators that cannot be made (the same
// device twice) or GOSS_GROUP_TRANSPORT=peer -> hipMemcpyPeerAsync.
struct Rccl {
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool tried = false;
    std::map<std::vector<int>, std::vector<void*>> comms;          // device list -> one communicator per member
    std::mutex m;
};
Rccl g_rccl;

bool rccl_load()
{
    if (g_rccl.tried) return g_rccl.lib != nullptr;
    g_rccl.tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
    {
        void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (!h) continue;
        Rccl r;
        r.lib = h;
        r.CommInitAll = (int (*)(void**, int, const int*))dlsym(h, "ncclCommInitAll");
        r.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
        r.GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
        r.GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
        r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclSend");
        r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclRecv");
        r.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
        if (r.CommInitAll && r.GroupStart && r.GroupEnd && r.Send && r.Recv)
        {
            g_rccl.lib = r.lib; g_rccl.CommInitAll = r.CommInitAll; g_rccl.CommDestroy = r.CommDestroy; g_rccl.GroupStart = r.GroupStart;
            g_rccl.GroupEnd = r.GroupEnd; g_rccl.Send = r.Send; g_rccl.Recv = r.Recv; g_rccl.GetErrorString = r.GetErrorString;
            return true;
        }
        dlclose(h);
    }
    return false;
}

// communicators of a device list (made once per list and process); nullptr = not to be had
const std::vector<void*>* rccl_comms(const std::vector<int>& devs)
{
    // (a device twice -- several contexts on one GPU, what a one-GPU box can show -- has no communicators: decided before
    // the library is loaded, which alone takes a second)
    std::vector<int> sorted = devs;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return nullptr;
    std::lock_guard<std::mutex> lk(g_rccl.m);
    if (!rccl_load()) return nullptr;
    auto it = g_rccl.comms.find(devs);
    if (it != g_rccl.comms.end()) return it->second.empty() ? nullptr : &it->second;
    std::vector<void*> cs;
    {
        cs.assign(devs.size(), nullptr);
        if (g_rccl.CommInitAll(cs.data(), (int)devs.size(), devs.data()) != 0) cs.clear();
    }
    auto& slot = g_rccl.comms[devs];
    slot = cs;
    return slot.empty() ? nullptr : &slot;
}

constexpr uint64_t kXferRound = 512ULL << 20;          // bytes per (source, destination) pair and round (RCCL 2.26 drops the second half of segments above 1 GiB)

void group_route_exchange(goss_gpu_ctx* const* ctxs, uint32_t n, int transport, goss_gpu_group_xstats* st)
{
    const uint64_t kRecBytes = rec_bytes(ctxs[0]);          // (all members have one k and mode)
    auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    // 0. the round before: its records are counted by a thread of every member while the caller stages this round's reads
    // (step 3); that counting must have ended before the inboxes are written again -- what is waited for here is the
    // part of it that the staging did not cover
    const auto tw = std::chrono::steady_clock::now();
    double prev_count_ms = 0;
    {
        int bad = GOSS_OK; std::string why;
        for (uint32_t i = 0; i < n; ++i)
        {
            try { HIP_TRY(hipSetDevice(ctxs[i]->device)); wait_background(ctxs[i]); }
            catch (const StatusError& e) { if (bad == GOSS_OK) { bad = e.status; why = "member " + std::to_string(i) + " counting the records of the round before: " + e.msg; } }
            prev_count_ms = std::max(prev_count_ms, ctxs[i]->grp_count_ms);
            ctxs[i]->grp_count_ms = 0;
        }
        if (bad != GOSS_OK) { for (uint32_t i = 0; i < n; ++i) ctxs[i]->build.broken = true; throw StatusError{bad, why}; }
    }
    const double wait_ms = ms_since(tw);
    const auto t0 = std::chrono::steady_clock::now();
    // 1. every member routes what it has staged into n parts (side by side: one host thread per device)
    std::vector<std::vector<uint64_t>> recs(n, std::vector<uint64_t>(n, 0)), wins(n, std::vector<uint64_t>(n, 0)), first(n, std::vector<uint64_t>(n, 0));
    std::vector<int> status(n, GOSS_OK);
    {
        // (a thread that cannot be started must not take the process down with the ones that were: join what runs,
        // then report; and once one member has failed, the others' staged reads are in records nobody will count --
        // the whole group is marked and refuses further work)
        std::vector<std::thread> pool;
        auto join_all = [&]() { for (auto& t : pool) if (t.joinable()) t.join(); };
        auto mark_broken = [&]() { for (uint32_t i = 0; i < n; ++i) ctxs[i]->build.broken = true; };
        auto start = [&](std::function<void()> f) {
            try { pool.emplace_back(std::move(f)); }
            catch (const std::system_error& e) { join_all(); mark_broken(); throw StatusError{GOSS_ERR_OOM, std::string("no thread for a member of the group: ") + e.what()}; }
        };
        for (uint32_t i = 0; i < n; ++i)
            start([&, i]() {
                goss_gpu_ctx* c = ctxs[i];
                status[i] = guarded(c, [&]() {
                    if (!c->stage || c->stage_fill == 0) return;
                    HIP_TRY(hipStreamSynchronize(c->copy_stream));          // (the copies that filled the buffer)
                    const uint64_t nb = c->stage_fill;
                    // room per part: ~7 windows per record, a third of slack; a part that needs more is reported and the
                    // routing is redone with what every part asked for
                    std::vector<uint64_t> cap(n, nb / 5 / n + nb / 15 / n + 4096);
                    for (int attempt = 0;; ++attempt)
                    {
                        uint64_t tot = 0;
                        for (uint32_t p = 0; p < n; ++p) { first[i][p] = tot; tot += cap[p]; }
                        if (tot > c->grp_send_cap)
                        {
                            if (c->grp_send) { HIP_TRY(hipFree(c->grp_send)); c->grp_send = nullptr; c->grp_send_cap = 0; }
                            if (hipMalloc((void**)&c->grp_send, tot * kRecBytes) != hipSuccess)
                            { (void)hipGetLastError(); throw StatusError{GOSS_ERR_OOM, "no device memory for the routed records"}; }
                            c->grp_send_cap = tot;
                        }
                        // (a packed staging buffer is routed as it is)
                        try
                        {
                            route_records(c, staged_src(c, c->stage, c->stage_pk[c->stage_cur]), nb, n, c->grp_send, first[i].data(), cap.data(),
                                          recs[i].data(), wins[i].data());
                            check_launch("a kernel launch was refused");
                            break;
                        }
                        catch (const StatusError& e)
                        {
                            if (e.status != GOSS_ERR_BUFFER || attempt) throw StatusError{e.status, "routing the staged reads: " + e.msg};
                        }
                        catch (const HipError& e)
                        {
                            throw StatusError{GOSS_ERR_HIP, std::string("routing the staged reads: ") + e.what + ": " + hipGetErrorString(e.e)};
                        }
                        catch (const std::bad_alloc&) { throw StatusError{GOSS_ERR_OOM, "routing the staged reads: host allocation failed"}; }
                        for (uint32_t p = 0; p < n; ++p) cap[p] = recs[i][p] + 1;
                    }
                    c->stage_fill = 0;          // (the windows of these bases now live in the records)
                });
            });
        join_all();
        for (uint32_t i = 0; i < n; ++i)
            if (status[i] != GOSS_OK) { mark_broken(); throw StatusError{status[i], "member " + std::to_string(i) + ": " + ctxs[i]->last_error}; }
    }
    const double route_ms = ms_since(t0);
    // 2. part p of every member -> member p's inbox
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<std::vector<uint64_t>> in_off(n, std::vector<uint64_t>(n + 1, 0));          // in_off[p][i]: where member i's records start in p's inbox
    uint64_t total_recs = 0, total_wins = 0;
    for (uint32_t p = 0; p < n; ++p)
    {
        for (uint32_t i = 0; i < n; ++i) { in_off[p][i + 1] = in_off[p][i] + recs[i][p]; total_wins += wins[i][p]; }
        total_recs += in_off[p][n];
        goss_gpu_ctx* d = ctxs[p];
        HIP_TRY(hipSetDevice(d->device));
        if (!d->xstream) HIP_TRY(hipStreamCreateWithFlags(&d->xstream, hipStreamNonBlocking));
        if (in_off[p][n] > d->grp_inbox_cap)
        {
            if (d->grp_inbox) { HIP_TRY(hipFree(d->grp_inbox)); d->grp_inbox = nullptr; d->grp_inbox_cap = 0; }
            const uint64_t want = in_off[p][n] + in_off[p][n] / 8 + 4096;
            if (hipMalloc((void**)&d->grp_inbox, want * kRecBytes) != hipSuccess)
            { (void)hipGetLastError(); throw StatusError{GOSS_ERR_OOM, "no device memory for the received records"}; }
            d->grp_inbox_cap = want;
        }
    }
    std::vector<int> devs(n);
    for (uint32_t i = 0; i < n; ++i) devs[i] = ctxs[i]->device;
    const std::vector<void*>* comms = nullptr;
    if (transport != 2) comms = rccl_comms(devs);
    if (transport == 1 && !comms) throw StatusError{GOSS_ERR_STATE, "RCCL transport asked for, but librccl or its communicators for these devices are not to be had"};
    uint32_t rounds = 0;
    if (comms)
    {
        uint64_t largest = 0;
        for (uint32_t i = 0; i < n; ++i) for (uint32_t p = 0; p < n; ++p) largest = std::max(largest, recs[i][p] * kRecBytes);
        for (uint64_t off = 0; off < std::max<uint64_t>(largest, 1); off += kXferRound, ++rounds)
        {
            if (largest == 0) break;
            auto nccl_check = [&](int rc, const char* what) {
                if (rc != 0) throw StatusError{GOSS_ERR_HIP, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error")};
            };
            nccl_check(g_rccl.GroupStart(), "ncclGroupStart");
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t p = 0; p < n; ++p)
                {
                    const uint64_t bytes = recs[i][p] * kRecBytes;
                    if (off >= bytes) continue;
                    const uint64_t len = std::min<uint64_t>(kXferRound, bytes - off);
                    nccl_check(g_rccl.Send(ctxs[i]->grp_send + first[i][p] * kRecBytes + off, len, 0 /* ncclInt8 */, (int)p, (*comms)[i], ctxs[i]->xstream), "ncclSend");
                    nccl_check(g_rccl.Recv(ctxs[p]->grp_inbox + in_off[p][i] * kRecBytes + off, len, 0, (int)i, (*comms)[p], ctxs[p]->xstream), "ncclRecv");
                }
            nccl_check(g_rccl.GroupEnd(), "ncclGroupEnd");
        }
    }
    else
    {
        for (uint32_t p = 0; p < n; ++p)
        {
            goss_gpu_ctx* d = ctxs[p];
            HIP_TRY(hipSetDevice(d->device));
            for (uint32_t i = 0; i < n; ++i)
                if (recs[i][p])
                {
                    // (one device listed several times -- how the tests run a group on one GPU: a plain device-to-device copy,
                    // the peer call takes a slow path between a device and itself)
                    if (ctxs[i]->device == d->device)
                        HIP_TRY(hipMemcpyAsync(d->grp_inbox + in_off[p][i] * kRecBytes, ctxs[i]->grp_send + first[i][p] * kRecBytes, recs[i][p] * kRecBytes,
                                               hipMemcpyDeviceToDevice, d->xstream));
                    else
                        HIP_TRY(hipMemcpyPeerAsync(d->grp_inbox + in_off[p][i] * kRecBytes, d->device, ctxs[i]->grp_send + first[i][p] * kRecBytes, ctxs[i]->device,
                                                   recs[i][p] * kRecBytes, d->xstream));
                }
        }
        rounds = 1;
    }
    for (uint32_t p = 0; p < n; ++p)
    {
        HIP_TRY(hipSetDevice(ctxs[p]->device));
        HIP_TRY(hipStreamSynchronize(ctxs[p]->xstream));
    }
    const double wire_ms = ms_since(t1);
    // 3. every member counts what it received -- on a thread of its own that this call does NOT wait for (round 5): the
    // members' staging buffers are free again (the windows of their bases live in the records), so the caller stages the
    // next round's reads while the devices count this round's.  The thread is the context's background thread: every
    // entry point that works on the arena or the runs (finish, emit, a device push, the next exchange round) waits for
    // it and takes over its failure; host pushes, which only stage, go on beside it.
    for (uint32_t p = 0; p < n; ++p)
    {
        goss_gpu_ctx* c = ctxs[p];
        const uint64_t nrec = in_off[p][n];
        if (!nrec) continue;
        uint64_t w = 0;
        for (uint32_t i = 0; i < n; ++i) w += wins[i][p];
        auto work = [c, nrec, w]() {
            const auto tc = std::chrono::steady_clock::now();
            try
            {
                HIP_TRY(hipSetDevice(c->device));
                (void)hipGetLastError();
                push_source(c, records_src(c, c->grp_inbox), nrec, w);
                check_launch("a kernel launch was refused");
            }
            catch (const HipError& e) { c->bg_status = GOSS_ERR_HIP; c->bg_error = std::string(e.what) + ": " + hipGetErrorString(e.e); }
            catch (const StatusError& e) { c->bg_status = e.status; c->bg_error = e.msg; }
            catch (const std::bad_alloc&) { c->bg_status = GOSS_ERR_OOM; c->bg_error = "host allocation failed"; }
            c->grp_count_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
        };
        c->bg_status = GOSS_OK;
        try { c->bg = std::thread(work); }
        catch (const std::system_error&) { work(); }          // (no thread to be had: this member's share on the caller's)
    }
    if (st)
    {
        st->transport = comms ? 1u : 2u;
        st->rounds = rounds;
        st->records = total_recs; st->windows = total_wins; st->record_bytes = total_recs * kRecBytes;
        st->route_ms = route_ms; st->wire_ms = wire_ms;
        st->count_ms = prev_count_ms;          // (of the round BEFORE this one: this round's counting has only been started)
        st->count_wait_ms = wait_ms;
    }
}

}  // namespace
}  // extern "C++"

int goss_gpu_set_deferred(goss_gpu_ctx* c, int on)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "deferred counting is set before the pushes"; return GOSS_ERR_STATE; }
    c->deferred = on != 0;
    return GOSS_OK;
}

int goss_gpu_stage_room(goss_gpu_ctx* c, uint64_t* free_bytes, uint64_t* capacity)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    return guarded(c, [&]() {
        ensure_stage(c);
        // (a push of n bytes takes n + 1: the separator behind it)
        if (free_bytes) *free_bytes = c->stage_cap > c->stage_fill + 64 ? c->stage_cap - c->stage_fill - 64 : 0;
        if (capacity) *capacity = c->stage_cap;
    }, false);
}

int goss_gpu_group_route_exchange(goss_gpu_ctx* const* ctxs, uint32_t n, int transport, goss_gpu_group_xstats* out)
{
    if (!ctxs || n == 0 || n > (uint32_t)kRouteMaxParts || transport < 0 || transport > 2) return GOSS_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) if (!ctxs[i]) return GOSS_ERR_INVALID_ARG;
    goss_gpu_ctx* c0 = ctxs[0];
    for (uint32_t i = 0; i < n; ++i)
    {
        goss_gpu_ctx* c = ctxs[i];
        if (c->k != c0->k || c->mode != c0->mode) { c0->last_error = "group: contexts of different k or mode"; return GOSS_ERR_INVALID_ARG; }
        if (c->build.finished) { c0->last_error = "group route exchange after finish"; return GOSS_ERR_STATE; }
        if (c->build.broken) { c0->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
        if (c->len > 63) { c0->last_error = "records carry windows of at most 63 bases"; return GOSS_ERR_INVALID_ARG; }
        for (uint32_t j = 0; j < i; ++j) if (ctxs[j] == c) { c0->last_error = "group: the same context twice"; return GOSS_ERR_INVALID_ARG; }
    }
    if (out) std::memset(out, 0, sizeof(*out));
    if (const char* e = std::getenv("GOSS_GROUP_TRANSPORT"))
    {
        if (!std::strcmp(e, "peer")) transport = 2;
        else if (!std::strcmp(e, "rccl")) transport = 1;
    }
    return guarded(c0, [&]() { group_route_exchange(ctxs, n, transport, out); });
}

int goss_gpu_file_device(goss_gpu_ctx* c, uint32_t i, const void** d_ptr)
{
    if (!c || !d_ptr || i >= c->build.files.size()) return GOSS_ERR_INVALID_ARG;
    *d_ptr = c->build.files[i].dev;          // NULL for a file built on the host
    return GOSS_OK;
}

int goss_gpu_emit_sparse_array(goss_gpu_ctx* c, const void* d_positions, uint32_t key_words, uint64_t n,
                               uint64_t N_lo, uint64_t N_hi, uint64_t M, uint64_t Nend_lo, uint64_t Nend_hi)
{
    if (!c || (key_words != 1 && key_words != 2) || (!d_positions && n)) return GOSS_ERR_INVALID_ARG;
    // its key copy and file images are permanent allocations: between pushes a later merge or an
    // out-of-memory rollback would rewind the permanent end underneath them
    if (!c->build.finished && (!c->build.runs.empty() || c->stage_fill))
    {
        c->last_error = "emit_sparse_array while a count is in progress (reset or finish first)";
        return GOSS_ERR_STATE;
    }
    return guarded(c, [&]() {
        ensure_arena(c);
        c->build.files.clear();
        PhaseTimer t(c, GOSS_T_EMIT, n);
        // private copy so the caller's buffer need not outlive the call
        const uint64_t ksz = key_words * 8;
        void* keys = c->arena.perm(std::max<uint64_t>(n * ksz, 16));
        if (n) HIP_TRY(hipMemcpyAsync(keys, d_positions, n * ksz, hipMemcpyDeviceToDevice, c->stream));
        if (key_words == 1) emit_sparse_array<Key1>(c, (const Key1*)keys, n, N_lo, N_hi, M, Nend_lo, Nend_hi, "");
        else emit_sparse_array<Key2>(c, (const Key2*)keys, n, N_lo, N_hi, M, Nend_lo, Nend_hi, "");
        t.stop();
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_file_count(goss_gpu_ctx* c, uint32_t* n)
{
    if (!c || !n) return GOSS_ERR_INVALID_ARG;
    *n = (uint32_t)c->build.files.size();
    return GOSS_OK;
}

int goss_gpu_file_info(goss_gpu_ctx* c, uint32_t i, char* suffix, size_t cap, uint64_t* size)
{
    if (!c || i >= c->build.files.size()) return GOSS_ERR_INVALID_ARG;
    if (suffix && cap) { std::snprintf(suffix, cap, "%s", c->build.files[i].suffix.c_str()); }
    if (size) *size = c->build.files[i].size;
    return GOSS_OK;
}

int goss_gpu_file_read(goss_gpu_ctx* c, uint32_t i, uint64_t offset, void* dst, uint64_t n)
{
    if (!c || i >= c->build.files.size() || (!dst && n)) return GOSS_ERR_INVALID_ARG;
    const OutFile& f = c->build.files[i];
    if (offset > f.size || n > f.size - offset) return GOSS_ERR_INVALID_ARG;
    if (n == 0) return GOSS_OK;
    if (!f.dev) { std::memcpy(dst, f.host.data() + offset, n); return GOSS_OK; }
    return guarded_reading(c, [&]() {
        HIP_TRY(hipMemcpyAsync(dst, f.dev + offset, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_timing_get(goss_gpu_ctx* c, goss_gpu_timing* out)
{
    if (!c || !out) return GOSS_ERR_INVALID_ARG;
    int rc = guarded_reading(c, [&]() { resolve_timing(c); });
    *out = c->timing;
    return rc;
}

int goss_gpu_timing_reset(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    int rc = guarded_reading(c, [&]() { resolve_timing(c); });
    c->timing = goss_gpu_timing{};
    return rc;
}

int goss_gpu_host_alloc(void** p, size_t bytes)
{
    if (!p || bytes == 0) return GOSS_ERR_INVALID_ARG;
    *p = nullptr;
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    return e == hipSuccess ? GOSS_OK : GOSS_ERR_OOM;
}

void goss_gpu_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int goss_gpu_host_register(void* p, size_t bytes)
{
    if (!p || bytes == 0) return GOSS_ERR_INVALID_ARG;
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? GOSS_OK : GOSS_ERR_OOM;
}

void goss_gpu_host_unregister(void* p)
{
    if (p) { if (hipHostUnregister(p) != hipSuccess) (void)hipGetLastError(); }
}

int goss_gpu_set_path(goss_gpu_ctx* c, int path)
{
    if (!c || path < 0 || path > 1) return GOSS_ERR_INVALID_ARG;
    c->path = path;
    return GOSS_OK;
}

int goss_gpu_reset(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    return guarded(c, [&]() {
        if (c->arena_thread.joinable()) ensure_arena(c);      // a background mapping (goss_gpu_prepare) ends first
        HIP_TRY(hipStreamSynchronize(c->stream));
        release_pending(c, true);
        c->build = Build{};                                   // (the knobs, demoted or not, and the counters stay)
        release_held(c);
        c->arena.lo = 0; c->arena.hi = c->arena.size;
        if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
        c->stage_cur = 0; c->stage = c->stage_buf[0]; c->stage_fill = 0;          // (the staging buffers stay)
        HIP_TRY(hipMemsetAsync(c->d_flags, 0, 16, c->stream));
    });
}

int goss_gpu_push_run_device(goss_gpu_ctx* c, const void* d_keys, const uint32_t* d_counts, uint64_t m)
{
    if (!c || (m && (!d_keys || !d_counts))) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (m == 0) return GOSS_OK;
    return guarded(c, [&]() {
        ensure_arena(c);
        flush_staging(c);
        const uint64_t ksz = c->words * 8;
        if (c->arena.avail() < m * (ksz + 4) + (64u << 20)) grow_arena(c, m * (ksz + 4) + (64u << 20));
        Run r{nullptr, nullptr, m};
        r.keys = c->arena.perm(m * ksz);
        r.counts = (uint32_t*)c->arena.perm(m * 4);
        HIP_TRY(hipMemcpyAsync(r.keys, d_keys, m * ksz, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(r.counts, d_counts, m * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->build.runs.push_back(r);
        c->build.pushed_counts = true;
        // keys_total keeps meaning "keys inserted": a run stands for the sum of its counts,
        // which the caller accounts for; windows are not known here.
    });
}

int goss_gpu_push_run_host(goss_gpu_ctx* c, const uint64_t* keys, const uint32_t* counts, uint64_t m)
{
    if (!c || (m && (!keys || !counts))) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (m == 0) return GOSS_OK;
    return guarded(c, [&]() {
        ensure_arena(c);
        flush_staging(c);
        const uint64_t ksz = c->words * 8;
        if (c->arena.avail() < m * (ksz + 4) + (64u << 20)) grow_arena(c, m * (ksz + 4) + (64u << 20));
        Run r{nullptr, nullptr, m};
        r.keys = c->arena.perm(m * ksz);
        r.counts = (uint32_t*)c->arena.perm(m * 4);
        HIP_TRY(hipMemcpyAsync(r.keys, keys, m * ksz, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(r.counts, counts, m * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->build.runs.push_back(r);
        c->build.pushed_counts = true;
    });
}

extern "C++" {
// Raw keys (unsorted, un-normalised) -> normalise (mode 0) -> count -> one run per piece.
template <class K>
static void push_keys(goss_gpu_ctx* c, const void* keys, uint64_t n, bool on_host)
{
    ensure_arena(c);
    flush_staging(c);
    const uint64_t ksz = sizeof(K);
    uint64_t done = 0;
    while (done < n)
    {
        // two key buffers, the sort's tables and the worst-case run of the piece (chunk_capacity's pessimistic sizing)
        auto capacity = [&]() { return (uint64_t)((double)c->arena.avail() * 0.95 / (2.0 * ksz + 1.2 + (ksz + 12.0))) & ~4095ULL; };
        uint64_t cap = capacity();
        if (cap < 4096 && c->build.runs.size() > 1) { merge_runs<K>(c); cap = capacity(); }
        if (cap < 4096 && grow_arena(c, 0)) cap = capacity();
        if (cap < 4096) throw StatusError{GOSS_ERR_OOM, "HBM budget too small for one piece of keys"};
        const uint64_t m = std::min(cap, n - done);
        {          // (the piece's buffers go before the arena may grow below)
            ArenaScope piece(c->arena);
            K* ka = (K*)c->arena.temp(m * ksz);
            K* kb = (K*)c->arena.temp(m * ksz);
            const K* src = (const K*)keys + done;
            if (on_host)
            {
                HIP_TRY(hipMemcpyAsync(kb, src, m * ksz, hipMemcpyHostToDevice, c->stream));
                src = kb;
            }
            HIP_TRY(hipMemsetAsync(c->d_flags + 2, 0, 4, c->stream));
            {
                PhaseTimer t(c, GOSS_T_EXTRACT, m);
                if (c->mode == GOSS_MODE_GRAPH)
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(normalize_keys_kernel<K, 1>), dim3(grid_for(m, kTB)), dim3(kTB), 0, c->stream, src, ka, m, c->len, c->d_flags);
                else
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(normalize_keys_kernel<K, 0>), dim3(grid_for(m, kTB)), dim3(kTB), 0, c->stream, src, ka, m, c->len, c->d_flags);
                t.stop();
            }
            uint32_t* hf = (uint32_t*)c->h_pinned;
            HIP_TRY(hipMemcpyAsync(hf, c->d_flags + 2, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (hf[0]) throw StatusError{GOSS_ERR_INVALID_ARG, "a pushed key has bits beyond 2*len"};
            c->extract_hist_shift = 0xFFFFFFFFu;          // no extraction kernel histogrammed THESE keys
            Run r = count_keys<K>(c, ka, kb, m);
            c->build.runs.push_back(r);
        }
        // a k-mer is one window and one key; a graph key is one of the two a rho-mer window contributes
        c->build.keys_total += m;
        c->build.windows += c->mode == GOSS_MODE_GRAPH ? m / 2 : m;
        done += m;
        uint64_t run_bytes = 0;
        for (auto& q : c->build.runs) run_bytes += q.m * (ksz + 4);
        if (c->build.runs.size() > 1 && run_bytes > c->arena.size / 4 &&
            (c->arena.avail() >= 2 * run_bytes + (512ULL << 20) || grow_arena(c, 2 * run_bytes + (512ULL << 20)))) merge_runs<K>(c);
    }
}
}

static int push_keys_entry(goss_gpu_ctx* c, const void* keys, uint64_t n, bool on_host)
{
    if (!c || (n && !keys)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (n == 0) return GOSS_OK;
    return guarded(c, [&]() {
        if (c->words == 1) push_keys<Key1>(c, keys, n, on_host); else push_keys<Key2>(c, keys, n, on_host);
    });
}
int goss_gpu_route_records_device(goss_gpu_ctx* c, const void* d_bases, uint64_t nbytes, uint32_t nparts, void* d_records,
                                  const uint64_t* part_first, const uint64_t* part_cap, uint64_t* part_records, uint64_t* part_windows)
{
    if (!c || (!d_bases && nbytes) || nparts == 0 || nparts > (uint32_t)kRouteMaxParts || !part_first || !part_cap || !part_records)
        return GOSS_ERR_INVALID_ARG;
    if (c->len > 63) { c->last_error = "records carry windows of at most 63 bases"; return GOSS_ERR_INVALID_ARG; }
    return guarded(c, [&]() { route_records(c, ReadSrc::of_bytes(d_bases), nbytes, nparts, d_records, part_first, part_cap, part_records, part_windows); });
}

int goss_gpu_push_records_device(goss_gpu_ctx* c, const void* d_records, uint64_t nrecords, uint64_t nwindows)
{
    if (!c || (nrecords && !d_records)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (c->len > 63) { c->last_error = "records carry windows of at most 63 bases"; return GOSS_ERR_INVALID_ARG; }
    return guarded(c, [&]() {
        flush_staging(c);
        push_source(c, records_src(c, d_records), nrecords, nwindows);
    });
}

int goss_gpu_push_keys_device(goss_gpu_ctx* c, const void* d_keys, uint64_t n) { return push_keys_entry(c, d_keys, n, false); }
int goss_gpu_push_keys_host(goss_gpu_ctx* c, const uint64_t* keys, uint64_t n) { return push_keys_entry(c, keys, n, true); }

extern "C++" {
// SparseArray in its on-disk form (host pointers) -> m decoded positions on the device
// (SparseArray::LazyIterator, SparseArray.hh:185-224).  Temporaries above `out` in the arena are the caller's to release.
template <class K>
static void decode_sparse(goss_gpu_ctx* c, const goss_gpu_sparse_run* s, K* out)
{
    const uint64_t m = s->count;
    uint64_t* words = (uint64_t*)c->arena.temp(std::max<uint64_t>(s->high_words, 1) * 8);
    uint64_t* prefix = (uint64_t*)c->arena.temp(std::max<uint64_t>(s->high_words, 1) * 8);
    HIP_TRY(hipMemcpyAsync(words, s->high_bits, s->high_words * 8, hipMemcpyHostToDevice, c->stream));
    EfColumnsIn cols{};
    cols.n = s->ncols;
    for (uint32_t i = 0; i < s->ncols; ++i)
    {
        uint8_t* d = (uint8_t*)c->arena.temp(m * s->col_bytes[i] + 16);
        HIP_TRY(hipMemcpyAsync(d, s->col[i], m * s->col_bytes[i], hipMemcpyHostToDevice, c->stream));
        cols.src[i] = d; cols.bytes[i] = s->col_bytes[i]; cols.shift[i] = s->col_shift[i];
    }
    hipLaunchKernelGGL(popc_words_kernel, dim3(grid_for(s->high_words, 256)), dim3(256), 0, c->stream,
                       (const uint64_t*)words, s->high_words, prefix);
    exclusive_scan_u64(c, prefix, s->high_words);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ef_decode_kernel<K>), dim3(grid_for(s->high_words, 256)), dim3(256), 0, c->stream,
                       (const uint64_t*)words, s->high_words, (const uint64_t*)prefix, (uint32_t)s->D, cols, m, out);
}
static bool sparse_run_ok(const goss_gpu_sparse_run* s) { return s && s->ncols >= 1 && s->ncols <= 4 && (!s->count || s->high_bits); }
static uint64_t sparse_run_need(const goss_gpu_sparse_run* s)
{
    uint64_t need = s->high_words * 16 + 4096;
    for (uint32_t i = 0; i < s->ncols; ++i) need += s->count * s->col_bytes[i] + 256;
    return need;
}
}  // extern "C++"

int goss_gpu_push_run_sparse(goss_gpu_ctx* c, const goss_gpu_sparse_run* s)
{
    if (!c || !sparse_run_ok(s)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    if (s->count == 0) return GOSS_OK;
    return guarded(c, [&]() {
        ensure_arena(c);
        flush_staging(c);
        const uint64_t m = s->count, ksz = c->words * 8;
        {
            const uint64_t need = m * (ksz + 4) + sparse_run_need(s) + (64u << 20);
            if (c->arena.avail() < need) grow_arena(c, need);
        }
        Run r{nullptr, nullptr, m};
        r.keys = c->arena.perm(m * ksz);
        r.counts = (uint32_t*)c->arena.perm(m * 4);
        ArenaScope scope(c->arena);
        if (c->words == 1) decode_sparse<Key1>(c, s, (Key1*)r.keys); else decode_sparse<Key2>(c, s, (Key2*)r.keys);
        if (s->counts) HIP_TRY(hipMemcpyAsync(r.counts, s->counts, m * 4, hipMemcpyHostToDevice, c->stream));
        else hipLaunchKernelGGL(fill_u32_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, r.counts, m, s->weight ? s->weight : 1u);
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->build.runs.push_back(r);
        c->build.pushed_counts = true;
    });
}

int goss_gpu_push_run_graph(goss_gpu_ctx* c, const goss_gpu_sparse_run* edges, const goss_gpu_vba* v)
{
    if (!c || !sparse_run_ok(edges) || !v || !sparse_run_ok(&v->ord1p) || !sparse_run_ok(&v->ord2p)) return GOSS_ERR_INVALID_ARG;
    if (c->build.finished) { c->last_error = "push after finish"; return GOSS_ERR_STATE; }
    if (c->build.broken) { c->last_error = kBrokenMsg; return GOSS_ERR_STATE; }
    const uint64_t m = edges->count, n1 = v->ord1p.count, n2 = v->ord2p.count;
    if (m == 0) return GOSS_OK;
    if (v->ord0_bytes < m || v->ord1_bytes < n1 || v->ord2_bytes < 2 * n2 || (m && !v->ord0) || (n1 && !v->ord1) || (n2 && !v->ord2))
    {
        c->last_error = "VariableByteArray files shorter than their presence arrays say";
        return GOSS_ERR_INVALID_ARG;
    }
    return guarded(c, [&]() {
        ensure_arena(c);
        flush_staging(c);
        const uint64_t ksz = c->words * 8;
        {
            const uint64_t need = m * (ksz + 5) + sparse_run_need(edges) + sparse_run_need(&v->ord1p) + sparse_run_need(&v->ord2p)
                                  + n1 * 9 + n2 * 10 + (64u << 20);
            if (c->arena.avail() < need) grow_arena(c, need);
        }
        Run r{nullptr, nullptr, m};
        r.keys = c->arena.perm(m * ksz);
        r.counts = (uint32_t*)c->arena.perm(m * 4);
        ArenaScope scope(c->arena);
        if (c->words == 1) decode_sparse<Key1>(c, edges, (Key1*)r.keys); else decode_sparse<Key2>(c, edges, (Key2*)r.keys);
        // the multiplicities: VariableByteArray read on the device
        uint8_t* d0 = (uint8_t*)c->arena.temp(m + 16);
        HIP_TRY(hipMemcpyAsync(d0, v->ord0, m, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(vba_read0_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, (const uint8_t*)d0, m, r.counts);
        if (n1)
        {
            Key1* p1 = (Key1*)c->arena.temp(n1 * 8);
            uint8_t* d1 = (uint8_t*)c->arena.temp(n1 + 16);
            decode_sparse<Key1>(c, &v->ord1p, p1);
            HIP_TRY(hipMemcpyAsync(d1, v->ord1, n1, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(vba_read1_kernel, dim3(grid_for(n1, 256)), dim3(256), 0, c->stream, (const Key1*)p1, (const uint8_t*)d1, n1, m, r.counts);
            if (n2)
            {
                Key1* p2 = (Key1*)c->arena.temp(n2 * 8);
                uint16_t* d2 = (uint16_t*)c->arena.temp(n2 * 2 + 16);
                decode_sparse<Key1>(c, &v->ord2p, p2);
                HIP_TRY(hipMemcpyAsync(d2, v->ord2, n2 * 2, hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(vba_read2_kernel, dim3(grid_for(n2, 256)), dim3(256), 0, c->stream, (const Key1*)p2, (const uint16_t*)d2, n2,
                                   (const Key1*)p1, n1, m, r.counts);
            }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->build.runs.push_back(r);
        c->build.pushed_counts = true;
    });
}

extern "C++" {
template <class K>
static void select_counts(goss_gpu_ctx* c, uint32_t lo, uint32_t hi)
{
    const uint64_t n = c->build.M;
    if (n == 0) return;
    ArenaScope scope(c->arena);
    const uint64_t ntiles = (n + kRedTile - 1) / kRedTile;
    uint64_t* tile_counts = (uint64_t*)c->arena.temp((ntiles + 1) * 8);
    hipLaunchKernelGGL(select_count_kernel, dim3(grid_for(n, kRedTile)), dim3(kTB), 0, c->stream,
                       (const uint32_t*)c->build.res_counts, n, lo, hi, tile_counts);
    const uint64_t m = scan_total(c, tile_counts, ntiles);
    K* keys = (K*)c->arena.perm(std::max<uint64_t>(m * sizeof(K), 16));
    uint32_t* counts = (uint32_t*)c->arena.perm(std::max<uint64_t>(m * 4, 16));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(select_write_kernel<K>), dim3(grid_for(n, kRedTile)), dim3(kTB), 0, c->stream,
                       (const K*)c->build.res_keys, (const uint32_t*)c->build.res_counts, n, lo, hi, (const uint64_t*)tile_counts, keys, counts);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->build.res_keys = keys; c->build.res_counts = counts; c->build.M = m;
}
}  // extern "C++"

int goss_gpu_select_counts(goss_gpu_ctx* c, uint32_t lo, uint32_t hi)
{
    if (!c || lo > hi) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished || c->build.emitted) { c->last_error = "select_counts belongs between finish and emit"; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        if (c->words == 1) select_counts<Key1>(c, lo, hi); else select_counts<Key2>(c, lo, hi);
        t.stop();
    });
}

int goss_gpu_select_normal(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished || c->build.emitted) { c->last_error = "select_normal belongs between finish and emit"; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        if (c->build.M)
        {
            const dim3 grid = unit_grid((c->build.M + kTB - 1) / kTB);
            if (c->words == 1)
            {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(mark_normal_kernel<Key1>), grid, dim3(kTB), 0, c->stream,
                                   (const Key1*)c->build.res_keys, c->build.M, c->len, c->build.res_counts);
                select_counts<Key1>(c, 1, 1);
            }
            else
            {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(mark_normal_kernel<Key2>), grid, dim3(kTB), 0, c->stream,
                                   (const Key2*)c->build.res_keys, c->build.M, c->len, c->build.res_counts);
                select_counts<Key2>(c, 1, 1);
            }
        }
        t.stop();
    });
}

// DenseSelect::DenseSelect (DenseArray.cc:36-91): the header's checks against the size of its file (`head`: at
// least the header's bytes of it on the host); the device view without its data pointer
static RdDenseSelect parse_dense_select(const void* head, uint64_t size, int invert, const std::string& name = "DenseSelect file")
{
    if (!head || size < sizeof(DsHeader)) throw StatusError{GOSS_ERR_INVALID_ARG, name + " too short"};
    DsHeader h;
    std::memcpy(&h, head, sizeof h);
    if (h.version != 2012092701ULL) throw StatusError{GOSS_ERR_INVALID_ARG, name + ": DenseSelect version mismatch"};
    if (h.logBlockSize > 40 || h.logSampleRate > h.logBlockSize || (1ULL << h.logBlockSize) != h.blockSize ||
        (1ULL << h.logSampleRate) != h.sampleRate || h.smallBlocks + h.intermediateBlocks + h.largeBlocks != h.numBlocks)
        throw StatusError{GOSS_ERR_INVALID_ARG, name + ": Corrupt DenseSelect index header"};
    if ((int)(h.flags & 1) != invert) throw StatusError{GOSS_ERR_INVALID_ARG, name + ": DenseSelect index does not have the expected sense"};
    if (h.indexArrayOffset > size || h.numBlocks > (size - h.indexArrayOffset) / 8 ||
        h.rankArrayOffset > size || h.numBlocks > (size - h.rankArrayOffset) / 8)
        throw StatusError{GOSS_ERR_INVALID_ARG, name + ": DenseSelect arrays lie outside the file"};
    RdDenseSelect r{};
    r.size = size; r.flags = h.flags; r.indexArrayOffset = h.indexArrayOffset; r.rankArrayOffset = h.rankArrayOffset;
    r.logBlockSize = h.logBlockSize; r.blockSize = h.blockSize; r.logSampleRate = h.logSampleRate; r.sampleRate = h.sampleRate;
    r.numBlocks = h.numBlocks;
    return r;
}

// ... then the device view of the file, copied into the context's arena
static RdDenseSelect open_dense_select(goss_gpu_ctx* c, const void* host, uint64_t size, int invert)
{
    RdDenseSelect r = parse_dense_select(host, size, invert);
    uint8_t* d = (uint8_t*)c->arena.temp(size + 16);
    HIP_TRY(hipMemcpyAsync(d, host, size, hipMemcpyHostToDevice, c->stream));
    r.data = d;
    return r;
}

int goss_gpu_check_index(goss_gpu_ctx* c, const goss_gpu_sparse_files* f, goss_gpu_index_report* out)
{
    if (!c || !f || !out || f->ncols == 0 || f->ncols > 4) return GOSS_ERR_INVALID_ARG;
    static_assert(sizeof(goss_gpu_index_report) == sizeof(IndexReport), "index report layout");
    if (!c->build.finished) { c->last_error = "check_index before finish"; return GOSS_ERR_STATE; }
    std::memset(out, 0, sizeof *out);
    if (c->build.M != f->count) { c->last_error = "the object's count differs from the number of decoded elements"; return GOSS_ERR_STATE; }
    if (c->build.M == 0) return GOSS_OK;
    return guarded(c, [&]() {
        ArenaScope scope(c->arena);
        RdSparse s{};
        s.D = f->D; s.count = f->count; s.size_lo = f->size_lo; s.size_hi = f->size_hi;
        uint64_t* hw = (uint64_t*)c->arena.temp(f->high_words * 8 + 16);
        HIP_TRY(hipMemcpyAsync(hw, f->high_bits, f->high_words * 8, hipMemcpyHostToDevice, c->stream));
        s.hi.w = hw; s.hi.nwords = f->high_words;
        s.d0 = open_dense_select(c, f->d0, f->d0_bytes, 1);
        s.d1 = open_dense_select(c, f->d1, f->d1_bytes, 0);
        s.ncols = f->ncols;
        for (uint32_t i = 0; i < f->ncols; ++i)
        {
            uint8_t* d = (uint8_t*)c->arena.temp(f->count * f->col_bytes[i] + 16);
            HIP_TRY(hipMemcpyAsync(d, f->col[i], f->count * f->col_bytes[i], hipMemcpyHostToDevice, c->stream));
            s.col[i] = d; s.col_bytes[i] = f->col_bytes[i]; s.col_shift[i] = f->col_shift[i];
        }
        IndexReport* rep = (IndexReport*)c->arena.temp(sizeof(IndexReport));
        HIP_TRY(hipMemsetAsync(rep, 0, sizeof(IndexReport), c->stream));
        if (c->words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(check_index_kernel<Key1>), dim3(grid_for(c->build.M, 256)), dim3(256), 0, c->stream, s,
                               (const Key1*)c->build.res_keys, c->build.M, rep);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(check_index_kernel<Key2>), dim3(grid_for(c->build.M, 256)), dim3(256), 0, c->stream, s,
                               (const Key2*)c->build.res_keys, c->build.M, rep);
        HIP_TRY(hipMemcpyAsync(out, rep, sizeof(IndexReport), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (out->nexamples > 16) out->nexamples = 16;
    });
}

int goss_gpu_set_budget_limit(goss_gpu_ctx* c, uint64_t max_bytes)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    c->budget_limit = max_bytes;
    return GOSS_OK;
}

int goss_gpu_stat(goss_gpu_ctx* c, const char* name, uint64_t* value)
{
    if (!c || !name || !value) return GOSS_ERR_INVALID_ARG;
    if (std::strcmp(name, "runs") == 0) *value = c->build.runs.size();
    else if (std::strcmp(name, "arena_bytes") == 0) *value = c->arena.size;
    else if (!stat_lookup(c->stats, name, value)) return GOSS_ERR_INVALID_ARG;
    return GOSS_OK;
}

int goss_gpu_emit_dump_range(goss_gpu_ctx* c, uint64_t flags, uint64_t first, uint64_t count)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (!c->build.finished) { c->last_error = "dump before finish"; return GOSS_ERR_STATE; }
    if (first > c->build.M || count > c->build.M - first) return GOSS_ERR_INVALID_ARG;
    return guarded(c, [&]() {
        c->build.files.clear();
        // the previous piece's text is dead: give its room back (nothing else was allocated since)
        if (c->build.dump_live) { c->arena.lo = c->dump_lo; c->build.dump_live = false; }
        PhaseTimer t(c, GOSS_T_EMIT, count);
        const uint64_t m = count;
        const uint32_t len = c->len;
        // "#<version>\nK\tcount\n" (GossCmdDumpKmerSet.cc:44-45) / "#<version>\nK\tcount\tflags\n"
        // (GossCmdDumpGraph.cc:50-51): in front of the first piece only
        char head[128];
        int hl = 0;
        if (first == 0)
            hl = c->mode == GOSS_MODE_KMER_SET
                     ? std::snprintf(head, sizeof head, "#%llu\n%u\t%llu\n", (unsigned long long)kKmerSetVersion, c->k, (unsigned long long)c->build.M)
                     : std::snprintf(head, sizeof head, "#%llu\n%u\t%llu\t%llu\n", (unsigned long long)kGraphVersion, c->k, (unsigned long long)c->build.M,
                                     (unsigned long long)flags);
        const uint64_t ksz = c->words * 8;
        const uint8_t* keys = (const uint8_t*)c->build.res_keys + first * ksz;
        const uint32_t* counts = c->build.res_counts + first;
        uint64_t body = 0;
        ArenaScope scope(c->arena);
        uint64_t* offs = nullptr;
        if (c->mode == GOSS_MODE_KMER_SET) body = m * (len + 1ULL);
        else if (m)
        {
            offs = (uint64_t*)c->arena.temp((m + 1) * 8);
            hipLaunchKernelGGL(dump_line_len_kernel, dim3(grid_for(m, 256)), dim3(256), 0, c->stream, counts, m, len, offs);
            body = scan_total(c, offs, m);
        }
        c->dump_lo = c->arena.lo;
        uint8_t* text = (uint8_t*)c->arena.perm(hl + body + 16);
        c->build.dump_live = true;
        if (hl) HIP_TRY(hipMemcpyAsync(text, head, hl, hipMemcpyHostToDevice, c->stream));
        if (m)
        {
            if (c->mode == GOSS_MODE_KMER_SET)
            {
                const uint32_t grid = (uint32_t)std::min<uint64_t>(grid_for(body, 256), 256 * 64);
                if (c->words == 1)
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(dump_kmers_kernel<Key1>), dim3(grid), dim3(256), 0, c->stream,
                                       (const Key1*)keys, m, len, text + hl);
                else
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(dump_kmers_kernel<Key2>), dim3(grid), dim3(256), 0, c->stream,
                                       (const Key2*)keys, m, len, text + hl);
            }
            else if (c->words == 1)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(dump_edges_kernel<Key1>), dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                                   (const Key1*)keys, counts, (const uint64_t*)offs, m, len, text + hl);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(dump_edges_kernel<Key2>), dim3(grid_for(m, 256)), dim3(256), 0, c->stream,
                                   (const Key2*)keys, counts, (const uint64_t*)offs, m, len, text + hl);
        }
        t.stop();
        HIP_TRY(hipStreamSynchronize(c->stream));
        add_dev_file(c, ".dump", text, hl + body);
    });
}

int goss_gpu_emit_dump(goss_gpu_ctx* c, uint64_t flags)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    return goss_gpu_emit_dump_range(c, flags, 0, c->build.M);
}

int goss_gpu_lint(goss_gpu_ctx* c, int asymmetric, goss_gpu_lint_report* out)
{
    if (!c || !out) return GOSS_ERR_INVALID_ARG;
    static_assert(sizeof(goss_gpu_lint_report) == sizeof(LintReport), "lint report layout");
    if (!c->build.finished) { c->last_error = "lint before finish"; return GOSS_ERR_STATE; }
    if (c->mode != GOSS_MODE_GRAPH) { c->last_error = "lint checks a graph"; return GOSS_ERR_STATE; }
    std::memset(out, 0, sizeof *out);
    if (c->build.M == 0) return GOSS_OK;
    return guarded_reading(c, [&]() {
        ArenaScope scope(c->arena);
        LintReport* rep = (LintReport*)c->arena.temp(sizeof(LintReport));
        HIP_TRY(hipMemsetAsync(rep, 0, sizeof(LintReport), c->stream));
        if (c->words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(lint_edges_kernel<Key1>), dim3(grid_for(c->build.M, 256)), dim3(256), 0, c->stream,
                               (const Key1*)c->build.res_keys, (const uint32_t*)c->build.res_counts, c->build.M, c->len, asymmetric, rep);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(lint_edges_kernel<Key2>), dim3(grid_for(c->build.M, 256)), dim3(256), 0, c->stream,
                               (const Key2*)c->build.res_keys, (const uint32_t*)c->build.res_counts, c->build.M, c->len, asymmetric, rep);
        HIP_TRY(hipMemcpyAsync(out, rep, sizeof(LintReport), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (out->nexamples > 32) out->nexamples = 32;
    });
}

int goss_gpu_prune_tips(goss_gpu_ctx* c, uint32_t iterations, goss_gpu_tips_report* reports)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    const int st = graph_pass_state(c, "prune_tips", "prune_tips works on a graph", "prune_tips belongs between finish and emit");
    if (st != GOSS_ERR_STATE && reports && iterations) std::memset(reports, 0, sizeof(goss_gpu_tips_report) * (size_t)iterations);
    if (st != GOSS_OK) return st;
    return guarded(c, [&]() { prune_tips(c, iterations, reports); });
}

int goss_gpu_trim_paths(goss_gpu_ctx* c, uint32_t flags, uint32_t cutoff, goss_gpu_paths_report* out)
{
    if (!c || !out || (flags & ~(uint32_t)GOSS_PATHS_CUTOFF)) return GOSS_ERR_INVALID_ARG;
    return paths_entry(c, out, "trim_paths", "trim_paths works on a graph", "trim_paths belongs between finish and emit", [&]() {
        if (c->words == 1) trim_paths<Key1>(c, flags, cutoff, out); else trim_paths<Key2>(c, flags, cutoff, out);
    });
}

int goss_gpu_clip_links(goss_gpu_ctx* c, uint32_t flags, goss_gpu_links_report* out)
{
    if (!c || !out || flags) return GOSS_ERR_INVALID_ARG;
    return paths_entry(c, out, "clip_links", "clip_links works on a graph", "clip_links belongs between finish and emit", [&]() {
        if (c->words == 1) clip_links<Key1>(c, out); else clip_links<Key2>(c, out);
    });
}

int goss_gpu_paths_timing(goss_gpu_ctx* c, float* ms)
{
    if (!c || !ms) return GOSS_ERR_INVALID_ARG;
    for (int i = 0; i < 5; ++i) ms[i] = c->paths_ms[i];
    return GOSS_OK;
}

int goss_gpu_trim_relative(goss_gpu_ctx* c, double rel, goss_gpu_relative_report* out)
{
    if (!c || !out) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "trim_relative", "trim_relative works on a graph", "trim_relative belongs between finish and emit")) return st;
    if (!std::isfinite(rel)) { c->last_error = "trim_relative: the relative cutoff must be a finite number"; return GOSS_ERR_INVALID_ARG; }
    const int rc = guarded(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        if (c->words == 1) trim_relative<Key1>(c, rel, out); else trim_relative<Key2>(c, rel, out);
        t.stop();
    });
    if (rc != GOSS_OK) std::memset(out, 0, sizeof *out);
    return rc;
}

int goss_gpu_relative_timing(goss_gpu_ctx* c, float* ms)
{
    if (!c || !ms) return GOSS_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i) ms[i] = c->relative_ms[i];
    return GOSS_OK;
}

int goss_gpu_segments_build(goss_gpu_ctx* c, uint64_t min_length, uint64_t min_coverage, uint32_t flags, goss_gpu_segments_info* out)
{
    if (!c || !out || (flags & ~(uint32_t)GOSS_SEGMENTS_NO_LINE_BREAKS)) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "segments", "segments are read from a graph", "segments belong between finish and emit")) return st;
    return build_held(c, Held::Segments, out, [&]() { segments_build(c, min_length, min_coverage, flags, out); });
}

int goss_gpu_segments_table(goss_gpu_ctx* c, uint64_t first, uint64_t count, goss_gpu_segment* out)
{
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind != Held::Segments) { c->last_error = "segments_table needs goss_gpu_segments_build before it"; return GOSS_ERR_STATE; }
    if (first > c->seg_count || count > c->seg_count - first) { c->last_error = "segments_table: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (count) HIP_TRY(hipMemcpyAsync(out, (const SegRec*)c->seg_recs + first, count * sizeof(SegRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_segments_text(goss_gpu_ctx* c, uint64_t text_offset, uint64_t bytes, char* dst)
{
    if (!c || (bytes && !dst)) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind != Held::Segments) { c->last_error = "segments_text needs goss_gpu_segments_build before it"; return GOSS_ERR_STATE; }
    if (text_offset > c->seg_text_bytes || bytes > c->seg_text_bytes - text_offset) { c->last_error = "segments_text: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (bytes) HIP_TRY(hipMemcpyAsync(dst, c->seg_text + text_offset, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_segments_release(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind == Held::Segments) release_held(c);
    return GOSS_OK;
}

int goss_gpu_entries_build(goss_gpu_ctx* c, goss_gpu_entries_info* out)
{
    if (!c || !out) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "entries", "an entry edge set is built from a graph", "entries belong between finish and emit")) return st;
    return build_held(c, Held::Entries, out, [&]() { entries_build(c, out); });
}

int goss_gpu_entries_release(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind == Held::Entries) release_held(c);
    return GOSS_OK;
}

static int components_mark_entry(goss_gpu_ctx* c, const void* bases, uint64_t nbytes, bool on_host, goss_gpu_mark_info* out)
{
    if (!c || !out || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "components", "edges are marked in a graph", "marking belongs between finish and emit")) return st;
    return build_held(c, Held::Components, out, [&]() { components_mark(c, bases, nbytes, on_host, out); },
                      c->held.kind == Held::Components && c->cmp_marks);
}

int goss_gpu_components_mark_host(goss_gpu_ctx* c, const void* bases, uint64_t nbytes, goss_gpu_mark_info* out)
{
    return components_mark_entry(c, bases, nbytes, true, out);
}

int goss_gpu_components_mark_device(goss_gpu_ctx* c, const void* d_bases, uint64_t nbytes, goss_gpu_mark_info* out)
{
    return components_mark_entry(c, d_bases, nbytes, false, out);
}

int goss_gpu_components_build(goss_gpu_ctx* c, uint32_t flags, goss_gpu_components_info* out)
{
    if (!c || !out || (flags & ~(uint32_t)GOSS_COMPONENTS_MARKED)) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "components", "components are found in a graph", "components belong between finish and emit")) return st;
    const bool marks = c->held.kind == Held::Components && c->cmp_marks;
    if ((flags & GOSS_COMPONENTS_MARKED) && !marks)
    {
        c->last_error = "components_build: GOSS_COMPONENTS_MARKED needs goss_gpu_components_mark_host / _device before it";
        return GOSS_ERR_STATE;
    }
    return build_held(c, Held::Components, out, [&]() {
        if (marks) components_drop_built(c); else c->cmp_built_lo = c->arena.lo;
        components_build(c, flags, out);
    }, marks);
}

int goss_gpu_components_table(goss_gpu_ctx* c, uint64_t first, uint64_t count, goss_gpu_component* out)
{
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind != Held::Components || !c->cmp_built) { c->last_error = "components_table needs goss_gpu_components_build before it"; return GOSS_ERR_STATE; }
    if (first > c->cmp_count || count > c->cmp_count - first) { c->last_error = "components_table: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (count) HIP_TRY(hipMemcpyAsync(out, (const CompRec*)c->cmp_recs + first, count * sizeof(CompRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_components_labels(goss_gpu_ctx* c, uint64_t first, uint64_t count, uint32_t* out)
{
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind != Held::Components || !c->cmp_built) { c->last_error = "components_labels needs goss_gpu_components_build before it"; return GOSS_ERR_STATE; }
    if (first > c->build.M || count > c->build.M - first) { c->last_error = "components_labels: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (count) HIP_TRY(hipMemcpyAsync(out, c->cmp_labels + first, count * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_components_keep(goss_gpu_ctx* c, uint64_t edge_rank, uint64_t* kept)
{
    if (!c || !kept) return GOSS_ERR_INVALID_ARG;
    *kept = 0;
    if (const int st = graph_pass_state(c, "components", "a component is kept of a graph", "keeping a component belongs between finish and emit")) return st;
    if (edge_rank >= c->build.M) { c->last_error = "components_keep: the graph has no edge of that rank"; return GOSS_ERR_INVALID_ARG; }
    return guarded(c, [&]() { *kept = components_keep(c, (uint32_t)edge_rank); });
}

int goss_gpu_components_release(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind == Held::Components) release_held(c);
    return GOSS_OK;
}

int goss_gpu_components_grow(goss_gpu_ctx* c, uint32_t radius, uint32_t flags, uint64_t* added, goss_gpu_grow_info* out)
{
    if (!c || !out || (flags & ~(uint32_t)GOSS_GROW_LINEAR_PATHS)) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (added) std::fill(added, added + radius, (uint64_t)0);
    if (const int st = graph_pass_state(c, "components_grow", "marks are grown in a graph", "growing the marks belongs between finish and emit")) return st;
    if (c->held.kind != Held::Components || !c->cmp_marks)
    {
        c->last_error = "components_grow needs goss_gpu_components_mark_host / _device before it";
        return GOSS_ERR_STATE;
    }
    return build_held(c, Held::Components, out, [&]() {
        components_drop_built(c);
        components_grow(c, radius, flags, added, out);
    }, true);
}

int goss_gpu_components_marks(goss_gpu_ctx* c, uint64_t first, uint64_t count, uint8_t* out)
{
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind != Held::Components || !c->cmp_marks) { c->last_error = "components_marks needs goss_gpu_components_mark_host / _device before it"; return GOSS_ERR_STATE; }
    if (first > c->build.M || count > c->build.M - first) { c->last_error = "components_marks: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (!count) return;
        const uint64_t w0 = first / 32, w1 = (first + count + 31) / 32;
        std::vector<uint32_t> words((size_t)(w1 - w0));
        HIP_TRY(hipMemcpyAsync(words.data(), c->cmp_marks + w0, (w1 - w0) * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < count; ++i)
        {
            const uint64_t b = first + i;
            out[i] = (uint8_t)((words[(size_t)(b / 32 - w0)] >> (b & 31u)) & 1u);
        }
    });
}

int goss_gpu_components_keep_marked(goss_gpu_ctx* c, uint64_t* kept)
{
    if (!c || !kept) return GOSS_ERR_INVALID_ARG;
    *kept = 0;
    if (const int st = graph_pass_state(c, "components", "the marked edges are kept of a graph", "keeping the marked edges belongs between finish and emit")) return st;
    if (c->held.kind != Held::Components || !c->cmp_marks)
    {
        c->last_error = "components_keep_marked needs goss_gpu_components_mark_host / _device before it";
        return GOSS_ERR_STATE;
    }
    // (the marks are read first; components_keep_marked gives them back)
    const int rc = guarded_reading(c, [&]() { *kept = components_keep_marked(c); });
    if (c->held.kind != Held::None) release_held(c);
    return rc;
}

// ---- read links -------------------------------------------------------------------------------------------------------

int goss_gpu_read_links_begin(goss_gpu_ctx* c, uint32_t flags, const uint8_t* unique, uint64_t unique_bits, goss_gpu_read_links_info* out)
{
    if (!c || !out || (flags & ~(uint32_t)GOSS_LINKS_CARRY) || (!unique && unique_bits)) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "read_links", "reads are threaded over a graph", "read links belong between finish and emit")) return st;
    return build_held(c, Held::Links, out, [&]() {
        if (c->words == 1) read_links_begin<Key1>(c, flags, unique, unique_bits, out);
        else read_links_begin<Key2>(c, flags, unique, unique_bits, out);
    });
}

static int read_links_state(goss_gpu_ctx* c, const char* who)
{
    if (c->held.kind == Held::Links) return GOSS_OK;
    c->last_error = std::string(who) + " needs goss_gpu_read_links_begin before it";
    return GOSS_ERR_STATE;
}

int goss_gpu_read_links_segments(goss_gpu_ctx* c, uint64_t first, uint64_t count, uint32_t* out)
{
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (const int st = read_links_state(c, "read_links_segments")) return st;
    if (first > c->build.M || count > c->build.M - first) { c->last_error = "read_links_segments: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (count) HIP_TRY(hipMemcpyAsync(out, c->lnk_seg_of + first, count * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

static int read_links_batch_entry(goss_gpu_ctx* c, const void* bases, uint64_t n, uint32_t* out, uint64_t capacity, bool accumulate,
                                  goss_gpu_read_links_batch* info, const char* who)
{
    if (!c || !info || (!bases && n) || (!accumulate && capacity && !out)) return GOSS_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    if (const int st = read_links_state(c, who)) return st;
    const int rc = guarded_reading(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, n);
        if (c->words == 1) read_links_batch<Key1>(c, bases, n, out, capacity, accumulate, info);
        else read_links_batch<Key2>(c, bases, n, out, capacity, accumulate, info);
        t.stop();
    });
    if (rc != GOSS_OK) std::memset(info, 0, sizeof *info);
    return rc;
}

int goss_gpu_read_links_windows_host(goss_gpu_ctx* c, const void* bases, uint64_t n, uint32_t* out, uint64_t capacity, goss_gpu_read_links_batch* info)
{
    return read_links_batch_entry(c, bases, n, out, capacity, false, info, "read_links_windows");
}

int goss_gpu_read_links_add_host(goss_gpu_ctx* c, const void* bases, uint64_t n, goss_gpu_read_links_batch* info)
{
    return read_links_batch_entry(c, bases, n, nullptr, 0, true, info, "read_links_add");
}

int goss_gpu_read_links_finish(goss_gpu_ctx* c, goss_gpu_read_links_table_info* info)
{
    if (!c || !info) return GOSS_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    if (const int st = read_links_state(c, "read_links_finish")) return st;
    const int rc = guarded_reading(c, [&]() {
        PhaseTimer t(c, GOSS_T_REDUCE, c->lnk_records);
        read_links_finish(c, info);
        t.stop();
    });
    if (rc != GOSS_OK) std::memset(info, 0, sizeof *info);
    return rc;
}

int goss_gpu_read_links_table(goss_gpu_ctx* c, uint64_t first, uint64_t count, goss_gpu_link_row* out)
{
    static_assert(sizeof(goss_gpu_link_row) == sizeof(LinkRow), "link row layout");
    if (!c || (count && !out)) return GOSS_ERR_INVALID_ARG;
    if (const int st = read_links_state(c, "read_links_table")) return st;
    if (!c->lnk_reduced) { c->last_error = "read_links_table needs goss_gpu_read_links_finish before it"; return GOSS_ERR_STATE; }
    if (first > c->lnk_row_count || count > c->lnk_row_count - first) { c->last_error = "read_links_table: a range past the end"; return GOSS_ERR_INVALID_ARG; }
    return guarded_reading(c, [&]() {
        if (count) HIP_TRY(hipMemcpyAsync(out, (const LinkRow*)c->lnk_rows + first, count * sizeof(LinkRow), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_gpu_read_links_release(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind == Held::Links) release_held(c);
    return GOSS_OK;
}

// ---- pool-samples ---------------------------------------------------------------------------------------------------

static int pool_state(goss_gpu_ctx* c, const char* who)
{
    if (c->held.kind == Held::Pool) return GOSS_OK;
    c->last_error = std::string(who) + " needs goss_gpu_pool_begin before it";
    return GOSS_ERR_STATE;
}

int goss_gpu_pool_begin(goss_gpu_ctx* c, uint32_t nsets, uint64_t z)
{
    if (!c || nsets == 0 || z == 0) return GOSS_ERR_INVALID_ARG;
    if (z > ~0ULL / nsets) { c->last_error = "pool_begin: z * nsets does not fit 64 bits"; return GOSS_ERR_INVALID_ARG; }
    // the rows are permanent allocations: between pushes a later merge or an out-of-memory rollback would rewind the
    // permanent end underneath them (the rule of goss_gpu_emit_sparse_array)
    if (!c->build.finished && (!c->build.runs.empty() || c->stage_fill))
    {
        c->last_error = "pool_begin while a count is in progress (reset or finish first)";
        return GOSS_ERR_STATE;
    }
    const int rc = guarded(c, [&]() { pool_begin(c, nsets, z); });
    if (rc != GOSS_OK && c->held.kind != Held::None) release_held(c);
    return rc;
}

int goss_gpu_pool_add_masks(goss_gpu_ctx* c, uint32_t first_set, uint32_t nbits, const uint32_t* d_masks, uint64_t z)
{
    if (!c || !d_masks || nbits == 0 || nbits > 32) return GOSS_ERR_INVALID_ARG;
    if (const int st = pool_state(c, "pool_add_masks")) return st;
    if (z != c->pool_z) { c->last_error = "pool_add_masks: z differs from goss_gpu_pool_begin's"; return GOSS_ERR_INVALID_ARG; }
    if (first_set >= c->pool_sets || nbits > c->pool_sets - first_set) { c->last_error = "pool_add_masks: sets past the end"; return GOSS_ERR_INVALID_ARG; }
    for (uint32_t i = 0; i < nbits; ++i)
        if (c->pool_added[first_set + i]) { c->last_error = "pool_add_masks: set " + std::to_string(first_set + i) + " was added before"; return GOSS_ERR_STATE; }
    return guarded_reading(c, [&]() { pool_add_masks(c, first_set, nbits, d_masks); });
}

int goss_gpu_pool_sizes(goss_gpu_ctx* c, uint64_t* sizes)
{
    if (!c || !sizes) return GOSS_ERR_INVALID_ARG;
    if (const int st = pool_state(c, "pool_sizes")) return st;
    return guarded_reading(c, [&]() { pool_sizes(c, sizes); });
}

int goss_gpu_pool_intersections(goss_gpu_ctx* c, uint64_t* inter)
{
    if (!c || !inter) return GOSS_ERR_INVALID_ARG;
    if (const int st = pool_state(c, "pool_intersections")) return st;
    return guarded_reading(c, [&]() { pool_intersections(c, inter); });
}

int goss_gpu_pool_emit_index(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (const int st = pool_state(c, "pool_emit_index")) return st;
    const int rc = guarded_reading(c, [&]() { pool_emit_index(c); });
    if (rc != GOSS_OK) { c->build.files.clear(); c->arena.lo = c->pool_top; }       // the rows stay; no half-built index does
    return rc;
}

int goss_gpu_pool_release(goss_gpu_ctx* c)
{
    if (!c) return GOSS_ERR_INVALID_ARG;
    if (c->held.kind == Held::Pool) release_held(c);
    return GOSS_OK;
}

int goss_gpu_emit_count_bits(goss_gpu_ctx* c, uint32_t mask, const char* suffix)
{
    if (!c || !suffix || !mask) return GOSS_ERR_INVALID_ARG;
    if (!c->build.emitted) { c->last_error = "emit_count_bits follows emit"; return GOSS_ERR_STATE; }
    return guarded(c, [&]() {
        // WordyBitVector::Builder after M push_backX calls and end(): floor((M-1)/64)+1 words,
        // one (zero) word when nothing was pushed (WordyBitVector.hh:90-116, .cc:18-29)
        const uint64_t m = c->build.M, nwords = m ? (m - 1) / 64 + 1 : 1;
        uint64_t* words = (uint64_t*)c->arena.perm(nwords * 8);
        if (m == 0) HIP_TRY(hipMemsetAsync(words, 0, 8, c->stream));
        else
            hipLaunchKernelGGL(count_bits_kernel, dim3(grid_for((nwords + 63) / 64 * 64, 256)), dim3(256), 0, c->stream,
                               (const uint32_t*)c->build.res_counts, m, mask, words, nwords);
        HIP_TRY(hipStreamSynchronize(c->stream));
        add_dev_file(c, suffix, words, nwords * 8);
    });
}

int goss_gpu_synth_reads(goss_gpu_ctx* c, void* d_out, uint64_t nreads, uint32_t read_len, uint64_t genome_len,
                         uint64_t seed, uint64_t first_read)
{
    if (!c || !d_out || read_len == 0 || genome_len < read_len) return GOSS_ERR_INVALID_ARG;
    return guarded(c, [&]() {
        hipLaunchKernelGGL(synth_reads_kernel, dim3(256 * 8), dim3(256), 0, c->stream, (uint8_t*)d_out, nreads, read_len,
                           genome_len, seed, first_read);
        HIP_TRY(hipStreamSynchronize(c->stream));
    });
}

int goss_synth_reads_host(char* out, uint64_t nreads, uint32_t read_len, uint64_t genome_len, uint64_t seed,
                          uint64_t first_read)
{
    if (!out || read_len == 0 || genome_len < read_len) return GOSS_ERR_INVALID_ARG;
    const uint64_t stride = read_len + 1;
    for (uint64_t r = 0; r < nreads; ++r)
        for (uint32_t j = 0; j <= read_len; ++j)
            out[r * stride + j] = synth_read_byte(seed, genome_len, read_len, first_read + r, j);
    return GOSS_OK;
}

}  // extern "C"

// ============================================================================================
// Objects opened for queries (goss_gpu_object_*): one KmerSet, Graph or SparseArray in one
// allocation of its own, outside every context's arena
// ============================================================================================

#include "object_path.hpp"

extern "C" {

int goss_gpu_object_open(goss_gpu_object** out, int device, void* stream, int kind, const char* base,
                         const goss_gpu_named_file* files, uint32_t nfiles)
{
    if (!out) return GOSS_ERR_INVALID_ARG;
    *out = nullptr;
    t_open_error.clear();
    if (kind != GOSS_OBJECT_KMER_SET && kind != GOSS_OBJECT_GRAPH && kind != GOSS_OBJECT_SPARSE_ARRAY && kind != GOSS_OBJECT_ENTRY_EDGE_SET)
        return GOSS_ERR_INVALID_ARG;
    if (!base || (!files && nfiles)) return GOSS_ERR_INVALID_ARG;
    if (int rc = usable_device(device)) return rc;
    ObjFiles fs;
    for (uint32_t i = 0; i < nfiles; ++i)
    {
        if (!files[i].name) return GOSS_ERR_INVALID_ARG;
        fs[files[i].name] = ObjSrc{(const uint8_t*)files[i].data, files[i].bytes, false};
    }
    return object_open(out, device, stream, kind, base, fs);
}

int goss_gpu_object_open_emitted(goss_gpu_object** out, goss_gpu_ctx* c)
{
    if (!out || !c) return GOSS_ERR_INVALID_ARG;
    *out = nullptr;
    t_open_error.clear();
    ObjFiles fs;
    for (auto& f : c->build.files) fs[f.suffix] = ObjSrc{f.dev ? f.dev : f.host.data(), f.size, f.dev != nullptr};
    int kind = -1;
    std::string base;
    if (fs.count(".kmers.header")) kind = GOSS_OBJECT_KMER_SET;
    else if (fs.count("-edges.header")) kind = GOSS_OBJECT_GRAPH;
    else if (fs.count(".high-bits")) kind = GOSS_OBJECT_SPARSE_ARRAY;
    else if (fs.count("-entries.header")) { kind = GOSS_OBJECT_ENTRY_EDGE_SET; base = "-entries"; }
    if (kind < 0) { t_open_error = "the context holds no emitted KmerSet, Graph, SparseArray or EntryEdgeSet"; return GOSS_ERR_STATE; }
    // what the context's stream still writes into its files (the call only reads: what is held stays)
    int rc = guarded_reading(c, [&]() { HIP_TRY(hipStreamSynchronize(c->stream)); });
    if (rc != GOSS_OK) { t_open_error = c->last_error; return rc; }
    return object_open(out, c->device, nullptr, kind, base, fs);
}

void goss_gpu_object_close(goss_gpu_object* o) { object_free(o); }

const char* goss_gpu_object_last_error(const goss_gpu_object* o) { return o ? o->last_error.c_str() : t_open_error.c_str(); }

int goss_gpu_object_info(const goss_gpu_object* o, goss_gpu_object_desc* out)
{
    if (!o || !out) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    out->kind = o->kind; out->K = o->K; out->count = o->q.s.count; out->key_words = o->key_words;
    out->asymmetric = o->asymmetric ? 1 : 0; out->N_lo = o->q.s.size_lo; out->N_hi = o->q.s.size_hi; out->D = o->q.s.D;
    out->resident_bytes = o->bytes;
    return GOSS_OK;
}

int goss_gpu_object_rank(goss_gpu_object* o, const void* d_keys, uint64_t n, uint32_t flags, uint64_t* d_rank, uint8_t* d_present)
{
    if (!o || (!d_keys && n) || (flags & ~(uint32_t)GOSS_QUERY_NORMALIZE)) return GOSS_ERR_INVALID_ARG;
    if ((flags & GOSS_QUERY_NORMALIZE) && o->kind == GOSS_OBJECT_SPARSE_ARRAY) { o->last_error = "a bare SparseArray has no strands"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        if (o->key_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_rank_kernel<Key1>), grid, dim3(256), 0, o->stream, o->q, (const Key1*)d_keys, n, flags, d_rank, d_present, o->d_bad);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_rank_kernel<Key2>), grid, dim3(256), 0, o->stream, o->q, (const Key2*)d_keys, n, flags, d_rank, d_present, o->d_bad);
    });
}

int goss_gpu_object_select(goss_gpu_object* o, const uint64_t* d_ranks, uint64_t n, void* d_keys)
{
    if (!o || ((!d_ranks || !d_keys) && n)) return GOSS_ERR_INVALID_ARG;
    return object_query(o, n, [&](dim3 grid) {
        if (o->key_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_select_kernel<Key1>), grid, dim3(256), 0, o->stream, o->q, d_ranks, n, (Key1*)d_keys, o->d_bad);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_select_kernel<Key2>), grid, dim3(256), 0, o->stream, o->q, d_ranks, n, (Key2*)d_keys, o->d_bad);
    });
}

int goss_gpu_object_multiplicity(goss_gpu_object* o, const uint64_t* d_ranks, uint64_t n, uint32_t* d_counts)
{
    if (!o || ((!d_ranks || !d_counts) && n)) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_GRAPH && o->kind != GOSS_OBJECT_ENTRY_EDGE_SET) { o->last_error = "multiplicity needs a Graph or an EntryEdgeSet"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        hipLaunchKernelGGL(query_multiplicity_kernel, grid, dim3(256), 0, o->stream, o->q, d_ranks, n, d_counts, o->d_bad);
    });
}

int goss_gpu_object_lookup(goss_gpu_object* o, const void* d_keys, uint64_t n, uint32_t flags, uint32_t* d_counts)
{
    if (!o || ((!d_keys || !d_counts) && n) || (flags & ~(uint32_t)GOSS_QUERY_NORMALIZE)) return GOSS_ERR_INVALID_ARG;
    if ((flags & GOSS_QUERY_NORMALIZE) && o->kind == GOSS_OBJECT_SPARSE_ARRAY) { o->last_error = "a bare SparseArray has no strands"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        if (o->key_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_lookup_kernel<Key1>), grid, dim3(256), 0, o->stream, o->q, (const Key1*)d_keys, n, flags, d_counts, o->d_bad);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_lookup_kernel<Key2>), grid, dim3(256), 0, o->stream, o->q, (const Key2*)d_keys, n, flags, d_counts, o->d_bad);
    });
}

// merge-graph-with-reference (TransCmdMergeGraphWithReference.cc:47-114): recount_from of graph_passes.hpp, over the
// context's result and an open graph that is only read
int goss_gpu_recount_from(goss_gpu_ctx* c, goss_gpu_object* ref, goss_gpu_recount_report* out)
{
    if (!c || !ref || !out) return GOSS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    if (const int st = graph_pass_state(c, "recount_from", "recount_from works on a graph", "recount_from belongs between finish and emit")) return st;
    if (ref->kind != GOSS_OBJECT_GRAPH) { c->last_error = "recount_from: the reference must be a Graph"; return GOSS_ERR_INVALID_ARG; }
    if (ref->K != c->k)
    {
        c->last_error = "recount_from: graphs involved in a merge must have the same kmer-size: the context has k=" + std::to_string(c->k) +
                        ", the reference has k=" + std::to_string(ref->K);
        return GOSS_ERR_INVALID_ARG;
    }
    if (ref->asymmetric) { c->last_error = "recount_from: the reference preserves sense; asymmetric graphs are not handled"; return GOSS_ERR_INVALID_ARG; }
    if (ref->device != c->device) { c->last_error = "recount_from: the reference lives on another device"; return GOSS_ERR_INVALID_ARG; }
    const int rc = guarded(c, [&]() {
        HIP_TRY(hipStreamSynchronize(ref->stream));      // (what the reference's own stream still does with its images)
        PhaseTimer t(c, GOSS_T_REDUCE, c->build.M);
        if (c->words == 1) recount_from<Key1>(c, ref->q, out); else recount_from<Key2>(c, ref->q, out);
        t.stop();
    });
    if (rc != GOSS_OK) std::memset(out, 0, sizeof *out);
    return rc;
}

int goss_gpu_object_node_ranks(goss_gpu_object* o, const void* d_nodes, uint64_t n, uint32_t flags, uint64_t* d_begin, uint64_t* d_end)
{
    if (!o || (!d_nodes && n) || (flags & ~(uint32_t)(GOSS_QUERY_NORMALIZE | GOSS_QUERY_INCOMING))) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_GRAPH) { o->last_error = "node ranks need a Graph"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        if (o->key_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_node_ranks_kernel<Key1, Key1>), grid, dim3(256), 0, o->stream, o->q, (const Key1*)d_nodes, n, flags, d_begin, d_end, o->d_bad);
        else if (o->node_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_node_ranks_kernel<Key1, Key2>), grid, dim3(256), 0, o->stream, o->q, (const Key1*)d_nodes, n, flags, d_begin, d_end, o->d_bad);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(query_node_ranks_kernel<Key2, Key2>), grid, dim3(256), 0, o->stream, o->q, (const Key2*)d_nodes, n, flags, d_begin, d_end, o->d_bad);
    });
}

int goss_gpu_entries_length(goss_gpu_object* o, const uint64_t* d_ranks, uint64_t n, uint32_t* d_lengths)
{
    if (!o || ((!d_ranks || !d_lengths) && n)) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_ENTRY_EDGE_SET) { o->last_error = "length needs an EntryEdgeSet"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        hipLaunchKernelGGL(query_length_kernel, grid, dim3(256), 0, o->stream, o->qe, d_ranks, n, d_lengths, o->d_bad);
    });
}

int goss_gpu_entries_end_rank(goss_gpu_object* o, const uint64_t* d_ranks, uint64_t n, uint64_t* d_ends)
{
    if (!o || ((!d_ranks || !d_ends) && n)) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_ENTRY_EDGE_SET) { o->last_error = "end_rank needs an EntryEdgeSet"; return GOSS_ERR_INVALID_ARG; }
    return object_query(o, n, [&](dim3 grid) {
        hipLaunchKernelGGL(query_end_rank_kernel, grid, dim3(256), 0, o->stream, o->qe, d_ranks, n, d_ends, o->d_bad);
    });
}

// compute-near-kmers (GossCmdComputeNearKmers.cc:58-121): kernels_near.hpp
int goss_gpu_object_near_kmers(goss_gpu_object* o, const uint64_t* d_lhs, const uint64_t* d_rhs, uint32_t flags,
                               uint64_t* d_lhs_out, uint64_t* d_rhs_out, uint64_t* gray)
{
    if (!o || !gray || (flags & ~(uint32_t)(GOSS_NEAR_WHOLE_BASES | GOSS_NEAR_NORMALIZE))) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "near_kmers needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    *gray = 0;
    const uint64_t nwords = (o->q.s.count + 63) / 64, bytes = nwords * 8;
    if (nwords == 0) return GOSS_OK;
    if (!d_lhs || !d_rhs || !d_lhs_out || !d_rhs_out) { o->last_error = "near_kmers: a bitmap pointer is NULL"; return GOSS_ERR_INVALID_ARG; }
    auto overlap = [&](const void* a, const void* b) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + bytes && y < x + bytes;
    };
    if (overlap(d_lhs_out, d_lhs) || overlap(d_lhs_out, d_rhs) || overlap(d_rhs_out, d_lhs) || overlap(d_rhs_out, d_rhs) ||
        overlap(d_lhs_out, d_rhs_out))
    {
        o->last_error = "near_kmers: an output bitmap overlaps an input or the other output (the kernel reads old bits only)";
        return GOSS_ERR_INVALID_ARG;
    }
    return obj_guarded(o->device, o->last_error, [&]() {
        HIP_TRY(hipMemsetAsync(o->d_bad, 0xFF, 8, o->stream));
        HIP_TRY(hipMemsetAsync(o->d_bad + 1, 0, 8, o->stream));
        const dim3 grid((uint32_t)std::min<uint64_t>(((nwords + 63) / 64 + 3) / 4, 65536));       // (a wave per 64 words)
        if (o->key_words == 1)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(near_kmers_kernel<Key1>), grid, dim3(256), 0, o->stream, o->q, d_lhs, d_rhs, flags, d_lhs_out, d_rhs_out, o->d_bad + 1, o->d_bad);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(near_kmers_kernel<Key2>), grid, dim3(256), 0, o->stream, o->q, d_lhs, d_rhs, flags, d_lhs_out, d_rhs_out, o->d_bad + 1, o->d_bad);
        HIP_TRY(hipMemcpyAsync(o->h_bad, o->d_bad, 16, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        const unsigned long long bad = o->h_bad[0];
        if (bad != ~0ULL)
            throw StatusError{GOSS_ERR_INVALID_ARG, "rank " + std::to_string(bad >> 2) + ": the index walk cannot answer (damaged object)"};
        *gray = o->h_bad[1];
    });
}

int goss_gpu_object_near_kmers_host(goss_gpu_object* o, const uint64_t* lhs, const uint64_t* rhs, uint32_t flags,
                                    uint64_t* lhs_out, uint64_t* rhs_out, uint64_t* gray)
{
    if (!o || !gray) return GOSS_ERR_INVALID_ARG;
    const uint64_t nwords = o->kind == GOSS_OBJECT_KMER_SET ? (o->q.s.count + 63) / 64 : 0, bytes = nwords * 8;
    if (nwords == 0) return goss_gpu_object_near_kmers(o, nullptr, nullptr, flags, nullptr, nullptr, gray);
    if (!lhs || !rhs || !lhs_out || !rhs_out) { o->last_error = "near_kmers: a bitmap pointer is NULL"; return GOSS_ERR_INVALID_ARG; }
    uint64_t* d = nullptr;
    int rc = obj_guarded(o->device, o->last_error, [&]() {
        HIP_TRY(hipMalloc((void**)&d, 4 * bytes));
        HIP_TRY(hipMemcpyAsync(d, lhs, bytes, hipMemcpyHostToDevice, o->stream));
        HIP_TRY(hipMemcpyAsync(d + nwords, rhs, bytes, hipMemcpyHostToDevice, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
    });
    if (rc == GOSS_OK) rc = goss_gpu_object_near_kmers(o, d, d + nwords, flags, d + 2 * nwords, d + 3 * nwords, gray);
    if (rc == GOSS_OK)
        rc = obj_guarded(o->device, o->last_error, [&]() {
            HIP_TRY(hipMemcpyAsync(lhs_out, d + 2 * nwords, bytes, hipMemcpyDeviceToHost, o->stream));
            HIP_TRY(hipMemcpyAsync(rhs_out, d + 3 * nwords, bytes, hipMemcpyDeviceToHost, o->stream));
            HIP_TRY(hipStreamSynchronize(o->stream));
        });
    if (d) (void)hipFree(d);
    return rc;
}

}  // extern "C"

// ============================================================================================
// Reads against an object (goss_gpu_object_match_reads, _classify_reads, _taxo_*, _colour_reads): the pass, the staged
// batch, the classify bitmaps, the taxonomy and the colour words are reads_path.hpp; what follows checks the arguments
// and calls it
// ============================================================================================

#include "reads_path.hpp"

extern "C" {

int goss_gpu_object_match_reads(goss_gpu_object* o, const void* d_bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                uint32_t* d_windows, uint32_t* d_hits, uint64_t* d_read_starts, goss_gpu_match_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)(GOSS_MATCH_NORMALIZE | GOSS_MATCH_ANY)) { o->last_error = "match_reads: unknown flag bits"; return GOSS_ERR_INVALID_ARG; }
    if (o->kind == GOSS_OBJECT_SPARSE_ARRAY) { o->last_error = "match_reads needs a KmerSet or a Graph: a bare SparseArray has no key length"; return GOSS_ERR_INVALID_ARG; }
    ReadsPass res;
    const int rc = reads_pass(o, ReadsJob{"match_reads", flags & GOSS_MATCH_ANY ? kModeAny : kModeCount, d_bases, nbytes, flags, max_reads, d_windows, d_hits, d_read_starts}, &res);
    return pass_report(rc, res, info, [&](goss_gpu_match_info& i) { i.windows = res.sums[0]; i.hits = res.sums[1]; i.matched_reads = res.sums[2]; });
}

int goss_gpu_object_match_reads_host(goss_gpu_object* o, const void* bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                     uint32_t* windows, uint32_t* hits, uint64_t* read_starts, goss_gpu_match_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    return reads_staged(o, bases, nbytes, max_reads, windows, hits, read_starts, nullptr, info, [&](const StagedBatch& s, goss_gpu_match_info* mine) {
        return goss_gpu_object_match_reads(o, s.bases, nbytes, flags, max_reads, s.a, s.b, s.starts, mine);
    });
}

int goss_gpu_object_classify_bits_host(goss_gpu_object* o, const uint64_t* lhs, const uint64_t* rhs)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "classify_bits needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (o->q.s.count && (!lhs || !rhs)) { o->last_error = "classify_bits: a bitmap pointer is NULL"; return GOSS_ERR_INVALID_ARG; }
    return obj_guarded(o->device, o->last_error, [&]() { classify_keep_bits(o, lhs, rhs); });
}

int goss_gpu_object_classify_reads(goss_gpu_object* o, const void* d_bases, uint64_t nbytes, const uint64_t* d_lhs, const uint64_t* d_rhs,
                                   uint32_t flags, uint64_t max_reads, uint32_t* d_classes, uint32_t* d_windows, uint64_t* d_read_starts,
                                   goss_gpu_classify_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)GOSS_CLASSIFY_NORMALIZE) { o->last_error = "classify_reads: unknown flag bits"; return GOSS_ERR_INVALID_ARG; }
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "classify_reads needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (!d_lhs != !d_rhs) { o->last_error = "classify_reads: one bitmap pointer is NULL and the other is not"; return GOSS_ERR_INVALID_ARG; }
    const uint64_t nwords = (o->q.s.count + 63) / 64;
    if (!d_lhs && nwords)
    {
        if (!o->classify_kept)
        {
            o->last_error = "classify_reads: no bitmaps given and none kept (goss_gpu_object_classify_bits_host)";
            return GOSS_ERR_INVALID_ARG;
        }
        d_lhs = o->classify_bits;
        d_rhs = o->classify_bits + nwords;
    }
    ReadsPass res;
    const int rc = reads_pass(o, ReadsJob{"classify_reads", kModeClassify, d_bases, nbytes, flags, max_reads, d_windows, d_classes, d_read_starts, false,
                                          MatchAux{d_lhs, d_rhs, TaxoView{}}}, &res);
    return pass_report(rc, res, info, [&](goss_gpu_classify_info& i) {
        i.windows = res.sums[0];
        for (int k = 0; k < 16; ++k) i.counts[k] = res.counts[k];
    });
}

int goss_gpu_object_classify_reads_host(goss_gpu_object* o, const void* bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                        uint32_t* classes, uint32_t* windows, uint64_t* read_starts, goss_gpu_classify_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    return reads_staged(o, bases, nbytes, max_reads, windows, classes, read_starts, nullptr, info, [&](const StagedBatch& s, goss_gpu_classify_info* mine) {
        return goss_gpu_object_classify_reads(o, s.bases, nbytes, nullptr, nullptr, flags, max_reads, s.b, s.a, s.starts, mine);
    });
}

int goss_gpu_object_colours_host(goss_gpu_object* o, const uint64_t* colours, uint32_t ncolours)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "colours needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (ncolours < 1 || ncolours > GOSS_ELECT_MAX_COLOURS) { o->last_error = "colours: ncolours must be 1 .. 64"; return GOSS_ERR_INVALID_ARG; }
    if (o->q.s.count && !colours) { o->last_error = "colours: the pointer is NULL"; return GOSS_ERR_INVALID_ARG; }
    return obj_guarded(o->device, o->last_error, [&]() { colours_keep_host(o, colours, ncolours); });
}

int goss_gpu_object_colours_from_index(goss_gpu_object* o, goss_gpu_object* index, uint32_t* ncolours_out)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "colours_from_index needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (!index || index->kind != GOSS_OBJECT_SPARSE_ARRAY) { o->last_error = "colours_from_index: the index must be a SparseArray"; return GOSS_ERR_INVALID_ARG; }
    if (index->device != o->device) { o->last_error = "colours_from_index: the index lies on another device"; return GOSS_ERR_INVALID_ARG; }
    return obj_guarded(o->device, o->last_error, [&]() {
        const uint32_t S = colours_keep_index(o, index);
        if (ncolours_out) *ncolours_out = S;
    });
}

int goss_gpu_object_colour_reads(goss_gpu_object* o, const void* d_bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                 uint64_t* d_colours, uint32_t* d_windows, uint64_t* d_read_starts, goss_gpu_elect_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)GOSS_ELECT_NORMALIZE) { o->last_error = "colour_reads: unknown flag bits"; return GOSS_ERR_INVALID_ARG; }
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "colour_reads needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (o->q.s.count && !o->colours_kept)
    {
        o->last_error = "colour_reads: no colours kept (goss_gpu_object_colours_host, goss_gpu_object_colours_from_index)";
        return GOSS_ERR_INVALID_ARG;
    }
    MatchAux aux;
    aux.colours = o->colours;
    ReadsPass res;
    const int rc = reads_pass(o, ReadsJob{"colour_reads", kModeColour, d_bases, nbytes, flags, max_reads, d_windows, reinterpret_cast<uint32_t*>(d_colours),
                                          d_read_starts, false, aux}, &res);
    return pass_report(rc, res, info, [&](goss_gpu_elect_info& i) {
        i.windows = res.sums[0];
        for (int k = 0; k < 65; ++k) i.by_count[k] = res.by_count[k];
    });
}

int goss_gpu_object_colour_reads_host(goss_gpu_object* o, const void* bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                      uint64_t* colours, uint32_t* windows, uint64_t* read_starts, goss_gpu_elect_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    return reads_staged(o, bases, nbytes, max_reads, windows, reinterpret_cast<uint32_t*>(colours), read_starts, nullptr, info,
                        [&](const StagedBatch& s, goss_gpu_elect_info* mine) {
                            return goss_gpu_object_colour_reads(o, s.bases, nbytes, flags, max_reads, reinterpret_cast<uint64_t*>(s.b), s.a, s.starts, mine);
                        }, 8);
}

int goss_gpu_object_taxo_tree_host(goss_gpu_object* o, uint32_t n, const uint32_t* ids, const uint32_t* parent_index)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "taxo_tree needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (!n || !ids || !parent_index) { o->last_error = "taxo_tree: no nodes"; return GOSS_ERR_INVALID_ARG; }
    if (n >= 0xFFFFFFFEu) { o->last_error = "taxo_tree: too many nodes"; return GOSS_ERR_INVALID_ARG; }
    return obj_guarded(o->device, o->last_error, [&]() { taxo_build_tree(o, n, ids, parent_index); });
}

int goss_gpu_object_taxo_annotation_host(goss_gpu_object* o, const uint32_t* ann)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    bool empty = false;
    const int rc = taxo_ready(o, "taxo_annotation", false, &empty);
    if (rc != GOSS_OK || empty) return rc;
    return obj_guarded(o->device, o->last_error, [&]() { taxo_keep_annotation(o, ann); });
}

int goss_gpu_object_taxo_annotation_read(goss_gpu_object* o, uint32_t* ann_out, uint64_t* counts_out)
{
    if (!o) return GOSS_ERR_INVALID_ARG;
    bool empty = false;
    const int rc = taxo_ready(o, "taxo_annotation_read", true, &empty);
    if (rc != GOSS_OK) return rc;
    if (empty)
    {
        if (counts_out) for (uint32_t i = 0; i < o->taxo_n; ++i) counts_out[i] = 0;
        return GOSS_OK;
    }
    return obj_guarded(o->device, o->last_error, [&]() { taxo_read_annotation(o, ann_out, counts_out); });
}

int goss_gpu_object_taxo_annotate(goss_gpu_object* o, const void* d_bases, uint64_t nbytes, const uint32_t* d_read_nodes, uint32_t flags,
                                  uint64_t max_reads, uint32_t* d_windows, goss_gpu_taxo_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)GOSS_TAXO_NORMALIZE) { o->last_error = "taxo_annotate: unknown flag bits"; return GOSS_ERR_INVALID_ARG; }
    bool empty = false;
    int rc = taxo_ready(o, "taxo_annotate", true, &empty);
    if (rc != GOSS_OK) return rc;
    if (!d_read_nodes && max_reads && nbytes) { o->last_error = "taxo_annotate: no node ids for the reads"; return GOSS_ERR_INVALID_ARG; }
    if (empty)
        return taxo_empty_pass(o, "taxo_annotate", d_bases, nbytes, flags, max_reads, nullptr, d_windows, nullptr, true, info);
    if (nbytes == 0) return GOSS_OK;
    ReadsJob job{"taxo_annotate", kModeAnnotate, d_bases, nbytes, flags, max_reads, d_windows, nullptr, nullptr, true};
    rc = obj_guarded(o->device, o->last_error, [&]() {
        uint32_t* cls = (uint32_t*)o->taxo_scratch.room(max_reads * 4 + 256);
        taxo_dense(o, "taxo_annotate", "read", d_read_nodes, max_reads, 0, cls);
        job.aux.tx = taxo_view(o);
        job.aux.tx.read_class = cls;
    });
    if (rc != GOSS_OK) return rc;
    ReadsPass res;
    rc = reads_pass(o, job, &res);
    return pass_report(rc, res, info, [&](goss_gpu_taxo_info& i) { i.windows = res.sums[0]; i.hits = res.sums[1]; });
}

int goss_gpu_object_taxo_classify_reads(goss_gpu_object* o, const void* d_bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                        uint32_t* d_result, uint32_t* d_windows, uint64_t* d_read_starts, goss_gpu_taxo_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!d_bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (flags & ~(uint32_t)GOSS_TAXO_NORMALIZE) { o->last_error = "taxo_classify_reads: unknown flag bits"; return GOSS_ERR_INVALID_ARG; }
    bool empty = false;
    int rc = taxo_ready(o, "taxo_classify_reads", true, &empty);
    if (rc != GOSS_OK) return rc;
    if (empty) return taxo_empty_pass(o, "taxo_classify_reads", d_bases, nbytes, flags, max_reads, d_result, d_windows, d_read_starts, false, info);
    ReadsPass res;
    rc = reads_pass(o, ReadsJob{"taxo_classify_reads", kModeTaxon, d_bases, nbytes, flags, max_reads, d_windows, d_result, d_read_starts, false,
                                MatchAux{nullptr, nullptr, taxo_view(o)}}, &res);
    return pass_report(rc, res, info, [&](goss_gpu_taxo_info& i) {
        i.windows = res.sums[0]; i.none = res.counts[0]; i.many = res.counts[1]; i.unannotated = res.sums[3];
    });
}

int goss_gpu_object_taxo_annotate_host(goss_gpu_object* o, const void* bases, uint64_t nbytes, const uint32_t* read_nodes, uint32_t flags,
                                       uint64_t max_reads, uint32_t* windows, goss_gpu_taxo_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    if (!read_nodes && max_reads && nbytes) { o->last_error = "taxo_annotate: no node ids for the reads"; return GOSS_ERR_INVALID_ARG; }
    // (the node ids are the batch's extra array)
    return reads_staged(o, bases, nbytes, max_reads, windows, nullptr, nullptr, read_nodes, info, [&](const StagedBatch& s, goss_gpu_taxo_info* mine) {
        return goss_gpu_object_taxo_annotate(o, s.bases, nbytes, s.extra, flags, max_reads, s.a, mine);
    });
}

int goss_gpu_object_taxo_classify_reads_host(goss_gpu_object* o, const void* bases, uint64_t nbytes, uint32_t flags, uint64_t max_reads,
                                             uint32_t* result, uint32_t* windows, uint64_t* read_starts, goss_gpu_taxo_info* info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!o || (!bases && nbytes)) return GOSS_ERR_INVALID_ARG;
    return reads_staged(o, bases, nbytes, max_reads, windows, result, read_starts, nullptr, info, [&](const StagedBatch& s, goss_gpu_taxo_info* mine) {
        return goss_gpu_object_taxo_classify_reads(o, s.bases, nbytes, flags, max_reads, s.b, s.a, s.starts, mine);
    });
}

int goss_gpu_object_taxo_pair(goss_gpu_object* o, const uint32_t* d_a, const uint32_t* d_b, uint64_t n, uint32_t* d_out)
{
    if (!o || (n && (!d_a || !d_b || !d_out))) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "taxo_pair needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (!o->taxo_n) { o->last_error = "taxo_pair: no tree (goss_gpu_object_taxo_tree_host)"; return GOSS_ERR_STATE; }
    if (!n) return GOSS_OK;
    return obj_guarded(o->device, o->last_error, [&]() { taxo_pair(o, d_a, d_b, n, d_out); });
}

int goss_gpu_object_taxo_tally(goss_gpu_object* o, const uint32_t* d_values, uint64_t n, uint64_t* counts)
{
    if (!o || !counts || (n && !d_values)) return GOSS_ERR_INVALID_ARG;
    if (o->kind != GOSS_OBJECT_KMER_SET) { o->last_error = "taxo_tally needs a KmerSet"; return GOSS_ERR_INVALID_ARG; }
    if (!o->taxo_n) { o->last_error = "taxo_tally: no tree (goss_gpu_object_taxo_tree_host)"; return GOSS_ERR_STATE; }
    return obj_guarded(o->device, o->last_error, [&]() {
        uint32_t* cls = (uint32_t*)o->taxo_scratch.room(n * 4 + 256);
        taxo_dense(o, "taxo_tally", "value", d_values, n, kTaxoAllowNone | kTaxoAllowMany, cls);
        taxo_tally(o, cls, n);
        taxo_bins_out(o, counts);
        check_launch("taxo_tally");
    });
}

int goss_gpu_object_taxo_pair_host(goss_gpu_object* o, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out)
{
    if (!o || (n && (!a || !b || !out))) return GOSS_ERR_INVALID_ARG;
    return taxo_staged(o, {a, b}, n, out, [&](uint32_t* da, uint32_t* db, uint32_t* dout) { return goss_gpu_object_taxo_pair(o, da, db, n, dout); });
}

int goss_gpu_object_taxo_tally_host(goss_gpu_object* o, const uint32_t* values, uint64_t n, uint64_t* counts)
{
    if (!o || !counts || (n && !values)) return GOSS_ERR_INVALID_ARG;
    return taxo_staged(o, {values}, n, nullptr, [&](uint32_t* dv, uint32_t*, uint32_t*) { return goss_gpu_object_taxo_tally(o, dv, n, counts); });
}

}  // extern "C"
