// goss_read_src.hpp -- what a count reads its windows from, as one value: ASCII bases in HBM, a packed string (2-bit
// codes + non-base flags, sixteen positions a group) or super-k-mer records.  Plain host C++: a host compiler can
// include this header by itself (tests/read_src_check.cpp does); goss_gpu.hip passes a ReadSrc by value from the entry
// points down to the launch sites, which ask it for the kernels' arguments.
#pragma once
#include <cstdint>

namespace goss {

struct ReadSrc {
    enum Kind { Bytes, Packed, Records };
    Kind kind = Bytes;
    const uint8_t* bytes = nullptr;          // Bytes: the string; Records: the first record
    const uint32_t* codes = nullptr;         // Packed: group 0 of the string, its codes ...
    const uint16_t* bad = nullptr;           // ... and its flags
    uint64_t pos = 0;                        // Packed: position of the first base within the two arrays
    uint32_t rec_bytes = 0;                  // Records: bytes of one record (12 or 20)

    static constexpr uint64_t kRecSlots = 16;          // window slots of a record: n records count as 16 n window starts

    static ReadSrc of_bytes(const void* p) { ReadSrc s; s.kind = Bytes; s.bytes = (const uint8_t*)p; return s; }
    static ReadSrc of_packed(const uint32_t* codes, const uint16_t* bad, uint64_t pos = 0)
    {
        ReadSrc s; s.kind = Packed; s.codes = codes; s.bad = bad; s.pos = pos; return s;
    }
    static ReadSrc of_records(const void* first, uint32_t rec_bytes)
    {
        ReadSrc s; s.kind = Records; s.bytes = (const uint8_t*)first; s.rec_bytes = rec_bytes; return s;
    }
    bool packed() const { return kind == Packed; }
    bool records() const { return kind == Records; }

    // the source of a later chunk, `starts` window starts on (records: a multiple of 16, whole records)
    ReadSrc advance(uint64_t starts) const
    {
        ReadSrc s = *this;
        if (kind == Packed) s.pos += starts;
        else if (kind == Records) s.bytes += starts / kRecSlots * rec_bytes;
        else s.bytes += starts;
        return s;
    }

    // What a kernel that reads the source is handed: `base` is the 16-byte-aligned address the first byte lies at or
    // behind (Bytes), the codes of the group the first position lies in (Packed; `bad` that group's flags) or the first
    // record; `mis` the first byte's / position's place within its sixteen -- 0 for records, which are read where they lie.
    struct Launch { Kind kind; const uint8_t* base; uint32_t mis; const uint16_t* bad; };
    Launch launch() const
    {
        if (kind == Packed) return {kind, (const uint8_t*)(codes + (pos >> 4)), (uint32_t)(pos & 15u), bad + (pos >> 4)};
        if (kind == Records) return {kind, bytes, 0u, nullptr};
        const uintptr_t addr = (uintptr_t)bytes;
        const uint32_t mis = (uint32_t)(addr & 15u);
        return {kind, (const uint8_t*)(addr - mis), mis, nullptr};
    }
    // bytes / positions from the first one to the next that begins a sixteen (0 when it does itself)
    uint64_t to_next16() const { return (16u - launch().mis) & 15u; }
};

}  // namespace goss
