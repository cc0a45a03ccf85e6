// GossReads.hpp -- what the commands that look reads up in an object resident on the device share: the object as it lies
// on disk (Object), the reads in and one word per read out in batches (Matcher), and the input files in the reference's
// order, and the files the reads are written to (OutFile).  Used by GossMatch.cpp (extract-reads, filter-reads,
// group-reads), GossTaxo.cpp (annotate-kmers, classify-reads) and GossElect.cpp (elect-reads).
#pragma once

#include <fcntl.h>
#include <glob.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../include/goss_gpu.h"
#include "GossHost.hpp"

namespace gosshost {
namespace reads {

inline std::string num(uint64_t v) { return std::to_string(v); }

// An object's files, mapped, under the names they have on disk.
struct ObjectFiles {
    std::vector<std::string> names;
    std::vector<std::pair<const void*, size_t>> maps;
    ~ObjectFiles() { for (auto& m : maps) if (m.first && m.second) munmap((void*)m.first, m.second); }
    void add(const std::string& name)
    {
        int fd = ::open(name.c_str(), O_RDONLY);
        if (fd < 0) throw Error::Errno(name, errno);
        struct stat st;
        if (fstat(fd, &st) != 0) { int e = errno; ::close(fd); throw Error::Errno(name, e); }
        const void* p = nullptr;
        if (S_ISREG(st.st_mode) && st.st_size)
        {
            void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { int e = errno; ::close(fd); throw Error::Errno(name, e); }
            p = m;
        }
        ::close(fd);
        if (!S_ISREG(st.st_mode)) return;
        names.push_back(name);
        maps.emplace_back(p, (size_t)st.st_size);
    }
};

struct Object {
    goss_gpu_object* h = nullptr;
    goss_gpu_object_desc desc{};
    ~Object() { if (h) goss_gpu_object_close(h); }
    void check(int rc, const char* what) const
    {
        if (rc == GOSS_OK) return;
        std::string msg = std::string(what) + ": " + goss_gpu_strerror(rc);
        const char* d = goss_gpu_object_last_error(h);
        if (d && *d) msg += std::string(" (") + d + ")";
        throw Error::General(msg + "\n");
    }
    // Graph::open(name, fac) / KmerSet(name, fac): every file "<name>." or "<name>-" something
    void open(const GossCmdContext& cxt, const std::string& name, bool graph) { openAs(cxt, name, graph ? GOSS_OBJECT_GRAPH : GOSS_OBJECT_KMER_SET); }
    // the same for any kind of object (GOSS_OBJECT_*)
    void openAs(const GossCmdContext& cxt, const std::string& name, int kind)
    {
        ObjectFiles files;
        glob_t g{};
        std::string pat;
        for (char c : name) { if (c == '*' || c == '?' || c == '[' || c == '\\') pat += '\\'; pat += c; }
        pat += "[.-]*";
        if (::glob(pat.c_str(), 0, nullptr, &g) == 0)
            for (size_t i = 0; i < g.gl_pathc; ++i)
            {
                const std::string f = g.gl_pathv[i];
                if (f.size() >= 4 && f.compare(f.size() - 4, 4, ".txt") == 0) continue;
                files.add(f);
            }
        globfree(&g);
        std::vector<goss_gpu_named_file> nf(files.names.size());
        for (size_t i = 0; i < nf.size(); ++i) nf[i] = goss_gpu_named_file{files.names[i].c_str(), files.maps[i].first, files.maps[i].second};
        int rc = goss_gpu_object_open(&h, cxt.device, nullptr, kind, name.c_str(), nf.data(), (uint32_t)nf.size());
        if (rc != GOSS_OK)
        {
            std::string msg = "\tunable to open graph '" + name + "'\n\t" + goss_gpu_strerror(rc);
            const char* d = goss_gpu_object_last_error(nullptr);
            if (d && *d) msg += std::string(" (") + d + ")";
            throw Error::General(msg + "\n");
        }
        check(goss_gpu_object_info(h, &desc), "describing the object");
    }
};

// Reads in, one word per read out, in order: batches end at read boundaries and hold `cap` bytes (one read more than
// that is a batch of its own).  The word is what the Answer makes of a read: match_reads' hits (with GOSS_MATCH_ANY 1 / 0),
// pClassify: classify_reads' mask, or whatever a command's own Answer gives.  Word is uint32_t (Matcher) but where a
// command needs more per read: elect-reads' Coloured.
template <class Word>
class BasicMatcher {
public:
    typedef std::function<void(const char* seq, size_t len, Word word)> Verdict;
    // the reads of a batch answered: `bytes` of reads ('\n' after each), n of them, one word each; returns the reads seen
    typedef std::function<uint64_t(const char* buf, size_t bytes, uint64_t n, Word* words)> Answer;
    BasicMatcher(size_t cap, Answer a, Verdict v) : mCap(cap), mAnswer(std::move(a)), mVerdict(std::move(v)) {}
    BasicMatcher(const Object& obj, uint32_t flags, size_t cap, Verdict v, bool pClassify = false)
        : BasicMatcher(cap, pClassify ? classifyAnswer(obj, flags) : matchAnswer(obj, flags), std::move(v)) {}
    static Answer matchAnswer(const Object& obj, uint32_t flags)
    {
        return [&obj, flags](const char* buf, size_t bytes, uint64_t n, uint32_t* words) {
            goss_gpu_match_info info;
            obj.check(goss_gpu_object_match_reads_host(obj.h, buf, bytes, flags, n, nullptr, words, nullptr, &info), "matching a batch of reads");
            return info.reads;
        };
    }
    static Answer classifyAnswer(const Object& obj, uint32_t flags)
    {
        return [&obj, flags](const char* buf, size_t bytes, uint64_t n, uint32_t* words) {
            goss_gpu_classify_info info;
            obj.check(goss_gpu_object_classify_reads_host(obj.h, buf, bytes, flags, n, words, nullptr, nullptr, &info), "classifying a batch of reads");
            return info.reads;
        };
    }
    void push(const char* seq, size_t len)
    {
        if (!mBuf.empty() && mBuf.size() + len + 1 > mCap) flush();
        mStart.push_back(mBuf.size());
        mBuf.insert(mBuf.end(), seq, seq + len);
        mBuf.push_back('\n');
    }
    void flush()
    {
        if (mStart.empty()) return;
        const uint64_t n = mStart.size();
        mHits.resize(n);
        const uint64_t answered = mAnswer(mBuf.data(), mBuf.size(), n, mHits.data());
        if (answered != n) throw Error::General("matching a batch of reads: " + num(n) + " reads sent, " + num(answered) + " answered\n");
        mStart.push_back(mBuf.size());
        for (uint64_t r = 0; r < n; ++r) mVerdict(mBuf.data() + mStart[r], mStart[r + 1] - mStart[r] - 1, mHits[r]);
        mBuf.clear();
        mStart.clear();
        ++mBatches;
    }
    uint64_t batches() const { return mBatches; }
private:
    const size_t mCap;
    Answer mAnswer;
    Verdict mVerdict;
    std::vector<char> mBuf;
    std::vector<uint64_t> mStart;
    std::vector<Word> mHits;
    uint64_t mBatches = 0;
};
typedef BasicMatcher<uint32_t> Matcher;

// FileFactory::out(name): "-" is standard output
struct OutFile {
    std::string name;
    FILE* fp = nullptr;
    std::string pending;
    void open(const std::string& n)
    {
        name = n;
        fp = n == "-" ? stdout : fopen(n.c_str(), "wb");
        if (!fp) throw Error::Errno(n, errno);
    }
    // GossReadBaseString::print (GossReadBaseString.hh:115-118): the bases as parsed, then '\n'
    void print(const char* seq, size_t len)
    {
        pending.append(seq, len);
        pending += '\n';
        if (pending.size() >= (4u << 20)) drain();
    }
    void drain()
    {
        if (!pending.empty() && fwrite(pending.data(), 1, pending.size(), fp) != pending.size()) throw Error::Write(name);
        pending.clear();
    }
    void close()
    {
        if (!fp) return;
        drain();
        if (fp == stdout) fflush(stdout);
        else if (fclose(fp) != 0) { fp = nullptr; throw Error::Write(name); }
        fp = nullptr;
    }
    ~OutFile() { if (fp && fp != stdout) fclose(fp); }
};

enum Format { kLine, kFasta, kFastq };
struct Item { std::string name; Format fmt; };

// the reference's item order: all line files, then all FASTA files, then all FASTQ files
// (GossCmdExtractReads.cc:64-88, GossCmdFilterReads.cc:186-212)
inline std::vector<Item> itemsOf(const strings& fastas, const strings& fastqs, const strings& lines)
{
    std::vector<Item> items;
    for (auto& f : lines) items.push_back(Item{f, kLine});
    for (auto& f : fastas) items.push_back(Item{f, kFasta});
    for (auto& f : fastqs) items.push_back(Item{f, kFastq});
    return items;
}

inline uint64_t parseItem(const Item& it, const ReadSink& sink)
{
    return it.fmt == kLine ? parseLines(it.name, sink) : it.fmt == kFasta ? parseFasta(it.name, sink) : parseFastq(it.name, sink);
}

}  // namespace reads
}  // namespace gosshost
