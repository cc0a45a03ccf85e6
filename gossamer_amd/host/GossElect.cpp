// GossElect.cpp -- `goss elect-reads` (`electus classify`, ElectApp.cc:150-701): reads against up to 64 references in one
// pass.
//
// The references become one object: a k-mer set per --ref-fasta file (GossCmdBuildKmerSet), then every --ref-index set as it
// is, pooled by GossCmdPoolSamples into <tmp>-union and <tmp>-index; colour bit i is the i-th reference in that order.  The
// union is opened on the device as it lies on disk, the index beside it as a bare SparseArray, and
// goss_gpu_object_colours_from_index makes the word per k-mer there.  With --pool the two are what pool-samples wrote.  The
// temporary objects go under --tmp-dir, or beside the outputs, and are removed once the device holds them.
//
// The reads are parsed in order, batched ('\n' after each), and each batch is answered by
// goss_gpu_object_colour_reads_host: a 64-bit word and a window count per read, exact, from which the decision is made on
// the host (electSingle / electPair) and the reads are written from the host's copy of the batch, in input order.  One
// kind of input after the other -- FASTA, FASTQ, lines --, each to files of its own suffix, as the reference does.
#include <glob.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "../../include/goss_gpu.h"
#include "GossHost.hpp"
#include "GossReads.hpp"

namespace gosshost {

using namespace reads;

bool electSingle(uint64_t word, uint32_t windows, uint64_t threshold)
{
    return windows >= 1 && (uint64_t)__builtin_popcountll(word) >= threshold;
}

// (the second test compares the word itself: ElectApp.cc:443 writes `c >= mRefThreshold` where :415 and :431 write popcnt(c))
bool electPair(uint64_t word1, uint32_t windows1, uint64_t word2, uint32_t windows2, uint64_t threshold)
{
    return electSingle(word1, windows1, threshold) || (windows2 >= 1 && (word1 | word2) >= threshold);
}

std::string electFileName(const std::string& prefix, int half, const std::string& suffix)
{
    return prefix + (half ? "_" + num((uint64_t)half) : std::string()) + suffix;
}

namespace {

// what a read brings back: its word and its number of windows
struct Coloured { uint64_t word; uint32_t windows; };
typedef BasicMatcher<Coloured> ColourMatcher;

// the Answer of a ColourMatcher: a batch through goss_gpu_object_colour_reads_host, by_count summed into byCount[65]
ColourMatcher::Answer colourAnswer(const Object& obj, uint64_t* byCount)
{
    return [&obj, byCount](const char* buf, size_t bytes, uint64_t n, Coloured* out) {
        std::vector<uint64_t> words(n);
        std::vector<uint32_t> windows(n);
        goss_gpu_elect_info info;
        obj.check(goss_gpu_object_colour_reads_host(obj.h, buf, bytes, GOSS_ELECT_NORMALIZE, n, words.data(), windows.data(), nullptr, &info),
                  "looking a batch of reads up");
        if (info.reads == n)
        {
            for (int j = 0; j < 65; ++j) byCount[j] += info.by_count[j];
            for (uint64_t r = 0; r < n; ++r) out[r] = Coloured{words[r], windows[r]};
        }
        return info.reads;
    };
}

// every file "<base>" followed by '.' or '-' and anything: what an object, or a pool, of that name consists of
void removeFilesOf(const std::string& base)
{
    glob_t g{};
    std::string pat;
    for (char c : base) { if (c == '*' || c == '?' || c == '[' || c == '\\') pat += '\\'; pat += c; }
    pat += "[.-]*";
    if (::glob(pat.c_str(), 0, nullptr, &g) == 0)
        for (size_t i = 0; i < g.gl_pathc; ++i) ::unlink(g.gl_pathv[i]);
    globfree(&g);
}

struct TmpObjects {
    std::string base;
    ~TmpObjects() { if (!base.empty()) removeFilesOf(base); }
};

// K of the k-mer set `name` (KmerSet's header: version, K, count)
uint64_t kmerSetK(const std::string& name)
{
    const std::string hn = name + ".header";
    FILE* fp = fopen(hn.c_str(), "rb");
    if (!fp) throw Error::Errno(hn, errno);
    uint64_t h[3] = {0, 0, 0};
    const bool ok = fread(h, 8, 3, fp) == 3;
    fclose(fp);
    if (!ok) throw Error::General("\tunable to open graph '" + name + "'\n");
    if (h[0] != 2011101701ULL) throw Error::General("\ta version mismatch was detected. goss expected 2011101701 but found " + num(h[0]) + ".\n");
    return h[1];
}

std::string dirOf(const std::string& path)
{
    const size_t slash = path.find_last_of('/');
    return slash == std::string::npos ? std::string(".") : slash == 0 ? std::string("/") : path.substr(0, slash);
}

}  // namespace

void GossCmdElectReads::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    const auto t0 = std::chrono::steady_clock::now();
    (void)mMaxMemory; (void)mPreserveReadOrder;

    // the kinds of input in the reference's order (ElectApp.cc:686-699), each with the suffix of its output files
    struct Kind { const strings* files; Format fmt; const char* suffix; };
    const Kind kinds[3] = {{&mFastas, kFasta, ".fasta"}, {&mFastqs, kFastq, ".fastq"}, {&mLines, kLine, ".txt"}};
    if (mPairs)
        for (const Kind& k : kinds)
            if (k.files->size() % 2)
                throw Error::General("elect-reads --pairs: an even number of input files of each kind is required (" + num(k.files->size()) + " given ending in "
                                     + k.suffix + ")\n");

    // the references as one union and its index
    std::string unionName, indexName;
    TmpObjects tmp;
    if (!mPool.empty())
    {
        unionName = mPool + "-union";
        indexName = mPool + "-index";
    }
    else
    {
        for (auto& r : mRefIndexes)
        {
            const uint64_t k = kmerSetK(r);
            if (k != mK) throw Error::Usage("reference index " + r + " has k=" + num(k) + ", but --kmer-size is " + num(mK) + ".\n");
        }
        const std::string dir = !pCxt.tmpDir.empty() ? pCxt.tmpDir : dirOf(!mMatch.empty() ? mMatch : !mNonMatch.empty() ? mNonMatch : std::string("."));
        tmp.base = dir + "/goss-elect-" + num((uint64_t)::getpid());
        // what pool-samples hands its builds for -B 2 (the reference's BackyardHash; accepted and ignored)
        const uint64_t N = (uint64_t)((double)(2ULL << 30) / (1.5 * 4 + 16)), S = (uint64_t)std::log2((double)N);
        strings sets;
        for (size_t i = 0; i < mRefFastas.size(); ++i)
        {
            log(info, "building k-mer set of reference " + mRefFastas[i]);
            const std::string out = tmp.base + "-r" + num(i);
            GossCmdBuildKmerSet cmd(mK, S, N, mNumThreads, out, strings(1, mRefFastas[i]), strings(), strings());
            cmd(pCxt);
            sets.push_back(out);
        }
        for (auto& r : mRefIndexes) sets.push_back(r);
        log(info, "pooling " + num(sets.size()) + " references");
        GossCmdPoolSamples pool(mK, S, N, mNumThreads, tmp.base + "-pool", strings(), strings(), sets);
        pool(pCxt);
        unionName = tmp.base + "-pool-union";
        indexName = tmp.base + "-pool-index";
    }
    Object g;
    g.open(pCxt, unionName, false);
    if (g.desc.K != mK) throw Error::Usage("the pool " + mPool + " has k=" + num(g.desc.K) + ", but --kmer-size is " + num(mK) + ".\n");
    uint32_t nrefs = 0;
    {
        Object index;
        index.openAs(pCxt, indexName, GOSS_OBJECT_SPARSE_ARRAY);
        g.check(goss_gpu_object_colours_from_index(g.h, index.h, &nrefs), "reading the references' index");
    }
    if (!tmp.base.empty()) { removeFilesOf(tmp.base); tmp.base.clear(); }
    const uint64_t threshold = mRefThreshold == ~0ULL ? nrefs : mRefThreshold;
    log(info, num(g.desc.count) + " " + num(mK) + "-mers in " + num(nrefs) + " references; a match needs " + num(threshold));

    log(info, "processing reads");
    const size_t cap = matchBatchBytes(pCxt);
    uint64_t byCount[65] = {};
    uint64_t n = 0, m = 0;
    for (const Kind& k : kinds)
    {
        if (k.files->empty()) continue;
        const int halves = mPairs ? 2 : 1;
        OutFile match[2], nonMatch[2];
        for (int s = 0; s < halves; ++s)
        {
            if (!mMatch.empty()) match[s].open(electFileName(mMatch, mPairs ? s + 1 : 0, k.suffix));
            if (!mNonMatch.empty()) nonMatch[s].open(electFileName(mNonMatch, mPairs ? s + 1 : 0, k.suffix));
        }
        if (!mPairs)
        {
            ColourMatcher batcher(cap, colourAnswer(g, byCount), [&](const char* seq, size_t len, Coloured c) {
                const bool hit = electSingle(c.word, c.windows, threshold);
                ++n;
                if (hit) ++m;
                OutFile& o = hit ? match[0] : nonMatch[0];
                if (o.fp) o.print(seq, len);
            });
            for (auto& f : *k.files) parseItem(Item{f, k.fmt}, [&](const char* seq, size_t len) { batcher.push(seq, len); });
            batcher.flush();
        }
        else
        {
            // as filter-reads --pairs: the word and the windows of every read of both files first, the decision per pair,
            // then both files once more, each read going where its pair belongs
            for (size_t i = 0; i + 1 < k.files->size(); i += 2)
            {
                std::vector<uint64_t> word[2];
                std::vector<uint32_t> win[2];
                for (int s = 0; s < 2; ++s)
                {
                    ColourMatcher batcher(cap, colourAnswer(g, byCount), [&](const char*, size_t, Coloured c) { word[s].push_back(c.word); win[s].push_back(c.windows); });
                    parseItem(Item{(*k.files)[i + s], k.fmt}, [&](const char* seq, size_t len) { batcher.push(seq, len); });
                    batcher.flush();
                }
                if (word[0].size() != word[1].size())
                    throw Error::General("elect-reads --pairs: '" + (*k.files)[i] + "' holds " + num(word[0].size()) + " reads, '" + (*k.files)[i + 1] + "' "
                                         + num(word[1].size()) + "\n");
                std::vector<uint8_t> verdict(word[0].size());
                for (size_t r = 0; r < verdict.size(); ++r)
                {
                    verdict[r] = electPair(word[0][r], win[0][r], word[1][r], win[1][r], threshold);
                    ++n;
                    m += verdict[r];
                }
                for (int s = 0; s < 2; ++s)
                {
                    if (!match[s].fp && !nonMatch[s].fp) continue;
                    uint64_t r = 0;
                    parseItem(Item{(*k.files)[i + s], k.fmt}, [&](const char* seq, size_t len) {
                        if (r >= verdict.size()) throw Error::General("elect-reads --pairs: '" + (*k.files)[i + s] + "' changed while it was read\n");
                        OutFile& o = verdict[r++] ? match[s] : nonMatch[s];
                        if (o.fp) o.print(seq, len);
                    });
                }
            }
        }
        for (int s = 0; s < halves; ++s) { match[s].close(); nonMatch[s].close(); }
    }
    log(info, std::string("matched ") + num(m) + (mPairs ? " pairs, unmatched " : " reads, unmatched ") + num(n - m));
    std::string hist;
    for (int j = 0; j < 65; ++j)
        if (byCount[j]) hist += (hist.empty() ? "" : ", ") + num((uint64_t)j) + ": " + num(byCount[j]);
    log(info, "reads by the number of references hit: " + (hist.empty() ? std::string("none") : hist));
    log(info, "total elapsed time: " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()));
}

}  // namespace gosshost
