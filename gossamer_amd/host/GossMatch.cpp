// GossMatch.cpp -- `goss extract-reads` (GossCmdExtractReads.cc) and `goss filter-reads` (GossCmdFilterReads.cc): the
// reads that share an edge with a graph, or a k-mer with a k-mer set.
//
// The object is opened on the device as it lies on disk (goss_gpu_object_open).  The reads are parsed in order, batched
// ('\n' after each), and each batch is answered by goss_gpu_object_match_reads_host with GOSS_MATCH_ANY; what comes back
// is one word per read, and the reads are written from the host's copy of the batch, in input order.  The object and the
// batching are GossReads.hpp's, shared with GossTaxo.cpp.
//
// `goss group-reads` (GossCmdGroupReads.cc, what `xenome classify` runs) is the same pipeline over
// goss_gpu_object_classify_reads_host: the word per read is then the 4-bit mask of the classes its k-mers fall into, which
// names the file the read goes to.  The reference handles one group of inputs only -- the line files if there are any, else
// the FASTA files, else the FASTQ files -- because it calls exit(0) after the first group that is not empty
// (GossCmdGroupReads.cc:900-1029); that is reproduced here, the later groups are not read.
#include <fcntl.h>
#include <glob.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

#include "../../include/goss_gpu.h"
#include "GossHost.hpp"
#include "GossReads.hpp"

namespace gosshost {

using namespace reads;

size_t matchBatchBytes(const GossCmdContext& cxt)
{
    if (const char* e = std::getenv("GOSS_MATCH_BATCH"))
    {
        char* end = nullptr;
        unsigned long long v = strtoull(e, &end, 10);
        if (end != e && *end == 0 && v > 0) return (size_t)v;
    }
    return cxt.batchBytes;
}

void pairFiles(const std::string& pBaseName, std::string& pName1, std::string& pName2)
{
    // (find_last_of = npos when there is no dot: substr(0, npos) is the whole name, substr(npos) throws in the
    // reference; here such a name gets the numbers at its end)
    const size_t lastDot = pBaseName.find_last_of('.');
    const std::string pre = pBaseName.substr(0, lastDot);
    const std::string suf = lastDot == std::string::npos ? std::string() : pBaseName.substr(lastDot);
    pName1 = pre + "_1" + suf;
    pName2 = pre + "_2" + suf;
}

void GossCmdExtractReads::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    Object g;
    g.open(pCxt, mIn, true);
    if (g.desc.asymmetric) throw Error::General("\tunable to open graph '" + mIn + "'\nAsymmetric graphs not yet handled");
    OutFile out;
    out.open(mOut);
    uint64_t n = 0, m = 0;
    Matcher matcher(g, GOSS_MATCH_ANY, matchBatchBytes(pCxt), [&](const char* seq, size_t len, uint32_t hit) {
        ++n;
        if (hit) { out.print(seq, len); ++m; }
    });
    for (auto& it : itemsOf(mFastas, mFastqs, mLines))
        parseItem(it, [&](const char* seq, size_t len) { matcher.push(seq, len); });
    matcher.flush();
    out.close();
    log(info, "extracted " + num(m) + " reads, out of " + num(n));
}

void GossCmdFilterReads::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<Item> items = itemsOf(mFastas, mFastqs, mLines);
    if (mPairs && items.size() % 2) throw Error::General("filter-reads --pairs: an even number of input files is required (" + num(items.size()) + " given)\n");
    Object g;
    g.open(pCxt, mIn, false);
    const uint32_t flags = GOSS_MATCH_ANY | GOSS_MATCH_NORMALIZE;
    const size_t cap = matchBatchBytes(pCxt);
    log(info, "Filtering reads....");
    uint64_t n = 0, m = 0;
    if (!mPairs)
    {
        OutFile match, nonMatch;
        if (!mMatch.empty()) match.open(mMatch);
        if (!mNonMatch.empty()) nonMatch.open(mNonMatch);
        Matcher matcher(g, flags, cap, [&](const char* seq, size_t len, uint32_t hit) {
            ++n;
            if (hit) ++m;
            OutFile& o = hit ? match : nonMatch;
            if (o.fp) o.print(seq, len);
        });
        for (auto& it : items) parseItem(it, [&](const char* seq, size_t len) { matcher.push(seq, len); });
        matcher.flush();
        match.close();
        nonMatch.close();
    }
    else
    {
        // files 2i and 2i + 1 read in lockstep: the verdict of every read of both files first (one byte per read), then
        // both files once more, each read going where its pair belongs
        OutFile match[2], nonMatch[2];
        std::string a, b;
        if (!mMatch.empty()) { pairFiles(mMatch, a, b); match[0].open(a); match[1].open(b); }
        if (!mNonMatch.empty()) { pairFiles(mNonMatch, a, b); nonMatch[0].open(a); nonMatch[1].open(b); }
        for (size_t i = 0; i + 1 < items.size(); i += 2)
        {
            std::vector<uint8_t> verdict[2];
            for (int s = 0; s < 2; ++s)
            {
                Matcher matcher(g, flags, cap, [&](const char*, size_t, uint32_t hit) { verdict[s].push_back(hit ? 1 : 0); });
                parseItem(items[i + s], [&](const char* seq, size_t len) { matcher.push(seq, len); });
                matcher.flush();
            }
            if (verdict[0].size() != verdict[1].size())
                throw Error::General("filter-reads --pairs: '" + items[i].name + "' holds " + num(verdict[0].size()) + " reads, '" + items[i + 1].name
                                     + "' " + num(verdict[1].size()) + "\n");
            for (size_t r = 0; r < verdict[0].size(); ++r) { verdict[0][r] |= verdict[1][r]; ++n; m += verdict[0][r]; }
            for (int s = 0; s < 2; ++s)
            {
                if (!match[s].fp && !nonMatch[s].fp) continue;
                uint64_t r = 0;
                parseItem(items[i + s], [&](const char* seq, size_t len) {
                    if (r >= verdict[0].size()) throw Error::General("filter-reads --pairs: '" + items[i + s].name + "' changed while it was read\n");
                    OutFile& o = verdict[0][r++] ? match[s] : nonMatch[s];
                    if (o.fp) o.print(seq, len);
                });
            }
        }
        for (int s = 0; s < 2; ++s) { match[s].close(); nonMatch[s].close(); }
    }
    log(info, std::string("matched ") + num(m) + (mPairs ? " pairs, out of " : " reads, out of ") + num(n));
    log(info, "total elapsed time: " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()));
}

namespace {

// classStr (GossCmdGroupReads.cc:488-526)
std::string classStr(const std::string& lhsName, const std::string& rhsName, unsigned i)
{
    switch (i & 7u)
    {
        case 0: return i ? "both" : "neither";
        case 1: return i == 9 ? "probably both" : "both";
        case 2: return "definitely " + rhsName;
        case 3: return "probably " + rhsName;
        case 4: return "definitely " + lhsName;
        case 5: return "probably " + lhsName;
        default: return "ambiguous";
    }
}

// the file of a mask (GossCmdGroupReads.cc:605-620): 0 neither, 1 both, 2 rhs, 3 lhs, 4 ambiguous
unsigned fileOf(unsigned mask)
{
    static const unsigned char kFile[16] = {0, 1, 2, 2, 3, 3, 4, 4, 1, 1, 2, 2, 3, 3, 4, 4};
    return kFile[mask & 15u];
}

// printStats (GossCmdGroupReads.cc:809-854); doubles as a C++ stream prints them by default
void printStats(const uint64_t* counts, bool dontWriteReads, const std::string& lhsName, const std::string& rhsName)
{
    uint64_t total = 0;
    for (unsigned i = 0; i < 16; ++i) total += counts[i];
    uint64_t sums[5] = {0, 0, 0, 0, 0};
    for (unsigned i = 0; i < 16; ++i) sums[fileOf(i)] += counts[i];
    const uint64_t graftC = sums[3], hostC = sums[2], bothC = sums[1], neitherC = sums[0], ambigC = sums[4];
    std::ostringstream out;
    if (dontWriteReads)
    {
        out << 100.0 * graftC / total << '\t' << 100.0 * hostC / total << '\t' << 100.0 * bothC / total << '\t' << 100.0 * neitherC / total << '\t'
            << 100.0 * ambigC / total << '\n';
    }
    else
    {
        out << "Statistics\n";
        out << "B\tG\tH\tM\tcount\tpercent\tclass\n";
        for (unsigned i = 0; i < 16; ++i)
            out << (i & 8 ? '1' : '0') << '\t' << (i & 4 ? '1' : '0') << '\t' << (i & 2 ? '1' : '0') << '\t' << (i & 1 ? '1' : '0') << '\t' << counts[i]
                << '\t' << (100.0 * double(counts[i]) / total) << '\t' << '"' << classStr(lhsName, rhsName, i) << '"' << '\n';
        out << "\nSummary\n";
        out << "count\tpercent\tclass\n";
        out << graftC << '\t' << 100.0 * graftC / total << '\t' << lhsName << '\n';
        out << hostC << '\t' << 100.0 * hostC / total << '\t' << rhsName << '\n';
        out << bothC << '\t' << 100.0 * bothC / total << '\t' << "both" << '\n';
        out << neitherC << '\t' << 100.0 * neitherC / total << '\t' << "neither" << '\n';
        out << ambigC << '\t' << 100.0 * ambigC / total << '\t' << "ambiguous" << '\n';
    }
    const std::string text = out.str();
    if (fwrite(text.data(), 1, text.size(), stdout) != text.size() || fflush(stdout) != 0) throw Error::Write("-");
}

// a whole file of 64-bit words
std::vector<uint64_t> readWords(const std::string& name, uint64_t* bytes)
{
    FILE* fp = fopen(name.c_str(), "rb");
    if (!fp) throw Error::Errno(name, errno);
    std::vector<uint64_t> words;
    *bytes = 0;
    uint64_t buf[8192];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0)
    {
        words.resize((*bytes + got + 7) / 8, 0);
        memcpy((char*)words.data() + *bytes, buf, got);
        *bytes += got;
    }
    const bool bad = ferror(fp) != 0;
    fclose(fp);
    if (bad) throw Error::Errno(name, EIO);
    return words;
}

}  // namespace

void GossCmdGroupReads::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    const auto t0 = std::chrono::steady_clock::now();
    (void)mMaxMemory; (void)mNumThreads; (void)mPreserveReadOrder;

    // the one group of inputs (see the head of this file)
    std::vector<Item> items;
    const char* suffix = "txt";
    if (!mLines.empty()) { for (auto& f : mLines) items.push_back(Item{f, kLine}); }
    else if (!mFastas.empty()) { suffix = "fasta"; for (auto& f : mFastas) items.push_back(Item{f, kFasta}); }
    else if (!mFastqs.empty()) { suffix = "fastq"; for (auto& f : mFastqs) items.push_back(Item{f, kFastq}); }
    if (mPairs && items.size() % 2) throw Error::General("group-reads --pairs: an even number of input files is required (" + num(items.size()) + " given)\n");

    // KmerSet(name, fac).count(), and the two bitmaps as WordyBitVector::Builder leaves them after count bits:
    // (count - 1) / 64 + 1 words, one word for none -- all before any device is asked for
    uint64_t hb = 0;
    const std::vector<uint64_t> hdr = readWords(mIn + ".header", &hb);
    if (hb < 24) throw Error::General("\tunable to open graph '" + mIn + "'\n");
    if (hdr[0] != 2011101701ULL)
        throw Error::General("\ta version mismatch was detected. goss expected 2011101701 but found " + num(hdr[0]) + ".\n");
    const uint64_t count = hdr[2];
    const std::string lname = mIn + ".lhs-bits", rname = mIn + ".rhs-bits";
    uint64_t lb = 0, rb = 0;
    const std::vector<uint64_t> lhs = readWords(lname, &lb), rhs = readWords(rname, &rb);
    const uint64_t nwords = count ? (count - 1) / 64 + 1 : 1;
    for (const auto& f : {std::make_pair(&lname, lb), std::make_pair(&rname, rb)})
        if (f.second != nwords * 8)
            throw Error::General("\tfile '" + *f.first + "' holds " + num(f.second) + " bytes; the " + num(count) + " k-mers of '" + mIn + "' need "
                                 + num(nwords * 8) + "\n");

    Object g;
    g.open(pCxt, mIn, false);
    if (g.desc.count != count) throw Error::General("\tunable to open graph '" + mIn + "'\n\tits header and its k-mers disagree\n");
    g.check(goss_gpu_object_classify_bits_host(g.h, lhs.data(), rhs.data()), "keeping the bitmaps");
    log(info, "performing 1 pass");

    // neither, both, rhs, lhs, ambiguous (fileOf), one per half with pairs
    const std::string cls[5] = {"neither", "both", mRhsName.empty() ? "host" : mRhsName, mLhsName.empty() ? "graft" : mLhsName, "ambiguous"};
    auto filename = [&](unsigned c, int half) {
        std::string n;
        if (!mPrefix.empty()) n = mPrefix + "_";
        n += cls[c];
        if (half) n += "_" + num((uint64_t)half);
        return n + "." + suffix;
    };
    OutFile outs[2][5];
    if (!mDontWriteReads)
    {
        // the order the reference creates and logs them in (GossCmdGroupReads.cc:594-603, 704-723)
        static const unsigned kSingle[5] = {0, 1, 3, 2, 4}, kPaired[5] = {0, 1, 4, 3, 2};
        for (unsigned i = 0; i < 5; ++i)
            for (int s = 0; s < (mPairs ? 2 : 1); ++s)
            {
                const unsigned c = mPairs ? kPaired[i] : kSingle[i];
                const std::string n = filename(c, mPairs ? s + 1 : 0);
                outs[s][c].open(n);
                log(info, "writing to " + n);
            }
    }
    log(info, "pass 0");

    const uint32_t flags = GOSS_CLASSIFY_NORMALIZE;
    const size_t cap = matchBatchBytes(pCxt);
    uint64_t counts[16] = {};
    if (!mPairs)
    {
        Matcher matcher(g, flags, cap, [&](const char* seq, size_t len, uint32_t mask) {
            ++counts[mask & 15u];
            if (!mDontWriteReads) outs[0][fileOf(mask)].print(seq, len);
        }, true);
        for (auto& it : items) parseItem(it, [&](const char* seq, size_t len) { matcher.push(seq, len); });
        matcher.flush();
    }
    else
    {
        // as filter-reads --pairs: the mask of every read of both files first (one byte per read), ORed per pair, then both
        // files once more, each read going where its pair belongs
        for (size_t i = 0; i + 1 < items.size(); i += 2)
        {
            std::vector<uint8_t> mask[2];
            for (int s = 0; s < 2; ++s)
            {
                Matcher matcher(g, flags, cap, [&](const char*, size_t, uint32_t m) { mask[s].push_back((uint8_t)(m & 15u)); }, true);
                parseItem(items[i + s], [&](const char* seq, size_t len) { matcher.push(seq, len); });
                matcher.flush();
            }
            if (mask[0].size() != mask[1].size())
                throw Error::General("group-reads --pairs: '" + items[i].name + "' holds " + num(mask[0].size()) + " reads, '" + items[i + 1].name + "' "
                                     + num(mask[1].size()) + "\n");
            for (size_t r = 0; r < mask[0].size(); ++r) { mask[0][r] |= mask[1][r]; ++counts[mask[0][r]]; }
            if (mDontWriteReads) continue;
            for (int s = 0; s < 2; ++s)
            {
                uint64_t r = 0;
                parseItem(items[i + s], [&](const char* seq, size_t len) {
                    if (r >= mask[0].size()) throw Error::General("group-reads --pairs: '" + items[i + s].name + "' changed while it was read\n");
                    outs[s][fileOf(mask[0][r++])].print(seq, len);
                });
            }
        }
    }
    for (auto& half : outs) for (auto& o : half) o.close();
    printStats(counts, mDontWriteReads, mLhsName, mRhsName);
    log(info, "total elapsed time: " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()));
}

}  // namespace gosshost
