// GossHost.hpp -- host-side C++ for the `goss` commands: errors, logger, input files, the three
// read parsers, and the command classes that mirror the reference's operator interface
// (GossCmdBuildKmerSet.hh:25-38, GossCmdBuildGraph.hh:23-29).  GossHost.cpp holds the files, the
// parsers, the parallel FASTQ framer and the build commands; the command line -- option parser,
// checker, the table of commands and its driver -- is GossCli.cpp.
//
// The parsers frame records exactly like the reference (FastqParser.hh:78-176,
// FastaParser.hh:51-87, LineParser.hh:71-82 over PlainLineSource, LineSource.cc:17-48) but
// emit only what the device needs: the read's bases followed by '\n', appended to a batch
// buffer that is handed to libgossgpu.so (include/goss_gpu.h).
#pragma once

#include <cstdint>
#include <cstdio>
#include <ctime>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct goss_gpu_ctx;

namespace gosshost {

// ---- errors (role of Gossamer::error + boost::error_info tags, GossamerException.hh:27-40) ----
struct Error {
    std::string general;       // general_error_info
    std::string usage;         // usage_info
    std::string parse;         // parse_error_info
    std::string file;          // errinfo_file_name
    std::string write_name;    // write_error_info
    std::string cmd;           // cmd_name_info
    int err_no = 0;            // errinfo_errno

    static Error General(const std::string& m) { Error e; e.general = m; return e; }
    static Error Usage(const std::string& m) { Error e; e.usage = m; return e; }
    static Error Parse(const std::string& file, const std::string& m) { Error e; e.file = file; e.parse = m; return e; }
    static Error Write(const std::string& name) { Error e; e.write_name = name; return e; }
    static Error Errno(const std::string& file, int eno) { Error e; e.file = file; e.err_no = eno; return e; }
};

// ---- logger (Logger.hh:62-96: "<asctime>\t<severity>\t<message>") ----
enum Severity { info = 0, warning = 1, error = 2 };

class Logger {
public:
    Logger(FILE* out, Severity sev, bool owns = false) : mOut(out), mSev(sev), mOwns(owns) {}
    ~Logger() { if (mOwns && mOut) fclose(mOut); }
    void operator()(Severity sev, const std::string& msg)
    {
        if (mSev > sev) return;
        time_t rt; time(&rt);
        std::string now = asctime(localtime(&rt));
        now.erase(now.size() - 1);
        static const char* names[] = {"info", "warning", "error"};
        fprintf(mOut, "%s\t%s\t%s\n", now.c_str(), names[sev], msg.c_str());
        fflush(mOut);
    }
    Severity sev() const { return mSev; }
private:
    FILE* mOut; Severity mSev; bool mOwns;
};

// ---- input files: plain, .gz (zlib), "-" = stdin (PhysicalFileFactory.cc:262-298) ----
class InFile {
public:
    explicit InFile(const std::string& name);      // throws Error
    ~InFile();
    // read up to cap bytes; 0 at end of file
    size_t read(char* dst, size_t cap);
    const std::string& name() const { return mName; }
    static bool readable(const std::string& name);
private:
    std::string mName;
    void* mGz = nullptr;
    void* mBz = nullptr;            // BZFILE* of the stream being read (libbz2, loaded at run time)
    void* mBzFile = nullptr;        // FILE* under it
    bool mBzEnd = false;
    unsigned mBzStreams = 0;        // complete streams decoded so far
    bool mBzFresh = true;           // nothing decoded from the current stream yet
    int mFd = -1;
    bool mStdin = false;
};

// ---- line source: std::getline semantics over a large refillable buffer ----
class LineReader {
public:
    explicit LineReader(const std::string& name, size_t bufBytes = 16u << 20);
    // PlainLineSource::valid(): stream good, or a non-empty last line without '\n'
    bool valid() const { return mGood || mLen; }
    const char* line() const { return mLine; }
    size_t len() const { return mLen; }
    void next();                                  // operator++
    const std::string& name() const { return mFile.name(); }
    uint64_t offset() const { return 0; }         // streams have no record-boundary limit
    static constexpr bool kStableLines = false;   // line() is only valid until next()
private:
    void getline();
    bool refill();
    InFile mFile;
    std::vector<char> mBuf;
    size_t mBeg = 0, mEnd = 0;
    bool mEof = false, mGood = true;
    const char* mLine = nullptr;
    size_t mLen = 0;
    std::string mSpill;                           // a line that straddled a refill
};

// A sink for reads: called with the bases of one read (no terminator).
using ReadSink = std::function<void(const char* seq, size_t len)>;

// Parse a whole file; every read goes to `sink`.  Returns the number of reads.
uint64_t parseFastq(const std::string& name, const ReadSink& sink);
uint64_t parseFasta(const std::string& name, const ReadSink& sink);
uint64_t parseLines(const std::string& name, const ReadSink& sink);

// One goss_gpu_ctx lent from step to step of one process (`xenome index`: two builds, the merge, the gray set; DESIGN.md
// section 4o).  A command that finds one in its GossCmdContext takes its context from it (GpuCtx::open) -- created by
// the first step, on its (device, k, mode), with an arena of arenaBytes, and returned to a clean state with
// goss_gpu_reset for every later step of the same (device, k, mode) -- and leaves it there when it ends; the holder
// destroys it.  Without a holder, which is every goss command, a command creates and destroys its own as ever.
struct SharedContext {
    goss_gpu_ctx* h = nullptr;
    int device = 0;
    uint64_t k = 0;
    int mode = 0;
    uint64_t arenaBytes = 0;        // what the first step maps (0: what that step would map alone); --hbm-budget wins
    SharedContext() = default;
    SharedContext(const SharedContext&) = delete;
    SharedContext& operator=(const SharedContext&) = delete;
    ~SharedContext();
};

// The arena of a shared context, sized once for the largest step of a pipeline over `inputBases` bases of sequence (the
// one definition: DESIGN.md section 4o).
uint64_t sharedArenaBytes(uint64_t inputBases);

// ---- command context (GossCmdContext.hh:25-39, minus the FileFactory: files are real) ----
struct GossCmdContext {
    Logger& log;
    std::string cmdName;
    int device = 0;                 // HIP device ordinal
    std::vector<int> devices = {};  // --devices a,b,..: the build commands count on all of them (one context each)
    uint64_t hbmBudget = 0;         // bytes; 0 = library default (80% of free HBM)
    size_t batchBytes = 256u << 20; // bases handed to the device per push
    // --tmp-dir (App.cc:233-240, PhysicalFileFactory::tmpName): where temporary files go.  Given: the partial results of a
    // merge with more inputs than --max-merge are written there as runs and removed by the command (the reference's
    // temporary objects, GossCmdMerge.tcc:176-208); not given: they stay in host memory.  The build commands need no
    // temporary file: the runs of their chunks are held in HBM.
    std::string tmpDir = {};
    // set by a command that runs several commands in its process: they share one goss_gpu_ctx (SharedContext)
    std::shared_ptr<SharedContext> gpu = {};
};

// A command's counting context: its own, destroyed with it, or the one GossCmdContext::gpu lends, which stays.
struct GpuCtx {
    goss_gpu_ctx* h = nullptr;
    bool lent = false;
    GpuCtx() = default;
    GpuCtx(const GpuCtx&) = delete;
    GpuCtx& operator=(const GpuCtx&) = delete;
    ~GpuCtx();
    void check(int rc, const char* what);       // throws Error::General with the library's text
    // goss_gpu_create(device, K, mode, budget), or the shared context after goss_gpu_reset; under -v the log says
    // which, once: "GPU context created ..." or "GPU context reused ..." (quiet: the caller logs `said` itself -- the
    // build opens its contexts on a thread beside the parser, and the logger is the command's thread's)
    void open(const GossCmdContext& cxt, int device, uint64_t K, int mode, uint64_t budget, bool quiet = false);
    std::string said;
};

typedef std::vector<std::string> strings;

struct BuildStats { uint64_t reads = 0, windows = 0, keys = 0, distinct = 0; double seconds = 0; };

// Same constructor arguments as the reference (K, S, N, T, out, fastas, fastqs, lines).
// S and N size the reference's BackyardHash, whose layout never reaches disk: they are
// accepted and ignored.  T = host parser threads.
class GossCmdBuildKmerSet {
public:
    GossCmdBuildKmerSet(const uint64_t& pK, const uint64_t& pS, const uint64_t& pN, const uint64_t& pT,
                        const std::string& pKmerSetName, const strings& pFastaNames,
                        const strings& pFastqNames, const strings& pLineNames)
        : mK(pK), mS(pS), mN(pN), mT(pT), mKmerSetName(pKmerSetName),
          mFastaNames(pFastaNames), mFastqNames(pFastqNames), mLineNames(pLineNames) {}
    void operator()(const GossCmdContext& pCxt);
    const BuildStats& stats() const { return mStats; }
private:
    const uint64_t mK, mS, mN, mT;
    const std::string mKmerSetName;
    const strings mFastaNames, mFastqNames, mLineNames;
    BuildStats mStats;
};

class GossCmdBuildGraph {
public:
    GossCmdBuildGraph(const uint64_t& pK, const uint64_t& pS, const uint64_t& pN, const uint64_t& pT,
                      const std::string& pGraphName, const strings& pFastaNames,
                      const strings& pFastqNames, const strings& pLineNames)
        : mK(pK), mS(pS), mN(pN), mT(pT), mGraphName(pGraphName),
          mFastaNames(pFastaNames), mFastqNames(pFastqNames), mLineNames(pLineNames) {}
    void operator()(const GossCmdContext& pCxt);
    const BuildStats& stats() const { return mStats; }
private:
    const uint64_t mK, mS, mN, mT;
    const std::string mGraphName;
    const strings mFastaNames, mFastqNames, mLineNames;
    BuildStats mStats;
};

// merge-kmer-sets / merge-graphs: GossCmdMerge<T>(ins, maxMerge, out) (GossCmdMerge.hh:22-37).
class GossCmdMergeKmerSets {
public:
    GossCmdMergeKmerSets(const strings& pIns, const uint64_t& pMaxMerge, const std::string& pOut)
        : mIns(pIns), mMaxMerge(pMaxMerge), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const strings mIns; const uint64_t mMaxMerge; const std::string mOut;
};

class GossCmdMergeGraphs {
public:
    GossCmdMergeGraphs(const strings& pIns, const uint64_t& pMaxMerge, const std::string& pOut)
        : mIns(pIns), mMaxMerge(pMaxMerge), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const strings mIns; const uint64_t mMaxMerge; const std::string mOut;
};

// Set algebra on existing k-mer sets: GossCmdIntersectKmerSets.hh:23, GossCmdSubtractKmerSet.hh:23,
// GossCmdMergeAndAnnotateKmerSets.hh:21 (same constructor arguments).
class GossCmdIntersectKmerSets {
public:
    GossCmdIntersectKmerSets(const strings& pIns, const std::string& pOut) : mIns(pIns), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const strings mIns; const std::string mOut;
};

class GossCmdSubtractKmerSet {
public:
    GossCmdSubtractKmerSet(const strings& pIns, const std::string& pOut) : mIns(pIns), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const strings mIns; const std::string mOut;
};

// GossCmdGraphToKmerSet (GossCmdGraphToKmerSet.{hh,cc}): the normal-form edges of a graph as a
// k-mer set of k = K + 1.
class GossCmdGraphToKmerSet {
public:
    GossCmdGraphToKmerSet(const std::string& pIn, const std::string& pOut) : mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut;
};

class GossCmdMergeAndAnnotateKmerSets {
public:
    GossCmdMergeAndAnnotateKmerSets(const std::string& pLhs, const std::string& pRhs, const std::string& pOut)
        : mLhs(pLhs), mRhs(pRhs), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mLhs, mRhs, mOut;
};

// GossCmdPoolSamples (GossCmdPoolSamples.{hh,cc}; same constructor arguments): the samples -- the given k-mer sets, then
// a k-mer set <out>-a<i> per FASTA file, then <out>-q<i> per FASTQ file -- are merged into <out>-union, their membership in
// the union is written as the SparseArray <out>-index (sample i's k-mer of union rank r at position i * z + r), and the
// Jaccard similarity of every pair goes to <out>.sim.  Departures: pOutPrefix is mandatory (without it the reference
// writes under temporary names and to a file called ".sim"); samples of different K are a usage error (the reference
// compares their raw values); pT only reaches the builds of the per-file sets (the pairs are the device's).
class GossCmdPoolSamples {
public:
    GossCmdPoolSamples(const uint64_t& pK, const uint64_t& pS, const uint64_t& pN, const uint64_t& pT, const std::string& pOutPrefix,
                       const strings& pFastaNames, const strings& pFastqNames, const strings& pKmerSets)
        : mK(pK), mS(pS), mN(pN), mT(pT), mOutPrefix(pOutPrefix), mFastaNames(pFastaNames), mFastqNames(pFastqNames), mKmerSets(pKmerSets) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const uint64_t mK, mS, mN, mT;
    const std::string mOutPrefix;
    const strings mFastaNames, mFastqNames, mKmerSets;
};

// GossCmdComputeNearKmers (GossCmdComputeNearKmers.{hh,cc}): rewrites <in>.lhs-bits / <in>.rhs-bits, clearing both bits of
// every k-mer of one side that has a neighbour of the other side in the set -- with the reference's masks (b << j, a shift
// by bits) and its lookup of the neighbour as it is, not normalised, because those decide the files `xenome classify` reads.
// pNumThreads is accepted and unused.
class GossCmdComputeNearKmers {
public:
    GossCmdComputeNearKmers(const std::string& pIn, uint64_t pNumThreads) : mIn(pIn), mNumThreads(pNumThreads) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn; const uint64_t mNumThreads;
};

// Text form and self-check of existing objects: GossCmdDumpKmerSet.hh, GossCmdDumpGraph.hh,
// GossCmdRestoreGraph.hh (in = text file, out = graph), GossCmdLintGraph.hh.  "-" = stdin/stdout.
class GossCmdDumpKmerSet {
public:
    GossCmdDumpKmerSet(const std::string& pIn, const std::string& pOut) : mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut;
};

class GossCmdDumpGraph {
public:
    GossCmdDumpGraph(const std::string& pIn, const std::string& pOut) : mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut;
};

class GossCmdRestoreGraph {
public:
    GossCmdRestoreGraph(const std::string& pIn, const std::string& pOut) : mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut;
};

class GossCmdLintGraph {
public:
    GossCmdLintGraph(const std::string& pIn, bool pDumpProperties) : mIn(pIn), mDumpProperties(pDumpProperties) {}
    void operator()(const GossCmdContext& pCxt);
    uint64_t problems() const { return mProblems; }
private:
    const std::string mIn; const bool mDumpProperties; uint64_t mProblems = 0;
};

// GossCmdTrimGraph (GossCmdTrimGraph.{hh,cc}) with an explicit cutoff: the edges of multiplicity > cutoff.
class GossCmdTrimGraph {
public:
    GossCmdTrimGraph(const std::string& pIn, const std::string& pOut, uint64_t pCutoff) : mIn(pIn), mOut(pOut), mCutoff(pCutoff) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const uint64_t mCutoff;
};

// GossCmdPruneTips (GossCmdPruneTips.{hh,cc}) without its two cutoffs: pIterations rounds of tip removal.
class GossCmdPruneTips {
public:
    GossCmdPruneTips(const std::string& pIn, const std::string& pOut, uint64_t pIterations) : mIn(pIn), mOut(pOut), mIterations(pIterations) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const uint64_t mIterations;
};

// GossCmdTrimPaths (GossCmdTrimPaths.{hh,cc}): short paths that start at a node without incoming edges go.  pC is
// parsed and, as in the reference, decides nothing.
class GossCmdTrimPaths {
public:
    GossCmdTrimPaths(const std::string& pIn, const std::string& pOut, uint32_t pC) : mIn(pIn), mOut(pOut), mC(pC) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const uint32_t mC;
};

// GossCmdClipLinks (GossCmdClipLinks.{hh,cc}): short paths that leave a fork and enter a join as a minor branch go.
class GossCmdClipLinks {
public:
    GossCmdClipLinks(const std::string& pIn, const std::string& pOut) : mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut;
};

// TransCmdTrimRelative (`translucent trim-relative`, TransCmdTrimRelative.cc): at every node with two or more outgoing
// edges, the edges whose multiplicity is below pRelCoverage times the node's sum go, and their reverse complements
// with them.  Departures: an empty graph gives the empty graph (the reference calls select(0) on it); pNumThreads is
// accepted and unused (the reference's result does not depend on it); asymmetric graphs are refused; a non-finite
// pRelCoverage never reaches the command (the factory refuses it).
class TransCmdTrimRelative {
public:
    TransCmdTrimRelative(const std::string& pIn, const std::string& pOut, double pRelCoverage, uint64_t pNumThreads)
        : mIn(pIn), mOut(pOut), mRelCoverage(pRelCoverage), mNumThreads(pNumThreads) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const double mRelCoverage; const uint64_t mNumThreads;
};

// TransCmdMergeGraphWithReference (`translucent merge-graph-with-reference`, TransCmdMergeGraphWithReference.cc): the
// edges of pIn that pReference holds too, each with pReference's multiplicity, built with pIn's edge count as the
// size estimate as the reference builds them.  Asymmetric graphs are refused.
class TransCmdMergeGraphWithReference {
public:
    TransCmdMergeGraphWithReference(const std::string& pReference, const std::string& pIn, const std::string& pOut)
        : mReference(pReference), mIn(pIn), mOut(pOut) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mReference, mIn, mOut;
};

// GossCmdPrintContigs (GossCmdPrintContigs.{hh,cc}) in its linear-segments form: the non-branching paths of a graph
// as FASTA (or, with pOmitSequence, as a table of their figures).  Supergraph contigs are not part of this build.
class GossCmdPrintContigs {
public:
    GossCmdPrintContigs(const std::string& pIn, uint64_t pC, uint64_t pL, bool pOmitSequence, bool pVerboseHeaders,
                        bool pNoLineBreaks, const std::string& pOut)
        : mIn(pIn), mOut(pOut), mC(pC), mL(pL), mOmitSequence(pOmitSequence), mVerboseHeaders(pVerboseHeaders),
          mNoLineBreaks(pNoLineBreaks) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const uint64_t mC, mL; const bool mOmitSequence, mVerboseHeaders, mNoLineBreaks;
};

// GossCmdBuildEntryEdgeSet (GossCmdBuildEntryEdgeSet.{hh,cc}): the EntryEdgeSet of a graph, written beside it as
// <graph>-entries.*.
class GossCmdBuildEntryEdgeSet {
public:
    explicit GossCmdBuildEntryEdgeSet(const std::string& pIn) : mIn(pIn) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn;
};

// GossCmdCountComponents (GossCmdCountComponents.{hh,cc}): the connected components of a graph, or of the edges that
// the forward (K + 1)-windows of the given reads touch, as a table on standard output; with pOut, the component of the
// first row's start edge and its mirror image written as a graph.  Two defects of the reference are kept because they
// decide its output: every row counts its start edge twice, and the component written is the first listed, not the largest.
class GossCmdCountComponents {
public:
    GossCmdCountComponents(const std::string& pIn, const std::string& pOut, const strings& pFastas, const strings& pFastqs, const strings& pLines)
        : mIn(pIn), mOut(pOut), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const strings mFastas, mFastqs, mLines;
};

// GossCmdBuildSubgraph (GossCmdBuildSubgraph.{hh,cc}): the part of a graph within pRadius steps -- nodes, or with
// pLinearPaths linear paths -- of the edges that the (K + 1)-windows of the given reads and their reverse complements
// touch, written as a graph.  pBufferSize is accepted and unused, as in the reference.
class GossCmdBuildSubgraph {
public:
    GossCmdBuildSubgraph(const std::string& pIn, const std::string& pOut, const strings& pFastas, const strings& pFastqs, const strings& pLines,
                         uint64_t pRadius, bool pLinearPaths, uint64_t pBufferSize)
        : mIn(pIn), mOut(pOut), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines), mRadius(pRadius), mLinearPaths(pLinearPaths),
          mBufferSize(pBufferSize) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const strings mFastas, mFastqs, mLines; const uint64_t mRadius; const bool mLinearPaths; const uint64_t mBufferSize;
};

// GossCmdExtractReads (GossCmdExtractReads.{hh,cc}): the reads with at least one (K + 1)-mer that is an edge of the graph, as
// parsed, one per line, in input order (line files, then FASTA, then FASTQ).
class GossCmdExtractReads {
public:
    GossCmdExtractReads(const std::string& pIn, const strings& pFastas, const strings& pFastqs, const strings& pLines, const std::string& pOut)
        : mIn(pIn), mOut(pOut), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mOut; const strings mFastas, mFastqs, mLines;
};

// GossCmdFilterReads (GossCmdFilterReads.{hh,cc}): the reads (or, pPairs, the pairs of reads of files 2i and 2i + 1) go to
// the match file when either strand of one of their K-mers is in the k-mer set, else to the non-match file; with pPairs the
// two mates go to <pre>_1<suf> and <pre>_2<suf> (pairFiles).  pCount and pNumThreads are accepted and unused, as in the
// reference.  Two deliberate departures, both defects there and not behaviour to copy: its unpaired path cuts (K + 1)-windows
// against a K-mer set, keys outside the set's universe (GossCmdFilterReads.cc:48), and its pair path computes the normalised
// k-mer and then looks up the un-normalised one (:142-146); what both evidently intend -- either strand of a K-mer -- is what
// is built.  The reference writes in the order its threads finish; here the order is the input's.  An odd number of files
// with pPairs makes the reference throw the integer 42 (ReadPairSequenceFileSequence.hh:88-91); here it is an error that says so.
class GossCmdFilterReads {
public:
    GossCmdFilterReads(const std::string& pIn, const strings& pFastas, const strings& pFastqs, const strings& pLines, bool pPairs,
                       bool pCount, uint64_t pNumThreads, const std::string& pMatch, const std::string& pNonMatch)
        : mIn(pIn), mMatch(pMatch), mNonMatch(pNonMatch), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines), mPairs(pPairs),
          mCount(pCount), mNumThreads(pNumThreads) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mMatch, mNonMatch; const strings mFastas, mFastqs, mLines; const bool mPairs, mCount; const uint64_t mNumThreads;
};

// GossCmdGroupReads (GossCmdGroupReads.{hh,cc}, what `xenome classify` runs): every read (or, pPairs, every pair of reads
// of files 2i and 2i + 1) gets the 4-bit mask of the classes -- neither side, right only, left only, both: the set's
// .lhs-bits / .rhs-bits -- that its normalised K-mers fall into, and goes to one of [prefix_]{neither, both, ambiguous,
// <lhs name>, <rhs name>}[_1|_2].{txt, fasta, fastq} by that mask; the table of the sixteen masks and the summary go to
// standard output (pDontWriteReads: no file, one line of five percentages).  Only one group of inputs is processed -- the
// line files, else the FASTA files, else the FASTQ files --, as in the reference, which exits after the first group.
// Departures: the output keeps the input's order whatever pPreserveReadOrder says; pMaxMemory is accepted and exactly
// one pass is made (the reference's passes partition the ranks and OR the masks: the same result); pNumThreads is unused;
// pPairs is false when not given (the reference leaves it uninitialised); pair files of unequal length are an error.
class GossCmdGroupReads {
public:
    GossCmdGroupReads(const std::string& pIn, const strings& pFastas, const strings& pFastqs, const strings& pLines, bool pPairs,
                      double pMaxMemory, uint64_t pNumThreads, const std::string& pLhsName, const std::string& pRhsName,
                      const std::string& pPrefix, bool pDontWriteReads, bool pPreserveReadOrder)
        : mIn(pIn), mLhsName(pLhsName), mRhsName(pRhsName), mPrefix(pPrefix), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines),
          mPairs(pPairs), mDontWriteReads(pDontWriteReads), mPreserveReadOrder(pPreserveReadOrder), mMaxMemory(pMaxMemory),
          mNumThreads(pNumThreads) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn, mLhsName, mRhsName, mPrefix; const strings mFastas, mFastqs, mLines;
    const bool mPairs, mDontWriteReads, mPreserveReadOrder; const double mMaxMemory; const uint64_t mNumThreads;
};

// GossCmdAnnotateKmers (GossCmdAnnotateKmers.{hh,cc}): every k-mer of the set gets the lowest common ancestor, in the
// phylogeny pPhylogeny, of the nodes whose FASTA files (pAnnotList: whitespace-separated `file id` pairs, a repeated file
// keeping its last id) hold it; <set>.annotation receives a raw uint32 per rank, 0xFFFFFFFF for a k-mer nothing holds, and
// the phylogeny is written back over pPhylogeny with `count` (ranks whose class is exactly the node) and `total` (the sum
// over its subtree) on every node.  Departures: a node without `node` or `name`, an id that occurs twice, the ids
// 0xFFFFFFFF / 0xFFFFFFFE and an id in the list that the phylogeny lacks are errors raised before any device work (the
// reference throws the integer 42 or walks off its maps); pNumThreads is unused.
class GossCmdAnnotateKmers {
public:
    GossCmdAnnotateKmers(const std::string& pRef, const std::string& pAnnotList, const std::string& pPhylogeny, uint64_t pNumThreads)
        : mRef(pRef), mAnnotList(pAnnotList), mPhylogeny(pPhylogeny), mNumThreads(pNumThreads) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mRef, mAnnotList, mPhylogeny; const uint64_t mNumThreads;
};

// GossCmdClassifyReads (GossCmdClassifyReads.{hh,cc}): every read (or, pPairs, every pair of reads of files 2i and 2i + 1,
// their k-mers pooled) whose k-mers' classes in <set>.annotation lie on one root-to-leaf path of <set>.taxo is counted for
// the deepest of them; standard output gets, in post-order, `sum TAB kind TAB name` for every node whose subtree sum is
// not zero.  Departures: a k-mer whose annotation is 0xFFFFFFFF is ignored as if absent (the reference looks up a parent
// that does not exist); an id in the annotation that the phylogeny lacks is an error naming the id and the rank; a node
// without `node`, `name` or `kind` is an error at load; line, FASTA and FASTQ inputs are all read, in that order;
// pBufferSize and pNumThreads are accepted and unused; pair files of unequal length are an error.
class GossCmdClassifyReads {
public:
    GossCmdClassifyReads(const std::string& pIn, const strings& pFastas, const strings& pFastqs, const strings& pLines, uint64_t pBufferSize,
                         uint64_t pNumThreads, bool pPairs)
        : mIn(pIn), mFastas(pFastas), mFastqs(pFastqs), mLines(pLines), mBufferSize(pBufferSize), mNumThreads(pNumThreads), mPairs(pPairs) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const std::string mIn; const strings mFastas, mFastqs, mLines; const uint64_t mBufferSize, mNumThreads; const bool mPairs;
};

// GossCmdElectReads (`electus classify`, ElectApp.cc:150-701): every read (or, pPairs, every pair of reads of files 2i and
// 2i + 1) is looked up in up to 64 references at once -- a k-mer set built per pRefFastas file, then every pRefIndexes set as
// it is, pooled by GossCmdPoolSamples into a union whose k-mers carry one colour bit per reference; or pPool, what
// pool-samples wrote -- and goes to <pMatch>{.fasta,.fastq,.txt} when at least pRefThreshold references are hit (~0: all of
// them), else to <pNonMatch>...; with pPairs the mates go to ..._1 / ..._2 before the suffix.  A prefix that is empty
// writes nothing.  The pair rule compares the second mate's word as a number, as the reference does (ElectApp.cc:443).
// Departures: the output keeps the input's order whatever pPreserveReadOrder says; pMaxMemory and pNumThreads are
// accepted and unused (pNumThreads reaches the builds of the per-file sets); more than 64 references and a reference
// index whose K differs are usage errors; pair files of unequal length are an error naming both.
class GossCmdElectReads {
public:
    GossCmdElectReads(uint64_t pK, uint64_t pRefThreshold, const strings& pRefFastas, const strings& pRefIndexes, const std::string& pPool,
                      const strings& pFastas, const strings& pFastqs, const strings& pLines, bool pPairs, double pMaxMemory,
                      uint64_t pNumThreads, const std::string& pMatch, const std::string& pNonMatch, bool pPreserveReadOrder)
        : mK(pK), mRefThreshold(pRefThreshold), mRefFastas(pRefFastas), mRefIndexes(pRefIndexes), mPool(pPool), mFastas(pFastas),
          mFastqs(pFastqs), mLines(pLines), mPairs(pPairs), mMaxMemory(pMaxMemory), mNumThreads(pNumThreads), mMatch(pMatch),
          mNonMatch(pNonMatch), mPreserveReadOrder(pPreserveReadOrder) {}
    void operator()(const GossCmdContext& pCxt);
private:
    const uint64_t mK, mRefThreshold; const strings mRefFastas, mRefIndexes; const std::string mPool; const strings mFastas, mFastqs, mLines;
    const bool mPairs; const double mMaxMemory; const uint64_t mNumThreads; const std::string mMatch, mNonMatch; const bool mPreserveReadOrder;
};

// the decision of elect-reads (KmerFilter, ElectApp.cc:406-451) from a read's word and window count, and the name of an
// output file: <prefix>[_1|_2]<suffix>, half = 0 for single reads
bool electSingle(uint64_t word, uint32_t windows, uint64_t threshold);
bool electPair(uint64_t word1, uint32_t windows1, uint64_t word2, uint32_t windows2, uint64_t threshold);
std::string electFileName(const std::string& prefix, int half, const std::string& suffix);

// Bytes of reads in byte form ('\n' after each) handed to the device per batch by the commands that look reads up in a
// graph or k-mer set: GossCmdContext::batchBytes, or GOSS_MATCH_BATCH=<bytes> (tests).
size_t matchBatchBytes(const GossCmdContext& cxt);

// pairFiles (GossCmdFilterReads.cc:164-172): "a.b.fq" -> "a.b_1.fq", "a.b_2.fq"
void pairFiles(const std::string& pBaseName, std::string& pName1, std::string& pName2);

}  // namespace gosshost
struct goss_gpu_ctx;
namespace gosshost {

// Writes every file image of the emitted object to "<out><suffix>" (the write half of the
// reference's FileFactory for KmerSet::Builder / Graph::Builder::end()).
void writeObjectFiles(goss_gpu_ctx* h, const std::string& out);
void writeObjectFiles(const std::vector<goss_gpu_ctx*>& hs, const std::string& out);      // a group after goss_gpu_group_emit

// App::main for the commands of this build (App.cc:176-417): GossCli.cpp, one record per command in its table.
int gossMain(int argc, char* argv[]);
// The same driver under the name `translucent` with the table of TranslucentApp.cc:68-76, less pop-bubbles and assemble.
int translucentMain(int argc, char* argv[]);
// ... under `xenome` (XenoApp.cc:274-276: index, classify, help) and `electus` (ElectApp.cc:802-804: classify, index, help)
int xenomeMain(int argc, char* argv[]);
int electusMain(int argc, char* argv[]);

// What every executable's main is: `appMain` from its arguments to the end of the process.  Every file the command
// wrote is closed when appMain returns; what is left is tearing the device runtime down -- unmapping tens of GB of HBM,
// unlocking the parser's buffers, unloading the code: 0.05 to 0.1 s of a 1.3 s build that the kernel does anyway when
// the process ends, so the process ends with _exit.  GOSS_FULL_EXIT=1, or a tool that is loaded with the process and
// writes its results from an exit handler (rocprofv3, a sanitizer), keeps the orderly exit.
[[noreturn]] void runAndExit(int (*appMain)(int, char*[]), int argc, char* argv[]);

// The body of `goss dump-bases`: the bases of every read of the given files, one read per line, on standard output, in
// the order line, FASTA, FASTQ; T > 1 sends the FASTQ files through the parallel framer.  Throws when there is no read.
void dumpBases(const strings& fastas, const strings& fastqs, const strings& lines, uint64_t T);

// Gives back what the parser parked between files (page-locked buffers; registered slabs are unregistered first): the
// orderly exit's share of the tear-down (`goss` itself ends with _exit once its files are closed).
void releaseKeptBuffers();

}  // namespace gosshost
