// GossCli.cpp -- the goss command line (App.cc:176-417, GossApp.cc:145-202, GossOptionChecker.hh): the option parser,
// the checker, one `create` function per command in the manner of the reference's GossCmdFactory...::create, the table
// of commands (kCommands) and the one driver that takes a command from its arguments to its run.  A new command is one
// record in kCommands and its create function.  The driver takes the executable (App: its name and its table) as a
// parameter: `translucent` (TranslucentApp.cc) is the same driver over four of goss's records and two of its own,
// `xenome` (XenoApp.cc) and `electus` (ElectApp.cc) over two records each.  runAndExit is every executable's main.
#include "GossHost.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>

#include "../../include/goss_gpu.h"

namespace gosshost {
namespace {

std::string num(uint64_t v) { return std::to_string(v); }

enum OptKind { kFlag, kU64, kString, kStrings };
struct OptDef { const char* lng; const char* sht; OptKind kind; const char* help; };
struct OptGroup { const OptDef* defs; size_t n; };
template <size_t N> constexpr OptGroup group(const OptDef (&a)[N]) { return OptGroup{a, N}; }

// every command's table is kGlobal, its own groups in its own order, kGpuSpecific: -h prints it in that order and the
// unique-prefix guessing depends on what it holds
const OptDef kGlobal[] = {
    {"debug", "D", kStrings, "enable particular debugging output"},
    {"help", "h", kFlag, "show a help message"},
    {"log-file", "l", kString, "place to write messages"},
    {"tmp-dir", "", kStrings, "a directory to use for temporary files (default /tmp)"},
    {"num-threads", "T", kU64, "maximum number of worker threads to use, where possible"},
    {"verbose", "v", kFlag, "show progress messages"},
    {"version", "V", kFlag, "show the software version"},
};
// not in the reference: where and how much HBM to use
const OptDef kGpuSpecific[] = {
    {"device", "", kU64, "HIP device ordinal (default 0)"},
    {"devices", "", kString, "build commands: comma-separated HIP device ordinals to count on side by side (one context each)"},
    {"hbm-budget", "", kU64, "HBM budget in GB for keys and sort workspace (default: 80% of free HBM)"},
};
// the common options of the build commands: kBufferSize, kReadLists, kLineIn, kOutAndK
const OptDef kBufferSize[] = {
    {"buffer-size", "B", kU64, "maximum size (in GB) for in-memory buffers (default: 2)"},
};
const OptDef kReadLists[] = {
    {"fasta-in", "I", kStrings, "input file in FASTA format"},
    {"fastas-in", "F", kStrings, "input file containing filenames in FASTA format"},
    {"fastq-in", "i", kStrings, "input file in FASTQ format"},
    {"fastqs-in", "f", kStrings, "input file containing filenames in FASTQ format"},
};
const OptDef kLineIn[] = {
    {"line-in", "", kStrings, "input file with one sequence per line"},
};
const OptDef kOutAndK[] = {
    {"graph-out", "O", kString, "name of the output graph object"},
    {"kmer-size", "k", kU64, "kmer size to use"},
};
const OptDef kKmerSetSpecific[] = {
    {"log-hash-slots", "S", kU64, "log2 of the number of hash slots to use (default 24)"},
};
const OptDef kGraphIn[] = {
    {"graph-in", "G", kStrings, "name of the input graph object"},
};
const OptDef kGraphOut[] = {
    {"graph-out", "O", kString, "name of the output graph object"},
};
const OptDef kReadsIn[] = {
    {"fasta-in", "I", kStrings, "input file in FASTA format"},
    {"fastq-in", "i", kStrings, "input file in FASTQ format"},
    {"line-in", "", kStrings, "input file with one sequence per line"},
};
const OptDef kPairs[] = {
    {"pairs", "", kFlag, "treat reads as pairs"},
};
const OptDef kReadOrder[] = {
    {"dont-write-reads", "", kFlag, "do not produce any output read files"},
    {"preserve-read-order", "", kFlag, "maintain the same relative ordering of reads in output files"},
};
// the file family: the commands that take existing objects to a new object or a text
const OptDef kMerge[] = {
    {"graph-in", "G", kStrings, "name of the input graph object"},
    {"graphs-in", "", kStrings, "read graph names (one per line) from the given file."},
    {"graph-out", "O", kString, "name of the output graph object"},
    {"max-merge", "", kU64, "The maximum number of graphs to merge at once."},
    {"input-file", "f", kString, "input file name ('-' for standard input)"},
    {"output-file", "o", kString, "output file name ('-' for standard output)"},
    {"dump-properties", "", kFlag, "show the internal properties of the graph"},
};
const OptDef kCutoff[] = {
    {"cutoff", "C", kU64, "coverage cutoff"},
};
const OptDef kTrimPrune[] = {
    {"estimate-only", "", kFlag, "only estimate the coverage cutoff (trim-graph)"},
    {"scale-cutoff-by-k", "", kU64, "scale the coverage cutoff by k-mer size"},
    {"relative-cutoff", "", kString, "relative coverage cutoff"},
    {"iterate", "", kU64, "number of passes to perform"},
};
// GossCmdFactoryPrintContigs (GossCmdPrintContigs.cc:226-289).  The reference registers
// include-entailed-contigs and reads print-entailed-contigs (:260, :285); both belong to the supergraph form
const OptDef kContigs[] = {
    {"min-length", "", kU64, "minimum length of a printed sequence"},
    {"min-coverage", "", kU64, "minimum coverage"},
    {"no-sequence", "", kFlag, "print a table of the segments' figures instead of their sequence"},
    {"print-linear-segments", "", kFlag, "Only print individual linear paths, even if a supergraph is present."},
    {"verbose-headers", "", kFlag, "Print additional information in contig headers"},
    {"no-line-breaks", "", kFlag, "Print contig sequences without line breaks"},
    {"include-entailed-contigs", "", kFlag, "not offered (supergraph contigs)"},
    {"print-entailed-contigs", "", kFlag, "not offered (supergraph contigs)"},
    {"print-rcs", "", kFlag, "Include each sequence's reverse complement."},
};
const OptDef kPool[] = {
    {"kmer-set-in", "", kStrings, "input k-mer set"},
    {"kmer-sets-in", "", kStrings, "input file containing k-mer sets"},
};
const OptDef kSubgraph[] = {
    {"radius", "", kU64, "distance of the furthest node to include from any source"},
    {"linear-paths", "", kFlag, "interpret radius in terms of linear paths, not nodes"},
};
const OptDef kExtract[] = {
    {"output-file", "o", kString, "output file name ('-' for standard output)"},
};
const OptDef kFilter[] = {
    {"match-file", "", kString, "a file to put matching reads into"},
    {"non-match-file", "", kString, "a file to put non-matching reads into"},
    {"pairs", "", kFlag, "treat reads as pairs"},
    {"count", "", kFlag, "generate histogram of matching kmers per read"},
};
const OptDef kGroupMemory[] = {
    {"max-memory", "M", kString, "maximum memory (in GB) to use (default: unlimited)"},
};
const OptDef kGroupNames[] = {
    {"lhs-name", "", kString, "name for left-hand side reads"},
    {"rhs-name", "", kString, "name for right-hand side reads"},
    {"output-filename-prefix", "", kString, "prefix for output files"},
};
// electus' own option names (ElectApp.cc:806-820)
const OptDef kElectRefs[] = {
    {"ref-fasta", "", kStrings, "reference file in FASTA format"},
    {"ref-index", "", kStrings, "prefix of reference index"},
    {"pool", "", kString, "prefix of a pool written by pool-samples, used as the references"},
};
const OptDef kElectSizes[] = {
    {"max-memory", "M", kString, "maximum memory (in GB) to use"},
    {"kmer-size", "K", kU64, "kmer size to use (default 25)"},
};
const OptDef kElectOut[] = {
    {"ref-threshold", "", kU64, "the minimum number of references a read must match (default: all of them)"},
    {"match-prefix", "", kString, "filename prefix for matching reads"},
    {"non-match-prefix", "", kString, "filename prefix for non-matching reads"},
};
// translucent's own (TranslucentApp.cc:97, TransCmdMergeGraphWithReference.cc:141-142).  relative-cutoff is text here as
// in kTrimPrune: the command that takes it converts it
const OptDef kRelativeCutoff[] = {
    {"relative-cutoff", "", kString, "relative coverage cutoff"},
};
const OptDef kGraphRef[] = {
    {"graph-ref", "", kString, "name of the reference graph object"},
};
// xenome's and electus' own (XenoApp.cc:130-133, 231-236, 300; ElectApp.cc:143)
const OptDef kIndexPrefix[] = {
    {"prefix", "P", kString, "filename prefix for index"},
};
const OptDef kRefPrefix[] = {
    {"prefix", "P", kString, "reference output prefix"},
};
const OptDef kXenoRefs[] = {
    {"graft", "G", kString, "graft reference in FASTA format"},
    {"host", "H", kString, "host reference in FASTA format"},
};
const OptDef kXenoNames[] = {
    {"graft-name", "", kString, "name of graft reads"},
    {"host-name", "", kString, "name of host reads"},
    {"output-filename-prefix", "", kString, "prefix for output files"},
};
const OptDef kRefFasta[] = {
    {"ref-fasta", "", kStrings, "reference file in FASTA format"},
};
const OptDef kAnnotate[] = {
    {"annotation-list", "", kString, "A file containing a list of graph names, 1 per line."},
    {"phylogeny", "", kString, "A file containing a list of merges to perform to construct the phylogenetic tree."},
};

// --tmp-dir: the last one given, which must be a directory (the reference fails when it first creates a temporary file
// there: "PhysicalFileFactory::tmpName"; here the check comes first, with the name in the message)
std::string tmpDirOption(const std::map<std::string, std::vector<std::string>>& vals)
{
    auto it = vals.find("tmp-dir");
    if (it == vals.end() || it->second.empty()) return std::string();
    const std::string& d = it->second.back();
    struct stat st;
    if (::stat(d.c_str(), &st) != 0) throw Error::Errno(d, errno);
    if (!S_ISDIR(st.st_mode)) throw Error::General("--tmp-dir: " + d + " is not a directory\n");
    return d;
}

struct Parsed {
    std::map<std::string, std::vector<std::string>> vals;
    size_t count(const std::string& k) const { auto i = vals.find(k); return i == vals.end() ? 0 : i->second.size(); }
    const std::string& str(const std::string& k) const { return vals.at(k).back(); }
    const std::vector<std::string>& strs(const std::string& k) const { return vals.at(k); }
};

struct OptTable {
    std::vector<OptDef> defs;
    void add(const OptGroup& g) { defs.insert(defs.end(), g.defs, g.defs + g.n); }
    const OptDef* findLong(const std::string& n, bool& ambiguous) const
    {
        ambiguous = false;
        const OptDef* hit = nullptr;
        for (auto& d : defs) if (n == d.lng) return &d;
        for (auto& d : defs)                      // unique-prefix guessing, as program_options does
            if (strncmp(d.lng, n.c_str(), n.size()) == 0) { if (hit) { ambiguous = true; return nullptr; } hit = &d; }
        return hit;
    }
    const OptDef* findShort(char c) const
    {
        for (auto& d : defs) if (d.sht[0] == c && d.sht[0]) return &d;
        return nullptr;
    }
    std::string describe() const
    {
        std::ostringstream os;
        for (auto& d : defs)
        {
            std::string l = "  ";
            if (d.sht[0]) l += std::string("-") + d.sht + " [ --" + d.lng + " ]"; else l += std::string("--") + d.lng;
            if (d.kind != kFlag) l += " arg";
            if (l.size() < 40) l.resize(40, ' '); else l += " ";
            os << l << d.help << "\n";
        }
        return os.str();
    }
};

uint64_t toU64(const std::string& opt, const std::string& v)
{
    if (v.empty() || v[0] == '-') throw Error::Usage("the argument ('" + v + "') for option '--" + opt + "' is invalid\n");
    char* end = nullptr;
    errno = 0;
    unsigned long long x = strtoull(v.c_str(), &end, 10);
    if (errno || *end) throw Error::Usage("the argument ('" + v + "') for option '--" + opt + "' is invalid\n");
    return x;
}

// Parses argv[first..] against the table; unknown tokens are collected like
// command_line_parser(...).allow_unregistered() + the check at App.cc:255-262.
void parseArgs(int argc, char** argv, int first, const OptTable& t, Parsed& out, std::string& badMsg)
{
    for (int i = first; i < argc; ++i)
    {
        std::string tok = argv[i];
        const OptDef* d = nullptr;
        std::string inlineVal; bool hasInline = false;
        if (tok.size() > 2 && tok[0] == '-' && tok[1] == '-')
        {
            std::string name = tok.substr(2);
            size_t eq = name.find('=');
            if (eq != std::string::npos) { inlineVal = name.substr(eq + 1); name = name.substr(0, eq); hasInline = true; }
            bool amb;
            d = t.findLong(name, amb);
        }
        else if (tok.size() >= 2 && tok[0] == '-' && tok[1] != '-')
        {
            d = t.findShort(tok[1]);
            if (d && tok.size() > 2)
            {
                if (d->kind == kFlag) d = nullptr;      // grouped flags are not used by goss
                else { inlineVal = tok.substr(2); hasInline = true; }
            }
        }
        if (!d)
        {
            badMsg += "unknown option '" + tok + "'\n";
            continue;
        }
        if (d->kind == kFlag)
        {
            out.vals[d->lng].push_back("1");
            continue;
        }
        std::string v;
        if (hasInline) v = inlineVal;
        else if (i + 1 < argc) v = argv[++i];
        else throw Error::Usage(std::string("the required argument for option '--") + d->lng + "' is missing\n");
        if (d->kind == kU64) toU64(d->lng, v);
        out.vals[d->lng].push_back(v);
    }
}

// GossOptionChecker: accumulates error text, decides usage vs general error.
struct Checker {
    const Parsed& o;
    Logger* log;                        // the command's, for the checks that warn (none: dump-bases)
    std::string errors = {};
    bool suggestUsage = false;
    std::string notOffered = {};        // a part of the command that this build refuses: a usage error once the checks have passed
    std::string refused = {};           // an object the command cannot take: an error under the command's name, after those
    bool flag(const std::string& n) const { return o.count(n) != 0; }
    bool optional(const std::string& n, std::string& v) const
    {
        if (!o.count(n)) return false;
        v = o.str(n);
        return true;
    }
    bool mandatory(const std::string& n, std::string& v)
    {
        if (optional(n, v)) return true;
        errors += "mandatory option " + n + " was not given.\n";
        suggestUsage = true;
        return false;
    }
    bool mandatoryU64(const std::string& n, uint64_t& v, uint64_t maxv)
    {
        if (!o.count(n)) { errors += "mandatory option " + n + " was not given.\n"; suggestUsage = true; return false; }
        v = toU64(n, o.str(n));
        if (v > maxv)
        {
            errors += "The given value of the option " + n + " was invalid.\n";
            errors += "\tvalue " + num(v) + " is out of range.\n\tthe maximum allowed value is " + num(maxv) + ".\n";
            suggestUsage = true;
            return false;
        }
        return true;
    }
    bool optionalU64(const std::string& n, uint64_t& v)
    {
        if (!o.count(n)) return false;
        v = toU64(n, o.str(n));
        return true;
    }
    // --max-memory: a double as lexical_cast reads it; a value that is none ends the command at once, before -h is looked at
    void maxMemory(double& v)
    {
        if (!o.count("max-memory")) return;
        const std::string& s = o.str("max-memory");
        char* end = nullptr;
        errno = 0;
        v = strtod(s.c_str(), &end);
        if (s.empty() || errno || *end) throw Error::Usage("the argument ('" + s + "') for option '--max-memory' is invalid\n");
    }
    // getRepeatingOnce / getRepeatingTwice (GossOptionChecker.hh:235-254): all of them, or none and an error
    strings repeating(const std::string& n, size_t times)
    {
        if (o.count(n) == times) return o.strs(n);
        if (!o.count(n)) errors += "mandatory option " + n + " was not given.\n";
        else errors += "mandatory option " + n + " must be supplied exactly " + (times == 1 ? "once" : "twice") + ".\n";
        suggestUsage = true;
        return strings();
    }
    std::string once(const std::string& n)
    {
        const strings v = repeating(n, 1);
        return v.empty() ? std::string() : v[0];
    }
    // FileCreateCheck(fac, true): "<name>.test" must be creatable (GossOptionChecker.hh:80-122)
    bool mandatoryOut(const std::string& n, std::string& v)
    {
        if (!mandatory(n, v)) return false;
        std::string probe = v + ".test";
        FILE* fp = fopen(probe.c_str(), "wb");
        if (!fp)
        {
            errors += "The given value of the option " + n + " was invalid.\n";
            errors += "\tcannot create filenames with prefix '" + v + "'\n";
            return false;
        }
        fclose(fp);
        ::remove(probe.c_str());
        return true;
    }
    // --output-file with FileCreateCheck(fac, false): the file itself is created, and stays ("-" is standard output)
    void outputFile(std::string& v)
    {
        if (!optional("output-file", v) || v == "-") return;
        FILE* fp = fopen(v.c_str(), "wb");
        if (!fp)
        {
            errors += "The given value of the option output-file was invalid.\n";
            errors += "\tcannot create file '" + v + "'\n";
        }
        else fclose(fp);
    }
    // FileReadCheck (GossOptionChecker.hh:125-156)
    void repeatingIn(const std::string& n, strings& vals)
    {
        if (!o.count(n)) return;
        vals = o.strs(n);
        for (auto& f : vals)
            if (!InFile::readable(f))
            {
                errors += "The given value of the option " + n + " was invalid.\n";
                errors += "\tcannot open file '" + f + "' for reading\n";
            }
    }
    // expandFilenames (GossOptionChecker.hh:405-430): one name per '\n'-terminated line
    void expand(const std::string& n, strings& names)
    {
        if (!o.count(n)) return;
        for (auto& lf : o.strs(n))
        {
            InFile in(lf);
            std::string all; char buf[65536]; size_t got;
            while ((got = in.read(buf, sizeof buf)) > 0) all.append(buf, got);
            size_t b = 0;
            for (;;)
            {
                size_t e = all.find('\n', b);
                if (e == std::string::npos) break;      // a last line without '\n' is dropped
                names.push_back(all.substr(b, e - b));
                b = e + 1;
            }
        }
    }
    // --fasta-in, --fastq-in, --line-in: the read inputs of the commands that take no lists of them
    void readsIn(strings& fastas, strings& fastqs, strings& lines)
    {
        repeatingIn("fasta-in", fastas);
        repeatingIn("fastq-in", fastqs);
        repeatingIn("line-in", lines);
    }
    // the same with --fastas-in / --fastqs-in, each list behind its option's own files
    void readsAndListsIn(strings& fastas, strings& fastqs)
    {
        repeatingIn("fasta-in", fastas);
        expand("fastas-in", fastas);
        repeatingIn("fastq-in", fastqs);
        expand("fastqs-in", fastqs);
    }
    void throwIfNecessary()
    {
        if (errors.empty()) return;
        if (suggestUsage) throw Error::Usage(errors);
        throw Error::General(errors);
    }
};

// What the reference sizes its BackyardHash with for -B: N slots' worth of items and
// BackyardHash::maxSlotBits(B << 30) = floor(log2((B<<30)/22)) (BackyardHash.hh:414-418)
void hashSizes(uint64_t B, uint64_t& S, uint64_t& N)
{
    N = (uint64_t)((double)(B << 30) / (1.5 * 4 + 16));
    S = (uint64_t)std::log2((double)N);
}

// ---- one create per command: reads and checks its options, accumulating errors, and returns what to run ----

using Run = std::function<void(const GossCmdContext&)>;

template <class Cmd> Run run(Cmd cmd) { return [cmd](const GossCmdContext& cxt) mutable { cmd(cxt); }; }

// GossCmdFactoryBuildKmerSet/BuildGraph::create (GossCmdBuildKmerSet.cc:151-198, GossCmdBuildGraph.cc:428-476)
template <class Cmd, bool isGraph> Run createBuild(Checker& chk)
{
    if (chk.o.count("debug"))
        for (auto& d : chk.o.strs("debug")) (*chk.log)(warning, "unknown debug: " + d);
    uint64_t K = 0;
    chk.mandatoryU64("kmer-size", K, isGraph ? 62 : 63);
    uint64_t B = 2;
    chk.optionalU64("buffer-size", B);
    if (isGraph && B > 24)
    {
        (*chk.log)(warning, "Unsupported --buffer-size " + num(B) + ", truncating to 24.");
        B = 24;
    }
    uint64_t S = 0, N = 0;
    hashSizes(B, S, N);
    if (!isGraph) chk.optionalU64("log-hash-slots", S);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    strings fastas, fastqs, lines;
    chk.readsAndListsIn(fastas, fastqs);
    chk.repeatingIn("line-in", lines);
    return run(Cmd(K, S, N, T, outName, fastas, fastqs, lines));
}

// GossCmdFactoryMerge<T>::create (GossCmdMerge.tcc:329-378)
template <class Cmd> Run createMerge(Checker& chk)
{
    strings ins;
    if (chk.o.count("graph-in")) ins = chk.o.strs("graph-in");
    chk.expand("graphs-in", ins);
    if (ins.empty()) chk.errors += "At least one input graph must be supplied either using --graph-in or --graphs-in.\n";
    uint64_t maxMerge = 8;
    chk.optionalU64("max-merge", maxMerge);
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    return run(Cmd(ins, maxMerge, outName));
}

// GossCmdFactoryIntersectKmerSets::create (GossCmdIntersectKmerSets.cc:131-150),
// GossCmdFactorySubtractKmerSet::create (GossCmdSubtractKmerSet.cc:88-113)
template <class Cmd, bool exactlyTwo> Run createSetAlgebra(Checker& chk)
{
    strings ins;
    if (chk.o.count("graph-in")) ins = chk.o.strs("graph-in");
    chk.expand("graphs-in", ins);
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    if (exactlyTwo && ins.size() != 2) chk.errors += "Exactly two input k-mer sets required!";
    return run(Cmd(ins, outName));
}

// GossCmdFactoryMergeAndAnnotateKmerSets::create (GossCmdMergeAndAnnotateKmerSets.cc:209-224)
Run createMergeAndAnnotate(Checker& chk)
{
    strings ins = chk.repeating("graph-in", 2);
    ins.resize(2);
    std::string outName;
    chk.mandatory("graph-out", outName);
    return run(GossCmdMergeAndAnnotateKmerSets(ins[0], ins[1], outName));
}

// GossCmdFactoryGraphToKmerSet::create (GossCmdGraphToKmerSet.cc:62-77)
Run createGraphToKmerSet(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatory("graph-out", outName);
    return run(GossCmdGraphToKmerSet(in, outName));
}

// GossCmdFactoryDumpKmerSet/DumpGraph::create (GossCmdDumpKmerSet.cc:58-73, GossCmdDumpGraph.cc:64-79)
template <class Cmd> Run createDump(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string textName = "-";
    chk.outputFile(textName);
    return run(Cmd(in, textName));
}

// GossCmdFactoryRestoreGraph::create (GossCmdRestoreGraph.cc:138-152)
Run createRestoreGraph(Checker& chk)
{
    std::string textName = "-", outName;
    chk.optional("input-file", textName);
    chk.mandatoryOut("graph-out", outName);
    return run(GossCmdRestoreGraph(textName, outName));
}

// GossCmdFactoryLintGraph::create (GossCmdLintGraph.cc:278-292)
Run createLintGraph(Checker& chk)
{
    return run(GossCmdLintGraph(chk.once("graph-in"), chk.flag("dump-properties")));
}

// GossCmdFactoryTrimGraph::create (GossCmdTrimGraph.cc:130-172)
Run createTrimGraph(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    uint64_t cutoff = 0;
    const bool inferCutoff = !chk.optionalU64("cutoff", cutoff);
    if (chk.flag("estimate-only") && !inferCutoff) throw Error::Usage("cannot estimate cutoff unless it is also being inferred");
    if (inferCutoff && chk.flag("scale-cutoff-by-k")) throw Error::Usage("cannot scale an inferred cutoff");
    // the inferred cutoff (EstimateGraphStatistics, a Levenberg-Marquardt fit of the multiplicity histogram)
    // and what hangs on it are not part of this build
    if (inferCutoff || chk.flag("scale-cutoff-by-k"))
        chk.notOffered = ("not implemented: give -C (the cutoff is not inferred by this build; --estimate-only and "
                          "--scale-cutoff-by-k are not offered)\n");
    return run(GossCmdTrimGraph(in, outName, cutoff));
}

// GossCmdFactoryPruneTips::create (GossCmdPruneTips.cc:347-373)
Run createPruneTips(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    // the reference reads both optionals whether given or not (GossCmdPruneTips.cc:79-80) and compares
    // the count with the relative cutoff (:172): defined only when both are given -- neither is offered
    if (chk.flag("cutoff") || chk.flag("relative-cutoff"))
        chk.notOffered = ("not implemented: --cutoff and --relative-cutoff (the reference reads them unset "
                          "unless both are given, so their behaviour is undefined)\n");
    uint64_t iterations = 1;
    chk.optionalU64("iterate", iterations);
    return run(GossCmdPruneTips(in, outName, iterations));
}

// GossCmdFactoryTrimPaths::create (GossCmdTrimPaths.cc:251-279)
Run createTrimPaths(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    uint64_t cutoff = 0;
    chk.mandatoryU64("cutoff", cutoff, ~0ULL);
    uint64_t ignoredThreads = 4;            // (the walk is the device's)
    chk.optionalU64("num-threads", ignoredThreads);
    return [=](const GossCmdContext& cxt) {
        // numeric_cast<uint32_t>(c) (GossCmdTrimPaths.cc:270), thrown before the command exists
        if (cutoff > 0xFFFFFFFFULL) throw std::range_error("bad numeric conversion: positive overflow");
        GossCmdTrimPaths cmd(in, outName, (uint32_t)cutoff);
        cmd(cxt);
    };
}

// GossCmdFactoryClipLinks::create (GossCmdClipLinks.cc:177-199)
Run createClipLinks(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    return run(GossCmdClipLinks(in, outName));
}

// GossCmdFactoryPrintContigs::create (GossCmdPrintContigs.cc:226-289)
Run createPrintContigs(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    uint64_t ignoredThreads = 1, minCoverage = 0, minLength = 0;
    chk.optionalU64("num-threads", ignoredThreads);
    chk.optionalU64("min-coverage", minCoverage);
    chk.optionalU64("min-length", minLength);
    if (chk.flag("include-entailed-contigs") || chk.flag("print-entailed-contigs"))
        chk.notOffered = ("not implemented: --print-entailed-contigs / --include-entailed-contigs (they belong to "
                          "supergraph contigs; this build prints linear segments only)\n");
    std::string textName = "-";
    chk.outputFile(textName);
    // the reference would print the supergraph's contigs here (GossCmdPrintContigs.cc:208-221)
    if (!in.empty() && !chk.flag("print-linear-segments") && ::access((in + "-supergraph.header").c_str(), F_OK) == 0)
        chk.refused = ("\t'" + in + "' has a supergraph: supergraph contigs are not implemented by this build; "
                       "give --print-linear-segments to print the graph's linear segments\n");
    return run(GossCmdPrintContigs(in, minCoverage, minLength, chk.flag("no-sequence"), chk.flag("verbose-headers"),
                                   chk.flag("no-line-breaks"), textName));
}

// GossCmdFactoryBuildEntryEdgeSet::create (GossCmdBuildEntryEdgeSet.cc:68-84)
Run createBuildEntryEdgeSet(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    uint64_t ignoredThreads = 4;            // (the walk is the device's)
    chk.optionalU64("num-threads", ignoredThreads);
    return run(GossCmdBuildEntryEdgeSet(in));
}

// GossCmdFactoryComputeNearKmers::create (GossCmdComputeNearKmers.cc:230-243)
Run createComputeNearKmers(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    uint64_t T = 4;                         // (the loop is the device's)
    chk.optionalU64("num-threads", T);
    return run(GossCmdComputeNearKmers(in, T));
}

// GossCmdFactoryPoolSamples::create (GossCmdPoolSamples.cc:255-318)
Run createPoolSamples(Checker& chk)
{
    uint64_t K = 25;
    if (chk.o.count("kmer-size")) chk.mandatoryU64("kmer-size", K, 63);
    uint64_t B = 2, S = 0, N = 0;
    chk.optionalU64("buffer-size", B);
    hashSizes(B, S, N);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    std::string outName;
    chk.mandatoryOut("graph-out", outName);          // (optional in the reference: see GossCmdPoolSamples)
    strings kmerSets, fastas, fastqs;
    if (chk.o.count("kmer-set-in")) kmerSets = chk.o.strs("kmer-set-in");
    chk.expand("kmer-sets-in", kmerSets);
    chk.readsAndListsIn(fastas, fastqs);
    return run(GossCmdPoolSamples(K, S, N, T, outName, fastas, fastqs, kmerSets));
}

// GossCmdFactoryCountComponents::create (GossCmdCountComponents.cc:314-350)
Run createCountComponents(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.optional("graph-out", outName);
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    return run(GossCmdCountComponents(in, outName, fastas, fastqs, lines));
}

// GossCmdFactoryBuildSubgraph::create (GossCmdBuildSubgraph.cc:215-268)
Run createBuildSubgraph(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    uint64_t radius = 1, B = 2;
    chk.optionalU64("radius", radius);
    chk.optionalU64("buffer-size", B);
    return run(GossCmdBuildSubgraph(in, outName, fastas, fastqs, lines, radius, chk.flag("linear-paths"), B << 30));
}

// GossCmdFactoryExtractReads::create (GossCmdExtractReads.cc:113-139)
Run createExtractReads(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    std::string outName = "-";
    chk.outputFile(outName);
    return run(GossCmdExtractReads(in, fastas, fastqs, lines, outName));
}

// GossCmdFactoryFilterReads::create (GossCmdFilterReads.cc:312-349)
Run createFilterReads(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    std::string matchName, nonMatchName;
    chk.optional("match-file", matchName);
    chk.optional("non-match-file", nonMatchName);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    return run(GossCmdFilterReads(in, fastas, fastqs, lines, chk.flag("pairs"), chk.flag("count"), T, matchName, nonMatchName));
}

// GossCmdFactoryGroupReads::create (GossCmdGroupReads.cc:1037-1084)
Run createGroupReads(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    double M = 1.0e9;
    chk.maxMemory(M);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    std::string lhsName = "lhs", rhsName = "rhs", prefix;
    chk.optional("lhs-name", lhsName);
    chk.optional("rhs-name", rhsName);
    chk.optional("output-filename-prefix", prefix);
    return run(GossCmdGroupReads(in, fastas, fastqs, lines, chk.flag("pairs"), M, T, lhsName, rhsName, prefix,
                                 chk.flag("dont-write-reads"), chk.flag("preserve-read-order")));
}

// ElectCmdFactoryGroup::create (ElectApp.cc:703-783)
Run createElectReads(Checker& chk)
{
    strings refFastas, refIndexes, fastas, fastqs, lines;
    chk.repeatingIn("ref-fasta", refFastas);
    if (chk.o.count("ref-index")) refIndexes = chk.o.strs("ref-index");
    chk.readsIn(fastas, fastqs, lines);
    uint64_t K = 25;
    if (chk.o.count("kmer-size")) chk.mandatoryU64("kmer-size", K, 63);
    if (K == 0) { chk.errors += "The given value of the option kmer-size was invalid.\n\tvalue 0 is out of range.\n"; chk.suggestUsage = true; }
    double M = 1.0e9;
    chk.maxMemory(M);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    uint64_t refThreshold = ~0ULL;
    chk.optionalU64("ref-threshold", refThreshold);
    std::string match, nonMatch, pool;
    chk.optional("match-prefix", match);
    chk.optional("non-match-prefix", nonMatch);
    chk.optional("pool", pool);
    const size_t nrefs = refFastas.size() + refIndexes.size();
    if (pool.empty() && nrefs == 0) { chk.errors += "no references: give ref-fasta, ref-index or pool.\n"; chk.suggestUsage = true; }
    if (!pool.empty() && nrefs) { chk.errors += "pool stands in for the references: ref-fasta and ref-index cannot be given with it.\n"; chk.suggestUsage = true; }
    if (nrefs > 64)
    { chk.errors += num(nrefs) + " references were given; a read's word holds at most 64.\n"; chk.suggestUsage = true; }
    return run(GossCmdElectReads(K, refThreshold, refFastas, refIndexes, pool, fastas, fastqs, lines, chk.flag("pairs"), M, T, match, nonMatch,
                                 chk.flag("preserve-read-order")));
}

// GossCmdFactoryAnnotateKmers::create (GossCmdAnnotateKmers.cc:402-433)
Run createAnnotateKmers(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string annotList, phylogeny;
    chk.mandatory("annotation-list", annotList);
    chk.mandatory("phylogeny", phylogeny);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    return run(GossCmdAnnotateKmers(in, annotList, phylogeny, T));
}

// GossCmdFactoryClassifyReads::create (GossCmdClassifyReads.cc:512-557)
Run createClassifyReads(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    uint64_t B = 2, T = 4;
    chk.optionalU64("buffer-size", B);
    chk.optionalU64("num-threads", T);
    return run(GossCmdClassifyReads(in, fastas, fastqs, lines, B << 30, T, chk.flag("pairs")));
}

// TransCmdFactoryTrimRelative::create (TransCmdTrimRelative.cc:284-307).  The cutoff is a double as lexical_cast reads
// it, and must be a finite number: anything else is the usage error of a malformed numeric option.
Run createTrimRelative(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string outName;
    chk.mandatoryOut("graph-out", outName);
    double relCutoff = 0.02;
    if (chk.o.count("relative-cutoff"))
    {
        const std::string& s = chk.o.str("relative-cutoff");
        char* end = nullptr;
        errno = 0;
        relCutoff = strtod(s.c_str(), &end);
        if (s.empty() || isspace((unsigned char)s[0]) || errno || *end || !std::isfinite(relCutoff))
            throw Error::Usage("the argument ('" + s + "') for option '--relative-cutoff' is invalid\n");
    }
    uint64_t numThreads = 4;                // (the pass is the device's)
    chk.optionalU64("num-threads", numThreads);
    return run(TransCmdTrimRelative(in, outName, relCutoff, numThreads));
}

// TransCmdFactoryMergeGraphWithReference::create (TransCmdMergeGraphWithReference.cc:114-133)
Run createMergeGraphWithReference(Checker& chk)
{
    const std::string in = chk.once("graph-in");
    std::string ref, outName;
    chk.mandatory("graph-ref", ref);
    chk.mandatoryOut("graph-out", outName);
    return run(TransCmdMergeGraphWithReference(ref, in, outName));
}

// ---- xenome and electus: the commands of XenoApp.cc and ElectApp.cc, each a few of the commands above in one process ----

// What the reference sizes its BackyardHash with for -M (XenoApp.cc:54-57, ElectApp.cc:84-87): 0.2 GB held back.  The
// build accepts both and ignores them, so -M changes nothing here.
void hashSizesOfMemory(double M, uint64_t& S, uint64_t& N)
{
    const double bytes = std::max(0.0, M - 0.2) * 1024 * 1024 * 1024;
    N = (uint64_t)(bytes / (1.5 * 4 + 16));
    S = N ? (uint64_t)std::log2((double)N) : 0;
}

std::string elapsedSince(std::chrono::steady_clock::time_point t0)
{
    std::ostringstream os;
    os << "total elapsed time: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return os.str();
}

// bases of a FASTA file, from its size (0: unknown)
uint64_t fastaBases(const std::string& f)
{
    struct stat st;
    if (f == "-" || ::stat(f.c_str(), &st) != 0) return 0;
    const size_t n = f.size();
    const double x = n > 3 && f.compare(n - 3, 3, ".gz") == 0 ? 4.5 : n > 4 && f.compare(n - 4, 4, ".bz2") == 0 ? 5.0 : 1.0;
    return (uint64_t)((double)st.st_size * x);
}

// XenoCmdIndex (XenoApp.cc:49-98): the four steps with one GossCmdContext -- and here one goss_gpu_ctx, which the
// context carries from step to step (SharedContext).  The files go through the file system between the steps.
class XenoCmdIndex {
public:
    XenoCmdIndex(const std::string& pGraft, const std::string& pHost, const std::string& pOut, uint64_t pK, double pM, uint64_t pT)
        : mGraft(pGraft), mHost(pHost), mOut(pOut), mK(pK), mM(pM), mT(pT) {}
    void operator()(const GossCmdContext& pCxt)
    {
        const auto t0 = std::chrono::steady_clock::now();
        Logger& log = pCxt.log;
        uint64_t S = 0, N = 0;
        hashSizesOfMemory(mM, S, N);
        const std::string g = mOut + "-graft", h = mOut + "-host", b = mOut + "-both";
        GossCmdContext cxt = pCxt;
        if (!cxt.gpu) cxt.gpu = std::make_shared<SharedContext>();
        const uint64_t gb = fastaBases(mGraft), hb = fastaBases(mHost);
        if (gb && hb) cxt.gpu->arenaBytes = sharedArenaBytes(gb + hb);

        log(info, "building graft reference kmer set");
        GossCmdBuildKmerSet(mK, S, N, mT, g, strings(1, mGraft), strings(), strings())(cxt);
        log(info, "building host reference kmer set");
        GossCmdBuildKmerSet(mK, S, N, mT, h, strings(1, mHost), strings(), strings())(cxt);
        log(info, "merging host and graft reference kmer sets");
        GossCmdMergeAndAnnotateKmerSets(g, h, b)(cxt);
        log(info, "computing marginal kmers");
        GossCmdComputeNearKmers(b, mT)(cxt);
        log(info, elapsedSince(t0));
    }
private:
    const std::string mGraft, mHost, mOut; const uint64_t mK; const double mM; const uint64_t mT;
};

// XenoCmdFactoryIndex::create (XenoApp.cc:100-135): kmer-size, graft, host, prefix in the reference's order
Run createXenoIndex(Checker& chk)
{
    uint64_t K = 25;
    if (chk.o.count("kmer-size")) chk.mandatoryU64("kmer-size", K, 63);
    std::string graft, host, out;
    chk.mandatory("graft", graft);
    chk.mandatory("host", host);
    chk.mandatory("prefix", out);
    double M = 2;
    chk.maxMemory(M);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    return run(XenoCmdIndex(graft, host, out, K, M, T));
}

// XenoCmdFactoryGroup::create and XenoCmdGroup (XenoApp.cc:137-238): group-reads on <prefix>-both
Run createXenoClassify(Checker& chk)
{
    std::string in;
    chk.mandatory("prefix", in);
    strings fastas, fastqs, lines;
    chk.readsIn(fastas, fastqs, lines);
    double M = 1.0e9;
    chk.maxMemory(M);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    std::string graftName = "graft", hostName = "host", prefix;
    chk.optional("graft-name", graftName);
    chk.optional("host-name", hostName);
    chk.optional("output-filename-prefix", prefix);
    GossCmdGroupReads cmd(in + "-both", fastas, fastqs, lines, chk.flag("pairs"), M, T, graftName, hostName, prefix,
                          chk.flag("dont-write-reads"), chk.flag("preserve-read-order"));
    return [cmd](const GossCmdContext& cxt) mutable {
        const auto t0 = std::chrono::steady_clock::now();
        cmd(cxt);
        cxt.log(info, elapsedSince(t0));
    };
}

// ElectCmdFactoryIndex::create and ElectCmdIndex (ElectApp.cc:74-146): one k-mer set of all the reference files
Run createElectIndex(Checker& chk)
{
    uint64_t K = 25;
    if (chk.o.count("kmer-size")) chk.mandatoryU64("kmer-size", K, 63);
    strings refs;
    chk.repeatingIn("ref-fasta", refs);
    if (!chk.o.count("ref-fasta")) { chk.errors += "repeating option ref-fasta must be given at least once.\n"; chk.suggestUsage = true; }      // getRepeating1
    std::string out;
    chk.mandatory("prefix", out);
    double M = 2;
    chk.maxMemory(M);
    uint64_t T = 4;
    chk.optionalU64("num-threads", T);
    uint64_t S = 0, N = 0;
    hashSizesOfMemory(M, S, N);
    GossCmdBuildKmerSet cmd(K, S, N, T, out, refs, strings(), strings());
    return [cmd](const GossCmdContext& cxt) mutable {
        const auto t0 = std::chrono::steady_clock::now();
        cxt.log(info, "building reference kmer set");
        cmd(cxt);
        cxt.log(info, elapsedSince(t0));
    };
}

// ---- the commands that are no factory's: their own arguments, no help of their own, no logger ----

struct App;

int helpCommand(const App& app, int argc, char** argv);

// goss synth-reads <nreads> <read_len> <genome_len> <seed> <out.fq>: the bench's
// deterministic synthetic read set as 4-line FASTQ
int synthReadsCommand(const App&, int argc, char** argv)
{
    if (argc != 7) throw Error::Usage("usage: goss synth-reads <nreads> <read-len> <genome-len> <seed> <out.fq>\n");
    uint64_t n = toU64("nreads", argv[2]), L = toU64("read-len", argv[3]), G = toU64("genome-len", argv[4]);
    uint64_t seed = toU64("seed", argv[5]);
    FILE* fp = fopen(argv[6], "wb");
    if (!fp) throw Error::Errno(argv[6], errno);
    const uint64_t per = 65536;
    std::vector<char> bases(per * (L + 1));
    std::string out;
    std::string qual(L, 'I');
    for (uint64_t r0 = 0; r0 < n; r0 += per)
    {
        uint64_t m = std::min(per, n - r0);
        if (goss_synth_reads_host(bases.data(), m, (uint32_t)L, G, seed, r0) != GOSS_OK)
            throw Error::General("synth-reads: invalid arguments\n");
        out.clear();
        for (uint64_t i = 0; i < m; ++i)
        {
            out += "@r"; out += std::to_string(r0 + i); out += '\n';
            out.append(bases.data() + i * (L + 1), L + 1);
            out += "+\n"; out += qual; out += '\n';
        }
        if (fwrite(out.data(), 1, out.size(), fp) != out.size()) { fclose(fp); throw Error::Write(argv[6]); }
    }
    fclose(fp);
    return 0;
}

// goss dump-bases: the build commands' inputs (and -T) through the framers to standard output (dumpBases)
int dumpBasesCommand(const App&, int argc, char** argv)
{
    OptTable t;
    for (auto& g : {group(kGlobal), group(kBufferSize), group(kReadLists), group(kLineIn), group(kOutAndK)}) t.add(g);
    Parsed opts; std::string bad;
    parseArgs(argc, argv, 2, t, opts, bad);
    if (!bad.empty()) throw Error::Usage(bad);
    Checker chk{opts, nullptr};
    strings fastas, fastqs, lines;
    chk.readsAndListsIn(fastas, fastqs);
    chk.repeatingIn("line-in", lines);
    chk.throwIfNecessary();
    uint64_t T = 1;
    chk.optionalU64("num-threads", T);
    try { dumpBases(fastas, fastqs, lines, T); }
    catch (Error& e) { e.cmd = argv[1]; throw; }
    return 0;
}

// ---- the table: today's help order; the groups between kGlobal and kGpuSpecific in the order -h prints them ----

enum : unsigned {
    kHbmBudget = 1,         // the context honours --hbm-budget
    kTmpDir = 2,            // ... and --tmp-dir (a directory that is none ends the command before it runs)
    kBuild = 4,             // a build command: --devices is parsed, and --tmp-dir gets a note in the log
    kUsageUntagged = 8,     // a usage error from the run keeps its form (elect-reads: a reference of another K)
};

struct Command {
    const char* name;
    const char* summary;                    // nullptr: not listed by help
    std::vector<OptGroup> groups;
    unsigned flags;
    Run (*create)(Checker&);
    int (*plain)(const App& app, int argc, char** argv);    // set: run instead of the driver
};

// An executable: the name its help and its errors speak under, and its commands in help order.
struct App {
    const char* name;
    std::vector<const Command*> commands;
    const Command* find(const std::string& n) const
    {
        for (const Command* c : commands) if (n == c->name) return c;
        return nullptr;
    }
};

const unsigned kAll = kHbmBudget | kTmpDir;

const Command kCommands[] = {
    {"build-graph", "create a new graph", {group(kBufferSize), group(kReadLists), group(kLineIn), group(kOutAndK)}, kAll | kBuild,
     createBuild<GossCmdBuildGraph, true>, nullptr},
    {"build-kmer-set", "create a new graph", {group(kBufferSize), group(kReadLists), group(kLineIn), group(kOutAndK), group(kKmerSetSpecific)},
     kAll | kBuild, createBuild<GossCmdBuildKmerSet, false>, nullptr},
    {"dump-graph", "write out the graph in a robust text representation.", {group(kMerge)}, kAll, createDump<GossCmdDumpGraph>, nullptr},
    {"dump-kmer-set", "write out the graph in a robust text representation.", {group(kMerge)}, kAll, createDump<GossCmdDumpKmerSet>, nullptr},
    {"help", "print a summary of all the commands.", {}, 0, nullptr, helpCommand},
    {"lint-graph", "verify that a graph structure is internally consistent", {group(kMerge)}, kAll, createLintGraph, nullptr},
    {"restore-graph", "read in a graph from a robust text representation.", {group(kMerge)}, kAll, createRestoreGraph, nullptr},
    {"intersect-kmer-sets", "generate the intersection of the given k-mer sets", {group(kMerge)}, kAll,
     createSetAlgebra<GossCmdIntersectKmerSets, false>, nullptr},
    {"merge-and-annotate-kmer-sets", "Decorate a graph with an assignment of kmers to graphs.", {group(kMerge)}, kAll, createMergeAndAnnotate, nullptr},
    {"compute-near-kmers", "Decorate a graph with an assignment of kmers to graphs.", {group(kMerge)}, kAll, createComputeNearKmers, nullptr},
    {"merge-graphs", "create a new graph by merging zero or more existing graphs", {group(kMerge)}, kAll, createMerge<GossCmdMergeGraphs>, nullptr},
    {"merge-kmer-sets", "create a new graph by merging zero or more existing graphs", {group(kMerge)}, kAll, createMerge<GossCmdMergeKmerSets>, nullptr},
    {"subtract-kmer-set", "subtract the second k-mer set from the first", {group(kMerge)}, kAll,
     createSetAlgebra<GossCmdSubtractKmerSet, true>, nullptr},
    {"graph-to-kmer-set", "generate a graph's k-mer set", {group(kMerge)}, kAll, createGraphToKmerSet, nullptr},
    {"trim-graph", "create a new graph by trimming low frequency edges", {group(kMerge), group(kCutoff), group(kTrimPrune)}, kAll, createTrimGraph, nullptr},
    {"prune-tips", "create a new graph by removing low frequency tips", {group(kMerge), group(kCutoff), group(kTrimPrune)}, kAll, createPruneTips, nullptr},
    {"trim-paths", "create a new graph by removing low frequency paths", {group(kMerge), group(kCutoff)}, kAll, createTrimPaths, nullptr},
    {"clip-links", "create a new graph by removing spurious links", {group(kMerge)}, kAll, createClipLinks, nullptr},
    {"print-contigs", "print all the non-branching paths in the given assembly graph", {group(kMerge), group(kContigs)}, kAll, createPrintContigs, nullptr},
    {"build-entry-edge-set", "build an entry edge set for a graph", {group(kMerge)}, kAll, createBuildEntryEdgeSet, nullptr},
    {"count-components", "count connected components in the graph represented by the given reads", {group(kGraphIn), group(kGraphOut), group(kReadsIn)},
     kHbmBudget, createCountComponents, nullptr},
    {"build-subgraph", "generate a subgraph of an existing graph", {group(kGraphIn), group(kGraphOut), group(kReadsIn), group(kBufferSize), group(kSubgraph)},
     kHbmBudget, createBuildSubgraph, nullptr},
    {"extract-reads", "extract reads which map on to a graph", {group(kGraphIn), group(kReadsIn), group(kExtract)}, 0, createExtractReads, nullptr},
    {"filter-reads", "filter reads keeping/discarding those that coincide with a graph.", {group(kGraphIn), group(kReadsIn), group(kFilter)}, 0,
     createFilterReads, nullptr},
    {"group-reads", "filter reads keeping/discarding those that coincide with a graph.",
     {group(kGraphIn), group(kReadsIn), group(kGroupMemory), group(kPairs), group(kGroupNames), group(kReadOrder)}, 0, createGroupReads, nullptr},
    {"pool-samples", "pool all the samples", {group(kBufferSize), group(kReadLists), group(kOutAndK), group(kPool)}, kAll, createPoolSamples, nullptr},
    {"annotate-kmers", "Decorate a graph with an assignment of kmers to graphs.", {group(kGraphIn), group(kAnnotate)}, 0, createAnnotateKmers, nullptr},
    {"classify-reads", "thread the reads through the graph", {group(kBufferSize), group(kGraphIn), group(kReadsIn), group(kPairs)}, 0,
     createClassifyReads, nullptr},
    {"elect-reads", "classify reads according to reference",
     {group(kElectRefs), group(kReadsIn), group(kElectSizes), group(kPairs), group(kReadOrder), group(kElectOut)}, kAll | kUsageUntagged,
     createElectReads, nullptr},
    {"synth-reads", nullptr, {}, 0, nullptr, synthReadsCommand},
    {"dump-bases", nullptr, {}, 0, nullptr, dumpBasesCommand},
};

// translucent's own two commands (TranslucentApp.cc:72,76).  Both factories of the reference carry the same summary.
const char* const kTransSummary = "create a new graph from an existing graph, using coverage information from a reference graph";
const Command kTransCommands[] = {
    {"trim-relative", kTransSummary, {group(kGraphIn), group(kGraphOut), group(kRelativeCutoff)}, kAll, createTrimRelative, nullptr},
    {"merge-graph-with-reference", kTransSummary, {group(kGraphIn), group(kGraphOut), group(kGraphRef)}, kAll, createMergeGraphWithReference, nullptr},
};

// xenome's two commands (XenoApp.cc:274-275) and electus' (ElectApp.cc:802-803).  `electus classify` is goss's
// elect-reads record under that name: the same groups, the same create.
const Command kXenoCommands[] = {
    {"index", "build an index for classifying reads", {group(kIndexPrefix), group(kElectSizes), group(kXenoRefs)}, kAll, createXenoIndex, nullptr},
    {"classify", "classify reads according to index",
     {group(kReadsIn), group(kIndexPrefix), group(kGroupMemory), group(kPairs), group(kXenoNames), group(kReadOrder)}, 0, createXenoClassify, nullptr},
};
const Command kElectCommands[] = {
    {"classify", "classify reads according to reference",
     {group(kElectRefs), group(kReadsIn), group(kElectSizes), group(kPairs), group(kReadOrder), group(kElectOut)}, kAll | kUsageUntagged,
     createElectReads, nullptr},
    {"index", "build an index for classifying reads", {group(kRefFasta), group(kElectSizes), group(kRefPrefix)}, kAll, createElectIndex, nullptr},
};

const App& gossApp()
{
    static const App app = [] {
        App a{"goss", {}};
        for (auto& c : kCommands) a.commands.push_back(&c);
        return a;
    }();
    return app;
}

// The commands of TranslucentApp.cc:68-76 that this build implements, in its order: goss's records for the four it
// shares with goss, as they are, and the two above.  pop-bubbles and assemble are not built.
const App& translucentApp()
{
    static const App app = [] {
        App a{"translucent", {}};
        for (const char* n : {"help", "build-graph", "lint-graph", "trim-graph"}) a.commands.push_back(gossApp().find(n));
        a.commands.push_back(&kTransCommands[0]);
        a.commands.push_back(gossApp().find("prune-tips"));
        a.commands.push_back(&kTransCommands[1]);
        return a;
    }();
    return app;
}

// XenoApp.cc:274-276 and ElectApp.cc:802-804: their commands in their order, then goss's help record
const App& xenomeApp()
{
    static const App app{"xenome", {&kXenoCommands[0], &kXenoCommands[1], gossApp().find("help")}};
    return app;
}

const App& electusApp()
{
    static const App app{"electus", {&kElectCommands[0], &kElectCommands[1], gossApp().find("help")}};
    return app;
}

const char* kVersion = "1.3.0-mi355x";

void printHelp(const App& app, const std::string& cmdName, const OptTable* t)
{
    std::cerr << app.name << " <command> [options]\n\ncommands implemented by this build:\n";
    for (const Command* c : app.commands)
        if (c->summary)
        {
            std::string l = c->name;
            l.resize(std::max<size_t>(17, l.size() + 2), ' ');
            std::cerr << "  " << l << c->summary << "\n";
        }
    if (t)
    {
        std::cerr << "\n" << cmdName << "\n" << t->describe() << std::endl;
    }
}

int helpCommand(const App& app, int, char**)
{
    printHelp(app, "help", nullptr);
    return 0;
}

// --devices "0,1,2,3": one context per listed device (an ordinal may appear twice: two contexts share that GPU)
void devicesOption(const std::string& v, std::vector<int>& devices)
{
    size_t at = 0;
    while (at <= v.size())
    {
        const size_t comma = std::min(v.find(',', at), v.size());
        const std::string item = v.substr(at, comma - at);
        if (item.empty() || item.find_first_not_of("0123456789") != std::string::npos || item.size() > 3)
            throw Error::Usage("--devices takes a comma-separated list of device ordinals, e.g. 0,1,2,3\n");
        devices.push_back(atoi(item.c_str()));
        at = comma + 1;
    }
    if (devices.size() > 64) throw Error::Usage("--devices: at most 64 devices\n");
}

// The driver: one command from its arguments to its run, the steps in the order App::main takes them.
int runCommand(const App& app, const Command& c, int argc, char** argv)
{
    OptTable t;
    t.add(group(kGlobal));
    for (auto& g : c.groups) t.add(g);
    t.add(group(kGpuSpecific));
    Parsed opts; std::string bad;
    parseArgs(argc, argv, 2, t, opts, bad);
    if (!bad.empty())
    {
        if (opts.count("help")) { std::cerr << bad; printHelp(app, c.name, &t); return 1; }
        throw Error::Usage(bad);
    }

    // logging (App.cc:291-301)
    FILE* fp = stderr;
    if (opts.count("log-file"))
    {
        fp = fopen(opts.str("log-file").c_str(), "w");
        if (!fp) throw Error::Errno(opts.str("log-file"), errno);
    }
    std::unique_ptr<Logger> logger(new Logger(fp, opts.count("verbose") ? info : warning, fp != stderr));

    Checker chk{opts, logger.get()};
    Run go = c.create(chk);
    if (opts.count("help")) { printHelp(app, c.name, &t); return 1; }
    chk.throwIfNecessary();
    if (!chk.notOffered.empty()) throw Error::Usage(chk.notOffered);
    if (!chk.refused.empty())
    {
        Error e = Error::General(chk.refused);
        e.cmd = c.name;
        throw e;
    }

    GossCmdContext cxt{*logger, c.name};
    uint64_t dev = 0, budgetGb = 0;
    if (chk.optionalU64("device", dev)) cxt.device = (int)dev;
    if ((c.flags & kHbmBudget) && chk.optionalU64("hbm-budget", budgetGb)) cxt.hbmBudget = budgetGb << 30;
    if (c.flags & kTmpDir) cxt.tmpDir = tmpDirOption(opts.vals);
    if (c.flags & kBuild)
    {
        if (!cxt.tmpDir.empty())
            (*logger)(info, "--tmp-dir " + cxt.tmpDir + ": not needed by this build (the runs of its chunks are held in HBM and merged there; no temporary file is written)");
        if (opts.count("devices")) devicesOption(opts.str("devices"), cxt.devices);
    }
    try { go(cxt); }
    catch (Error& e)
    {
        if (!(c.flags & kUsageUntagged) || e.usage.empty()) e.cmd = c.name;
        throw;
    }
    return 0;
}

// App::main (App.cc:176-417) for one executable: the command named by the first argument, from `app`'s table.
int appMain(const App& app, int argc, char* argv[])
{
    std::string cmdName;
    try
    {
        for (int i = 1; i < argc; ++i)
            if (!strcmp(argv[i], "--version")) { std::cout << app.name << " version " << kVersion << std::endl; return 0; }

        if (argc < 2 || (argc == 2 && (!strcmp(argv[1], "--help") || !strcmp(argv[1], "-h")))) cmdName = "help";
        else cmdName = argv[1];
        if (const Command* c = app.find(cmdName)) return c->plain ? c->plain(app, argc, argv) : runCommand(app, *c, argc, argv);
        std::cerr << "unknown command '" << cmdName << "'" << std::endl;
        printHelp(app, cmdName, nullptr);
        return 0;
    }
    catch (const Error& e)
    {
        // the printing order of App.cc:328-417
        if (!e.cmd.empty()) std::cerr << "error performing " << e.cmd << ":" << std::endl;
        if (!e.parse.empty()) std::cerr << "\t'" << e.file << "': " << e.parse << std::endl;
        if (!e.write_name.empty()) std::cerr << "\tcannot write to '" << e.write_name << "'" << std::endl;
        if (!e.general.empty()) std::cerr << e.general;
        if (e.err_no)
        {
            std::cerr << "\t";
            if (!e.file.empty()) std::cerr << "'" << e.file << "': ";
            std::cerr << strerror(e.err_no) << std::endl;
        }
        if (!e.usage.empty())
        {
            std::cerr << e.usage;
            std::cerr << "use\n\t" << app.name << " " << cmdName << " -h\nfor more usage information." << std::endl;
        }
        return 1;
    }
    catch (std::exception& e)
    {
        std::cerr << "caught unexpected exception: " << e.what() << std::endl;
        return 1;
    }
    catch (...)
    {
        std::cerr << "caught unknown exception" << std::endl;
        return 1;
    }
    return 0;
}

}  // namespace

int gossMain(int argc, char* argv[]) { return appMain(gossApp(), argc, argv); }

int translucentMain(int argc, char* argv[]) { return appMain(translucentApp(), argc, argv); }

int xenomeMain(int argc, char* argv[]) { return appMain(xenomeApp(), argc, argv); }

int electusMain(int argc, char* argv[]) { return appMain(electusApp(), argc, argv); }

void runAndExit(int (*appMain)(int, char*[]), int argc, char* argv[])
{
    const int rc = appMain(argc, argv);
    const char* full = std::getenv("GOSS_FULL_EXIT");
    if ((full && *full == '1') || std::getenv("LD_PRELOAD") || std::getenv("ROCP_TOOL_LIBRARIES") || std::getenv("ROCPROFILER_REGISTER_FORCE_LOAD"))
    {
        releaseKeptBuffers();
        std::exit(rc);
    }
    std::fflush(nullptr);
    _exit(rc);
}

}  // namespace gosshost
