// GossTaxo.cpp -- `goss annotate-kmers` (GossCmdAnnotateKmers.cc) and `goss classify-reads` (GossCmdClassifyReads.cc): the
// many-way classification over a k-mer set and a phylogeny.
//
// annotate-kmers gives every k-mer of the set the lowest common ancestor of the taxa whose genomes hold it
// (goss_gpu_object_taxo_annotate_host: the reads of many files in one batch, each with the node id of its file), writes
// <set>.annotation -- a raw uint32 per rank, 0xFFFFFFFF for a k-mer no genome holds -- and writes the phylogeny back with
// `count` and `total` on every node.  classify-reads looks every read's k-mers up in that annotation
// (goss_gpu_object_taxo_classify_reads_host) and counts the read for the deepest of their classes when they lie on one
// root-to-leaf path; the per-node sums go to standard output.  Both reuse GossMatch.cpp's pipeline (GossReads.hpp).
//
// The phylogeny is a nested token list: "(" key value ... child ... ")", tokens separated by whitespace.  It is written as
// AnnotTree::write does: one space per depth, "(" on a line of its own, one key TAB value line per annotation in key order
// (the annotations are a std::map), the children in file order, ")".
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "GossReads.hpp"

namespace gosshost {

using namespace reads;

namespace {

struct TaxoNode {
    std::map<std::string, std::string> anns;
    std::vector<uint32_t> kids;
};

// A phylogeny as read: the nodes in file order (a node before its children), ids and parent indices as
// goss_gpu_object_taxo_tree_host takes them.
struct Phylo {
    std::vector<TaxoNode> nodes;
    std::vector<uint32_t> ids, parent;

    void read(const std::string& name, std::initializer_list<const char*> need)
    {
        std::ifstream in(name);
        if (!in) throw Error::Errno(name, errno ? errno : ENOENT);
        std::vector<std::string> toks;
        for (std::string t; in >> t;) toks.push_back(t);
        size_t at = 0;
        auto fail = [&](const std::string& why) { throw Error::General("\tphylogeny '" + name + "': " + why + "\n"); };
        if (toks.empty() || toks[0] != "(") fail("it does not begin with '('");
        std::vector<uint32_t> open;
        while (at < toks.size())
        {
            const std::string& t = toks[at];
            if (t == "(")
            {
                if (open.empty() && !nodes.empty()) fail("tokens after the root's ')'");
                const uint32_t i = (uint32_t)nodes.size();
                nodes.emplace_back();
                parent.push_back(open.empty() ? i : open.back());
                if (!open.empty()) nodes[open.back()].kids.push_back(i);
                open.push_back(i);
                ++at;
            }
            else if (t == ")")
            {
                if (open.empty()) fail("')' without '('");
                open.pop_back();
                ++at;
            }
            else
            {
                if (open.empty()) fail("tokens after the root's ')'");
                if (!nodes[open.back()].kids.empty()) fail("node " + num(open.back()) + " (in file order) has the key '" + t + "' after a child");
                if (at + 1 >= toks.size() || toks[at + 1] == "(" || toks[at + 1] == ")") fail("the key '" + t + "' has no value");
                nodes[open.back()].anns[t] = toks[at + 1];
                at += 2;
            }
        }
        if (!open.empty()) fail("it ends inside node " + num(open.back()) + " (in file order)");
        std::map<uint32_t, uint32_t> seen;
        for (uint32_t i = 0; i < nodes.size(); ++i)
        {
            for (const char* k : need)
                if (!nodes[i].anns.count(k)) fail("node " + num(i) + " (in file order) has no '" + k + "'");
            const std::string& v = nodes[i].anns["node"];
            char* end = nullptr;
            errno = 0;
            const unsigned long long id = strtoull(v.c_str(), &end, 10);
            if (v.empty() || v[0] < '0' || v[0] > '9' || errno || *end || id > 0xFFFFFFFFULL) fail("node " + num(i) + " (in file order) has the id '" + v + "'");
            if (id == GOSS_TAXO_NONE || id == GOSS_TAXO_MANY) fail("node id " + v + " is reserved");
            if (!seen.emplace((uint32_t)id, i).second) fail("node id " + v + " occurs twice");
            ids.push_back((uint32_t)id);
        }
    }

    // subtree sums of per-node values, children before parents (file order is a pre-order)
    std::vector<uint64_t> totals(const std::vector<uint64_t>& counts) const
    {
        std::vector<uint64_t> t(counts);
        for (size_t i = nodes.size(); i-- > 1;) t[parent[i]] += t[i];
        return t;
    }

    void write(const std::string& name) const
    {
        std::string out;
        // (node, child to visit next): AnnotTree::write without the recursion
        std::vector<std::pair<uint32_t, size_t>> st;
        auto openNode = [&](uint32_t i) {
            const size_t d = st.size();
            out.append(d, ' '); out += "(\n";
            for (const auto& kv : nodes[i].anns) { out.append(d + 1, ' '); out += kv.first; out += '\t'; out += kv.second; out += '\n'; }
            st.emplace_back(i, 0);
        };
        openNode(0);
        while (!st.empty())
        {
            const uint32_t i = st.back().first;
            if (st.back().second < nodes[i].kids.size()) { openNode(nodes[i].kids[st.back().second++]); continue; }
            st.pop_back();
            out.append(st.size(), ' '); out += ")\n";
        }
        FILE* fp = fopen(name.c_str(), "wb");
        if (!fp) throw Error::Errno(name, errno);
        const bool ok = fwrite(out.data(), 1, out.size(), fp) == out.size();
        if (fclose(fp) != 0 || !ok) throw Error::Write(name);
    }
};

void setTree(const Object& g, const Phylo& ph)
{
    g.check(goss_gpu_object_taxo_tree_host(g.h, (uint32_t)ph.ids.size(), ph.ids.data(), ph.parent.data()), "loading the phylogeny");
}

}  // namespace

void GossCmdAnnotateKmers::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    const auto t0 = std::chrono::steady_clock::now();
    (void)mNumThreads;

    // the list: whitespace-separated `file id` pairs, a repeated file keeping its last id; then the tree -- both checked
    // before any device is asked for
    std::map<std::string, uint32_t> ins;
    {
        std::ifstream in(mAnnotList);
        if (!in) throw Error::Errno(mAnnotList, errno ? errno : ENOENT);
        std::string file, id;
        while (in >> file)
        {
            if (!(in >> id)) throw Error::General("\tannotation list '" + mAnnotList + "': '" + file + "' has no node id\n");
            char* end = nullptr;
            errno = 0;
            const unsigned long long v = strtoull(id.c_str(), &end, 10);
            if (id[0] < '0' || id[0] > '9' || errno || *end || v > 0xFFFFFFFFULL)
                throw Error::General("\tannotation list '" + mAnnotList + "': '" + file + "' has the node id '" + id + "'\n");
            ins[file] = (uint32_t)v;
        }
    }
    Phylo ph;
    ph.read(mPhylogeny, {"node", "name"});
    {
        std::map<uint32_t, bool> known;
        for (uint32_t id : ph.ids) known[id] = true;
        for (const auto& kv : ins)
            if (!known.count(kv.second))
                throw Error::General("\tannotation list '" + mAnnotList + "': '" + kv.first + "' has node id " + num(kv.second) + ", which the phylogeny '"
                                     + mPhylogeny + "' lacks\n");
    }

    Object g;
    g.open(pCxt, mRef, false);
    setTree(g, ph);
    g.check(goss_gpu_object_taxo_annotation_host(g.h, nullptr), "starting the annotation");

    // the reads of all the files in batches, the node id of its file beside each read
    std::vector<uint32_t> nodes;
    Matcher matcher(matchBatchBytes(pCxt),
                    [&](const char* buf, size_t bytes, uint64_t n, uint32_t*) {
                        goss_gpu_taxo_info info;
                        g.check(goss_gpu_object_taxo_annotate_host(g.h, buf, bytes, nodes.data(), GOSS_TAXO_NORMALIZE, n, nullptr, &info),
                                "annotating a batch of reads");
                        nodes.clear();
                        return info.reads;
                    },
                    [](const char*, size_t, uint32_t) {});
    for (const auto& kv : ins)
    {
        log(info, "Computing kmers for " + kv.first);
        parseFasta(kv.first, [&](const char* seq, size_t len) {
            matcher.push(seq, len);              // (a full batch leaves first, with the ids it came with)
            nodes.push_back(kv.second);
        });
    }
    matcher.flush();

    log(info, "writing out lca index.");
    std::vector<uint32_t> ann(g.desc.count);
    std::vector<uint64_t> counts(ph.ids.size());
    g.check(goss_gpu_object_taxo_annotation_read(g.h, ann.data(), counts.data()), "reading the annotation");
    {
        const std::string name = mRef + ".annotation";
        FILE* fp = fopen(name.c_str(), "wb");
        if (!fp) throw Error::Errno(name, errno);
        const bool ok = ann.empty() || fwrite(ann.data(), 4, ann.size(), fp) == ann.size();
        if (fclose(fp) != 0 || !ok) throw Error::Write(name);
    }

    log(info, "writing count annotations.");
    const std::vector<uint64_t> totals = ph.totals(counts);
    for (size_t i = 0; i < ph.nodes.size(); ++i)
    {
        ph.nodes[i].anns["count"] = num(counts[i]);
        ph.nodes[i].anns["total"] = num(totals[i]);
    }
    ph.write(mPhylogeny);
    log(info, "total elapsed time: " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()));
}

void GossCmdClassifyReads::operator()(const GossCmdContext& pCxt)
{
    Logger& log(pCxt.log);
    (void)mBufferSize; (void)mNumThreads;
    const std::vector<Item> items = itemsOf(mFastas, mFastqs, mLines);
    if (mPairs && items.size() % 2) throw Error::General("classify-reads --pairs: an even number of input files is required (" + num(items.size()) + " given)\n");

    Phylo ph;
    ph.read(mIn + ".taxo", {"node", "name", "kind"});
    std::vector<uint32_t> ann;
    {
        const std::string name = mIn + ".annotation";
        FILE* fp = fopen(name.c_str(), "rb");
        if (!fp) throw Error::Errno(name, errno);
        uint32_t buf[16384];
        size_t got;
        uint64_t bytes = 0;
        while ((got = fread(buf, 1, sizeof buf, fp)) > 0)
        {
            ann.resize((bytes + got + 3) / 4, 0);
            memcpy((char*)ann.data() + bytes, buf, got);
            bytes += got;
        }
        const bool bad = ferror(fp) != 0;
        fclose(fp);
        if (bad) throw Error::Errno(name, EIO);
        if (bytes % 4) throw Error::General("\tfile '" + name + "' holds " + num(bytes) + " bytes, no whole number of node ids\n");
    }

    Object g;
    g.open(pCxt, mIn, false);
    if (ann.size() != g.desc.count)
        throw Error::General("\tfile '" + mIn + ".annotation' holds " + num(ann.size()) + " node ids; '" + mIn + "' has " + num(g.desc.count) + " k-mers\n");
    setTree(g, ph);
    g.check(goss_gpu_object_taxo_annotation_host(g.h, ann.data()), "loading the annotation");
    std::vector<uint32_t>().swap(ann);

    log(info, "Classifying reads....");
    const size_t cap = matchBatchBytes(pCxt);
    const uint64_t n = ph.ids.size();
    std::vector<uint64_t> counts(n, 0), part(n + 2);
    // the result of every read of one file, in order
    auto classify = [&](const Item& it, std::vector<uint32_t>& out) {
        Matcher matcher(cap,
                        [&](const char* buf, size_t bytes, uint64_t reads, uint32_t* words) {
                            goss_gpu_taxo_info info;
                            g.check(goss_gpu_object_taxo_classify_reads_host(g.h, buf, bytes, GOSS_TAXO_NORMALIZE, reads, words, nullptr, nullptr, &info),
                                    "classifying a batch of reads");
                            return info.reads;
                        },
                        [&](const char*, size_t, uint32_t r) { out.push_back(r); });
        parseItem(it, [&](const char* seq, size_t len) { matcher.push(seq, len); });
        matcher.flush();
    };
    auto tally = [&](const std::vector<uint32_t>& res) {
        g.check(goss_gpu_object_taxo_tally_host(g.h, res.data(), res.size(), part.data()), "counting the results");
        for (uint64_t i = 0; i < n; ++i) counts[i] += part[i];
    };
    if (!mPairs)
    {
        std::vector<uint32_t> res;
        for (const auto& it : items) { res.clear(); classify(it, res); tally(res); }
    }
    else
    {
        // files 2i and 2i + 1 hold the mates: a pair's classes are both mates' pooled, which is the join of the two results
        std::vector<uint32_t> res[2];
        for (size_t i = 0; i + 1 < items.size(); i += 2)
        {
            for (int s = 0; s < 2; ++s) { res[s].clear(); classify(items[i + s], res[s]); }
            if (res[0].size() != res[1].size())
                throw Error::General("classify-reads --pairs: '" + items[i].name + "' holds " + num(res[0].size()) + " reads, '" + items[i + 1].name + "' "
                                     + num(res[1].size()) + "\n");
            g.check(goss_gpu_object_taxo_pair_host(g.h, res[0].data(), res[1].data(), res[0].size(), res[0].data()), "joining the mates");
            tally(res[0]);
        }
    }

    // counts() (GossCmdClassifyReads.cc:397-418): post-order, children first in file order, the nodes whose subtree sum is
    // not zero.  File order is a pre-order, so a node's post-order place is after the last node of its subtree.
    const std::vector<uint64_t> sums = ph.totals(counts);
    std::string out;
    std::vector<std::pair<uint32_t, size_t>> st;
    st.emplace_back(0, 0);
    while (!st.empty())
    {
        const uint32_t i = st.back().first;
        if (st.back().second < ph.nodes[i].kids.size()) { st.emplace_back(ph.nodes[i].kids[st.back().second++], 0); continue; }
        st.pop_back();
        if (sums[i]) out += num(sums[i]) + '\t' + ph.nodes[i].anns.at("kind") + '\t' + ph.nodes[i].anns.at("name") + '\n';
    }
    if (fwrite(out.data(), 1, out.size(), stdout) != out.size() || fflush(stdout) != 0) throw Error::Write("-");
}

}  // namespace gosshost
