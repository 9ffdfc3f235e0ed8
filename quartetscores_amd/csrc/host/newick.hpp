// newick.hpp -- minimal tree model + Newick reader/writer of the C++ host.
//
// Stands where genesis (DefaultTreeNewickReader / NewickInputIterator / NewickWriter) stands in
// the reference (QuartetScores.cpp:23-32,97-98,149-158; QuartetCounterLookup.hpp:202-206). Only
// what the hot path needs: topology, leaf names, verbatim branch lengths, edge comments on output.
// Dialect: nested parentheses, labels plain or 'quoted', ':length', [comments] skipped, ';' ends a tree.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <istream>
#include <stdexcept>
#include <string>
#include <vector>

namespace qsh {

struct Tree {
    // nodes in preorder; node 0 is the root
    std::vector<int32_t> parent;
    std::vector<std::vector<int32_t>> children;
    std::vector<std::string> name;
    std::vector<std::string> length; // verbatim text after ':' ("" = none)

    size_t node_count() const { return parent.size(); }
    size_t edge_count() const { return parent.empty() ? 0 : parent.size() - 1; }
    bool is_leaf(size_t v) const { return children[v].empty(); }
    size_t leaf_count() const {
        size_t k = 0;
        for (size_t v = 0; v < parent.size(); ++v) k += children[v].empty();
        return k;
    }
};

struct NewickError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Streaming reader: one tree per call, from a text buffer.
class NewickReader {
public:
    explicit NewickReader(const std::string &text) : s_(text) {}
    // returns false at end of input
    bool next(Tree &out) {
        skip();
        if (i_ >= s_.size()) return false;
        parse_one(out);
        return true;
    }
    size_t offset() const { return i_; }

private:
    const std::string &s_;
    size_t i_ = 0;

    void skip() {
        while (i_ < s_.size()) {
            char c = s_[i_];
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r') ++i_;
            else if (c == '[') {
                size_t j = s_.find(']', i_);
                if (j == std::string::npos) throw NewickError("unterminated comment");
                i_ = j + 1;
            } else break;
        }
    }
    std::string label() {
        skip();
        std::string out;
        if (i_ < s_.size() && s_[i_] == '\'') {
            ++i_;
            while (i_ < s_.size()) {
                if (s_[i_] == '\'') {
                    if (i_ + 1 < s_.size() && s_[i_ + 1] == '\'') { out.push_back('\''); i_ += 2; continue; }
                    ++i_;
                    break;
                }
                out.push_back(s_[i_++]);
            }
            return out;
        }
        while (i_ < s_.size()) {
            char c = s_[i_];
            if (c == '(' || c == ')' || c == ',' || c == ':' || c == ';' || c == '[' || c == ' ' || c == '\t' || c == '\n' || c == '\r') break;
            out.push_back(c);
            ++i_;
        }
        return out;
    }
    int32_t add(Tree &t, int32_t par) {
        int32_t id = (int32_t)t.parent.size();
        t.parent.push_back(par);
        t.children.emplace_back();
        t.name.emplace_back();
        t.length.emplace_back();
        if (par >= 0) t.children[par].push_back(id);
        return id;
    }
    void parse_one(Tree &t) {
        t = Tree();
        int32_t cur = add(t, -1);
        skip();
        if (i_ < s_.size() && s_[i_] != '(') t.name[cur] = label();
        while (i_ < s_.size()) {
            skip();
            if (i_ >= s_.size()) break;
            char c = s_[i_];
            if (c == '(') {
                cur = add(t, cur);
                ++i_;
                skip();
                if (i_ < s_.size() && s_[i_] != '(' && s_[i_] != ',' && s_[i_] != ')') t.name[cur] = label();
            } else if (c == ',') {
                if (t.parent[cur] < 0) throw NewickError("',' outside parentheses");
                cur = add(t, t.parent[cur]);
                ++i_;
                skip();
                if (i_ < s_.size() && s_[i_] != '(' && s_[i_] != ',' && s_[i_] != ')') t.name[cur] = label();
            } else if (c == ')') {
                if (t.parent[cur] < 0) throw NewickError("unbalanced ')'");
                cur = t.parent[cur];
                ++i_;
                skip();
                if (i_ < s_.size() && s_[i_] != '(' && s_[i_] != ')' && s_[i_] != ',' && s_[i_] != ':' && s_[i_] != ';')
                    t.name[cur] = label();
            } else if (c == ':') {
                ++i_;
                skip();
                size_t j = i_;
                while (j < s_.size() && s_[j] != '(' && s_[j] != ')' && s_[j] != ',' && s_[j] != ';' && s_[j] != '[' && s_[j] != ' ' && s_[j] != '\t' && s_[j] != '\n' && s_[j] != '\r') ++j;
                t.length[cur] = s_.substr(i_, j - i_);
                i_ = j;
            } else if (c == ';') {
                ++i_;
                break;
            } else {
                throw NewickError("unexpected character '" + std::string(1, c) + "' at offset " + std::to_string(i_));
            }
        }
        if (cur != 0) throw NewickError("unbalanced '('");
        // nodes were created in parse order, which is preorder, but a sibling is appended after the
        // whole previous subtree, so ids are already preorder-consistent
    }
};

inline std::string quote_label(const std::string &n) {
    bool need = false;
    for (char c : n) if (c == ' ' || c == '\t' || c == '(' || c == ')' || c == '[' || c == ']' || c == '\'' || c == ':' || c == ';' || c == ',') need = true;
    if (!need) return n;
    std::string o = "'";
    for (char c : n) { if (c == '\'') o += "''"; else o.push_back(c); }
    return o + "'";
}

// Element layout: name, ':length' (only if the input had one), '[comment]'. The reference's layout
// is decided by genesis v0.16.0's NewickWriter (absent here; parity unpinned).
inline std::string write_newick(const Tree &t, const std::function<std::string(size_t)> &comment) {
    std::string out;
    struct Frame { int32_t node; size_t next_child; };
    std::vector<Frame> st;
    st.push_back({0, 0});
    if (!t.children[0].empty()) out.push_back('(');
    while (!st.empty()) {
        Frame &f = st.back();
        const auto &ch = t.children[f.node];
        if (f.next_child < ch.size()) {
            if (f.next_child > 0) out.push_back(',');
            int32_t c = ch[f.next_child++];
            st.push_back({c, 0});
            if (!t.children[c].empty()) out.push_back('(');
            continue;
        }
        if (!ch.empty()) out.push_back(')');
        out += quote_label(t.name[f.node]);
        if (!t.length[f.node].empty()) out += ":" + t.length[f.node];
        if (comment) {
            std::string cm = comment((size_t)f.node);
            if (!cm.empty()) out += "[" + cm + "]";
        }
        st.pop_back();
    }
    out.push_back(';');
    return out;
}

// The branch length of an edge that replaces two edges in a row: the one that is present, their sum when both are (the shortest of
// %.15g / %.16g / %.17g that reads back as the same double), none when neither is.
inline std::string add_lengths(const std::string &a, const std::string &b) {
    if (a.empty() || b.empty()) return a.empty() ? b : a;
    const double x = std::strtod(a.c_str(), nullptr) + std::strtod(b.c_str(), nullptr);
    char text[40];
    for (int digits = 15; digits <= 17; ++digits) {
        std::snprintf(text, sizeof text, "%.*g", digits, x);
        if (std::strtod(text, nullptr) == x) break;
    }
    return text;
}

// `t` without the leaves named in `drop` (names the tree lacks are ignored); false when no leaf is left (`out` is empty then).
// QuartetScores --without-taxa applies this to the reference tree; quartetscores_amd/newick.py prune is the same rule:
//   1. the named leaves go, and, repeatedly, inner nodes left without children;
//   2. a non-root node left with one child is spliced out: the child takes its place in the parent's child order, with the sum of the
//      two branch lengths (add_lengths); the spliced node's label goes;
//   3. a root left with one child is replaced by that child, whose branch length goes;
//   4. where the tree's root had three or more children before pruning and the root that is left -- the old one, or the node that
//      replaced it in step 3 -- has two, it takes the children of its first child that is an inner node in that child's place (whose
//      length goes to the other child, add_lengths): an unrooted tree stays unrooted, so that the scoring does not treat it as a
//      rooted one. Where the tree's root had two children the root is left alone: the tree was rooted;
//   5. child order never changes, so the kept leaves keep their relative depth-first order.
template <typename NameSet> bool prune(const Tree &t, const NameSet &drop, Tree &out) {
    out = Tree();
    const int32_t N = (int32_t)t.node_count();
    std::vector<int32_t> stands(N, -1);   // what stands in the parent's child list for the node (-1: nothing)
    std::vector<std::vector<int32_t>> kids(N);
    std::vector<std::string> length = t.length;
    for (int32_t v = N - 1; v >= 0; --v) {   // preorder ids: children before parents
        if (t.is_leaf(v)) { stands[v] = drop.count(t.name[v]) ? -1 : v; continue; }
        for (int32_t c : t.children[v]) if (stands[c] >= 0) kids[v].push_back(stands[c]);
        if (kids[v].empty()) continue;
        if (kids[v].size() == 1 && v != 0) {
            stands[v] = kids[v][0];
            length[stands[v]] = add_lengths(length[v], length[stands[v]]);
        } else stands[v] = v;
    }
    if (N == 0 || stands[0] < 0) return false;
    int32_t root = 0;
    while (kids[root].size() == 1) root = kids[root][0];
    length[root].clear();
    if (t.children[0].size() >= 3 && kids[root].size() == 2)
        for (size_t i = 0; i < 2; ++i) {
            const int32_t c = kids[root][i];
            if (kids[c].empty()) continue;
            const int32_t other = kids[root][1 - i];
            length[other] = add_lengths(length[c], length[other]);
            std::vector<int32_t> merged = kids[c];
            merged.insert(i == 0 ? merged.end() : merged.begin(), other);
            kids[root] = merged;
            break;
        }
    // preorder copy
    std::vector<std::pair<int32_t, int32_t>> st{{root, -1}};   // (node of t, parent in out)
    while (!st.empty()) {
        const auto [v, par] = st.back();
        st.pop_back();
        const int32_t id = (int32_t)out.parent.size();
        out.parent.push_back(par);
        out.children.emplace_back();
        out.name.push_back(t.name[v]);
        out.length.push_back(length[v]);
        if (par >= 0) out.children[par].push_back(id);
        for (auto it = kids[v].rbegin(); it != kids[v].rend(); ++it) st.push_back({*it, id});
    }
    return true;
}

} // namespace qsh
