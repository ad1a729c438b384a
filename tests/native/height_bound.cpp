// The height bound of the device builders (csrc/bvh_gpu.hip, "Height bound") restated on the host, for this test only: the same
// links / walk / rebuild steps, one loop iteration per device thread, over random binary trees and chains, checked against a
// plain top-down recursion of the rule. For every tree and every cap >= H(n): the result is a binary tree over the same leaves on
// the same inner node ids with h(root) <= cap, subtrees the rule keeps are untouched, and a rebuilt subtree is the median-split
// tree over its own leaves in their depth-first order. Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

namespace {
constexpr uint32_t kLeafMax = 2, kNoNode = 0xFFFFFFFFu;
struct Int2 { int x, y; };
struct Link { uint32_t parent, meta, lsib, lsize; };

uint32_t median_height(uint32_t k) { uint32_t h = 0; while (k > kLeafMax) { k = (k + 1) >> 1; h++; } return h; }

struct Tree {
    uint32_t n = 0; int root = 0;
    std::vector<Int2> children;              // n - 1 inner nodes; a leaf k is ~k
    std::vector<uint32_t> size, height;
    void measure() {                          // sizes and walk heights, bottom-up
        size.assign(n - 1, 0); height.assign(n - 1, 0);
        std::function<void(int)> go = [&](int v) {
            uint32_t s = 0, h = 0;
            for (int c : {children[v].x, children[v].y}) {
                if (c < 0) { s += 1; continue; }
                go(c); s += size[c]; h = std::max(h, height[c]);
            }
            size[v] = s; height[v] = s <= kLeafMax ? 0 : h + 1;
        };
        go(root);
    }
    void leaves_of(int v, std::vector<uint32_t>& out) const {
        if (v < 0) { out.push_back((uint32_t)~v); return; }
        leaves_of(children[v].x, out); leaves_of(children[v].y, out);
    }
};

// Random agglomeration as PLOC numbers its nodes (merge order, root last); `reach` = how far apart two merged clusters may lie
// (1: contiguous ranges, as the radix tree), `chain` = probability of extending the previous cluster (deep trees).
Tree random_tree(uint32_t n, std::mt19937& rng, uint32_t reach, double chain) {
    Tree t; t.n = n; t.children.resize(n - 1);
    std::vector<int> cl(n);
    for (uint32_t i = 0; i < n; i++) cl[i] = ~(int)i;
    uint32_t next = 0, last = 0;
    while (cl.size() > 1) {
        uint32_t i = std::uniform_real_distribution<>(0, 1)(rng) < chain && last < cl.size() ? last : rng() % cl.size();
        uint32_t d = 1 + rng() % reach, j = i + d < cl.size() ? i + d : (i >= d ? i - d : (i + 1) % (uint32_t)cl.size());
        if (j == i) j = (i + 1) % (uint32_t)cl.size();
        if (j < i) std::swap(i, j);
        t.children[next] = rng() & 1 ? Int2{cl[i], cl[j]} : Int2{cl[j], cl[i]};
        cl[i] = (int)next++; cl.erase(cl.begin() + j); last = i;
    }
    t.root = cl[0];
    if (rng() & 1) {                          // the radix tree's numbering: the root is node 0
        std::swap(t.children[0], t.children[t.root]);
        for (Int2& c : t.children) for (int* r : {&c.x, &c.y}) { if (*r == 0) *r = t.root; else if (*r == t.root) *r = 0; }
        t.root = 0;
    }
    t.measure();
    return t;
}

// ---- the device's steps ---------------------------------------------------------------------------------------------------
struct Rebalanced { Tree tree; uint32_t subtrees = 0, prims = 0; bool error = false; };
uint32_t median_gap(uint32_t lo, uint32_t hi) { return lo + ((hi - lo + 1) >> 1) - 1; }

Rebalanced rebalance(const Tree& t, int cap) {
    const uint32_t n = t.n;
    std::vector<Link> link(n - 1); std::vector<std::pair<uint32_t, uint32_t>> leaf_link(n);
    for (uint32_t u = 0; u + 1 < n; u++) {                         // links
        const Int2 ch = t.children[u];
        const uint32_t sl = ch.x < 0 ? 1 : t.size[ch.x], sr = ch.y < 0 ? 1 : t.size[ch.y];
        if (ch.x < 0) leaf_link[~ch.x] = {u, 0}; else { link[ch.x].parent = u; link[ch.x].lsib = 0; }
        if (ch.y < 0) leaf_link[~ch.y] = {u, sl}; else { link[ch.y].parent = u; link[ch.y].lsib = sl; }
        link[u].meta = std::min(t.height[u], 0xFFFFu) | (1 + std::max(median_height(sl), median_height(sr))) << 16;
        link[u].lsize = sl;
        if ((int)u == t.root) { link[u].parent = kNoNode; link[u].lsib = 0; }
    }
    std::vector<uint32_t> leaf_at_pos(n, kNoNode), inner_at_gap(n, kNoNode), rb_gap(n, 0);
    std::vector<std::pair<uint32_t, uint32_t>> rb_range(n, {0, 0});
    Rebalanced out; out.tree = t;
    for (uint32_t th = 0; th < 2 * n - 1; th++) {                  // walk
        const bool leaf = th < n;
        const uint32_t x = leaf ? th : th - n, u0 = leaf ? leaf_link[x].first : x;
        int depth = 0; uint32_t cur = u0;
        for (;; depth++) { if (cur >= n - 1) { out.error = true; break; } const uint32_t p = link[cur].parent; if (p == kNoNode) break; cur = p; }
        if (out.error) return out;
        uint32_t acc = leaf ? leaf_link[x].second : 0, r = kNoNode, rel = 0;
        cur = u0;
        for (int d = depth; d >= 0; d--) {
            const Link L = link[cur];
            const int allowance = cap - d, h = (int)(L.meta & 0xFFFF), need = (int)(L.meta >> 16);
            if (h <= allowance) r = kNoNode; else if (need > allowance) { r = cur; rel = acc; }
            acc += L.lsib; cur = L.parent;
        }
        if (r == kNoNode) continue;
        if (leaf) { leaf_at_pos.at(acc) = x; continue; }
        const uint32_t gap = acc + link[x].lsize - 1;
        inner_at_gap.at(gap) = x;
        rb_range[x] = {acc - rel, t.size[r]};
        rb_gap[x] = gap | (r == x ? 0x80000000u : 0);
    }
    uint32_t root = (uint32_t)t.root;
    auto child = [&](uint32_t lo, uint32_t hi) { return hi - lo == 1 ? ~(int)leaf_at_pos.at(lo) : (int)inner_at_gap.at(median_gap(lo, hi)); };
    for (uint32_t x = 0; x + 1 < n; x++) {                         // rebuild: reads the scratch arrays only
        const auto R = rb_range[x];
        if (R.second < 2) continue;
        const uint32_t g = rb_gap[x] & 0x7FFFFFFFu;
        uint32_t lo = R.first, hi = R.first + R.second;
        for (int i = 0; i < 64 && hi - lo >= 2; i++) { const uint32_t m = median_gap(lo, hi); if (g == m) break; if (g < m) hi = m + 1; else lo = m + 1; }
        if (hi - lo < 2 || median_gap(lo, hi) != g) { out.error = true; return out; }
        out.tree.children[x] = {child(lo, g + 1), child(g + 1, hi)};
        if (rb_gap[x] & 0x80000000u) {
            const uint32_t top = inner_at_gap.at(median_gap(R.first, R.first + R.second));
            if (link[x].parent == kNoNode) root = top;
            else (link[x].lsib ? out.tree.children[link[x].parent].y : out.tree.children[link[x].parent].x) = (int)top;
            out.subtrees++; out.prims += R.second;
        }
    }
    out.tree.root = (int)root;
    return out;
}

// ---- the rule, top-down ---------------------------------------------------------------------------------------------------
int fails = 0;
long rebuilt_total = 0, partial_total = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) printf("line %d: %s (n %u cap %d)\n", __LINE__, #c, t.n, cap); return; } } while (0)

void is_median_tree(const Tree& a, int v, const std::vector<uint32_t>& leaves, uint32_t lo, uint32_t hi, bool& ok) {
    if (hi - lo == 1) { ok = ok && v < 0 && (uint32_t)~v == leaves[lo]; return; }
    if (v < 0) { ok = false; return; }
    const uint32_t mid = median_gap(lo, hi) + 1;
    is_median_tree(a, a.children[v].x, leaves, lo, mid, ok);
    if (ok) is_median_tree(a, a.children[v].y, leaves, mid, hi, ok);
}

void check(const Tree& t, int cap) {
    const Rebalanced rb = rebalance(t, cap);
    CHECK(!rb.error);
    Tree a = rb.tree;
    // a binary tree over the same leaves on the same inner node ids
    std::vector<int> seen_leaf(t.n, 0), seen_inner(t.n - 1, 0);
    uint32_t visited = 0; bool bad = false;
    std::function<void(int)> go = [&](int v) {
        if (bad || ++visited > 2 * t.n) { bad = true; return; }
        if (v < 0) { if ((uint32_t)~v >= t.n || seen_leaf[~v]++) bad = true; return; }
        if ((uint32_t)v >= t.n - 1 || seen_inner[v]++) { bad = true; return; }
        go(a.children[v].x); go(a.children[v].y);
    };
    go(a.root);
    CHECK(!bad && visited == 2 * t.n - 1);
    a.measure();
    CHECK((int)a.height[a.root] <= cap);
    if ((int)t.height[t.root] <= cap) CHECK(rb.subtrees == 0);
    // the rule from the root: kept subtrees untouched, kept splits kept, rebuilt subtrees median trees over their own leaves
    uint32_t subtrees = 0, prims = 0; bool ok = true;
    std::function<void(int, int, int)> rule = [&](int v, int w, int allow) {      // v in t, w its counterpart in a
        if (!ok) return;
        if (v < 0) { ok = w == v; return; }
        if ((int)median_height(t.size[v]) > allow) { ok = false; return; }         // the induction's claim
        if ((int)t.height[v] <= allow) {                                            // whole subtree untouched
            ok = w == v && a.children[v].x == t.children[v].x && a.children[v].y == t.children[v].y;
            rule(t.children[v].x, a.children[v].x, allow - 1); rule(t.children[v].y, a.children[v].y, allow - 1);
            return;
        }
        const Int2 ch = t.children[v];
        const uint32_t sl = ch.x < 0 ? 1 : t.size[ch.x], sr = ch.y < 0 ? 1 : t.size[ch.y];
        if ((int)median_height(sl) <= allow - 1 && (int)median_height(sr) <= allow - 1) {
            if (w != v) { ok = false; return; }
            // a child that is rebuilt is replaced by the holder of its median gap; anything else keeps its id
            rule(ch.x, a.children[v].x, allow - 1); rule(ch.y, a.children[v].y, allow - 1);
            return;
        }
        std::vector<uint32_t> leaves; t.leaves_of(v, leaves);
        subtrees++; prims += (uint32_t)leaves.size();
        is_median_tree(a, w, leaves, 0, (uint32_t)leaves.size(), ok);
    };
    // below a kept-whole node the recursion compares ids one to one; at a rebuilt child only the shape is compared
    std::function<void(int, int, int)> top = rule;
    top(t.root, a.root, cap);
    CHECK(ok);
    CHECK(subtrees == rb.subtrees && prims == rb.prims);
    rebuilt_total += subtrees; partial_total += subtrees && prims < t.n;
}
}  // namespace

int main() {
    std::mt19937 rng(20240611);
    long cases = 0;
    for (int round = 0; round < 160; round++) {
        const uint32_t sizes[] = {2, 3, 4, 5, 7, 63, 64, 65, 200, 960, 3000};
        const uint32_t n = round < 40 ? 2 + round : sizes[rng() % 11];
        const double chain = (round % 4) * 0.33;
        const Tree t = random_tree(n, rng, 1 + (round % 3) * 7, chain);
        const int h0 = (int)median_height(n), h1 = (int)t.height[t.root];
        for (int cap = h0; cap <= std::max(h1, h0) + 1; cap += cap - h0 < 8 || h1 - cap < 3 ? 1 : 1 + (h1 - cap) / 4) { check(t, cap); cases++; }
    }
    {   // the pure chain of 63 under cap 26: 21 levels kept, one subtree of 42 leaves rebuilt
        Tree t; t.n = 63; t.children.resize(62); t.root = 0;
        for (int u = 0; u < 62; u++) t.children[u] = {~u, u == 61 ? ~62 : u + 1};
        t.measure();
        const Rebalanced rb = rebalance(t, 26);
        if (rb.error || rb.subtrees != 1 || rb.prims != 42 || t.height[0] != 61) { printf("chain of 63: %u subtrees, %u prims, height %u\n", rb.subtrees, rb.prims, t.height[0]); fails++; }
        for (int cap = 5; cap <= 62; cap++) { check(t, cap); cases++; }
    }
    if (rebuilt_total < cases / 4 || partial_total < cases / 8) { printf("too few rebuilds for the cases to mean anything\n"); fails++; }
    printf("%s: %ld cases, %ld subtrees rebuilt, %ld cases with a partial rebuild, %d failures\n", fails ? "height bound FAILED" : "height bound ok", cases, rebuilt_total,
           partial_total, fails);
    return fails ? 1 : 0;
}
