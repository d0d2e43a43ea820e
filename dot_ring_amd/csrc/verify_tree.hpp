// Which leaves of a sum tree fail, from tests of subset sums (dr_ringvrf_verify_each).  Host only, no GPU: the predicate is an argument.
//
// The tree is the heap of kernels_g1_claims.hip.h: B leaves padded to Bp = 2^depth, node 0 the root, children of k at 2k + 1 and
// 2k + 2, leaf i at Bp - 1 + i.  A node "passes" when the combination of the leaves under it holds.  The descent:
//   - the root is tested; if it passes every leaf passes (one test);
//   - a node is tested only if its parent failed;
//   - a node whose sibling passed under a failed parent is failed without a test (a failed parent has a failed child);
//   - a node with only padding under it is never tested: it passes, so its sibling inherits the parent's failure.
// Per level the left children of all failed parents are tested together, then the right children of those whose left child failed —
// `test` gets a list of nodes and answers for all of them (the caller spreads them over its worker pool).  With k bad leaves at most
// 2k nodes are tested per level: 1 + 2 k depth tests in all.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace drh {

struct VerifyTreeShape {
    size_t leaves, padded, depth;
    explicit VerifyTreeShape(size_t b) : leaves(b), padded(1), depth(0) {
        while (padded < b) { padded <<= 1; depth++; }
    }
    size_t nodes() const { return 2 * padded - 1; }
    // first leaf under `node` and how many (padding included)
    void span(size_t node, size_t& lo, size_t& count) const {
        size_t level = 0;
        while (((size_t)2 << level) - 1 <= node) level++;
        count = padded >> level;
        lo = (node - (((size_t)1 << level) - 1)) * count;
    }
    bool all_padding(size_t node) const {
        size_t lo, count;
        span(node, lo, count);
        return lo >= leaves;
    }
};

// test(nodes, pass): pass[j] = 1 if node nodes[j] holds.  verdicts[i] = 1 for a passing leaf.  Returns the number of nodes tested.
template <class Test>
size_t verify_tree_descend(const VerifyTreeShape& sh, Test&& test, uint8_t* verdicts) {
    size_t tested = 0;
    std::vector<size_t> ask, failed{0};
    std::vector<uint8_t> pass;
    auto run = [&] {
        pass.assign(ask.size(), 0);
        if (!ask.empty()) test(ask, pass);
        tested += ask.size();
    };
    for (size_t i = 0; i < sh.leaves; i++) verdicts[i] = 1;
    if (sh.leaves == 0) return 0;
    ask = failed;
    run();
    if (pass[0]) return tested;
    for (size_t level = 0; level < sh.depth; level++) {
        // left children first (a parent whose right child is padding hands its failure to the left child untested)
        std::vector<size_t> next, undecided;
        ask.clear();
        for (size_t k : failed) {
            if (sh.all_padding(2 * k + 2)) next.push_back(2 * k + 1);
            else { ask.push_back(2 * k + 1); undecided.push_back(k); }
        }
        run();
        ask.clear();
        std::vector<size_t> second;
        for (size_t j = 0; j < undecided.size(); j++) {
            const size_t k = undecided[j];
            if (pass[j]) next.push_back(2 * k + 2);                 // the sibling passed: this one failed
            else { next.push_back(2 * k + 1); ask.push_back(2 * k + 2); second.push_back(k); }
        }
        run();
        for (size_t j = 0; j < second.size(); j++)
            if (!pass[j]) next.push_back(2 * second[j] + 2);
        failed.swap(next);
    }
    for (size_t k : failed) verdicts[k - (sh.padded - 1)] = 0;
    return tested;
}

}  // namespace drh
