// Per-proof claim points of the ring verifier and the tree of their subset sums (dr_ringvrf_verify_each, dr_g1_claim_tree_selftest),
// over fq28.hip.h and the XYZZ law of g1.hip.h.
//
// RingVRF.batch_verify folds the claims of all proofs into two G1 points and one pairing equation.  To say WHICH proof fails, the
// proofs must be kept apart: proof i has L_i (seven claim scalars on its own points, four on the fixed points) and R_i (r1, r2 on its
// two opening proofs), and every subset sum of (L_i, R_i) is a random linear combination that can be tested by itself.
//
//   k_g1_claim_terms   one lane per term k * P: plain double-and-add from the lane's own top bit (all scalars are public, so no
//                      fixed schedule).  Points are Montgomery affine records (the verifier's resident bases), picked by an index
//                      list; zero scalars and points at infinity give the identity.
//   k_g1_claim_tree    leaf mode: a workgroup of 64 lanes owns 64 leaves; a lane sums the terms of its leaf (per component: L is 11
//                      consecutive terms of the proof's 13, R the other 2), the workgroup sums the 64-leaf subtree through LDS and
//                      writes every node.  Top mode: ONE more launch sums the subtree roots (at most 64 for 4096 leaves) the same way.
//   (k_g1_results_affine of kernels_g1.hip.h then brings all nodes to affine standard form in one pass.)
//
// Node array: `comps` trees one behind the other, each 2 * Bp - 1 XYZZ records in heap order (Bp = leaves padded to a power of two
// with the identity): node 0 is the root, the children of node k are 2k + 1 and 2k + 2, leaf i is node Bp - 1 + i.
// g1_add handles equal children (doubling), opposite children (identity) and infinite ones: all three happen with honest inputs.
#pragma once
#include "g1.hip.h"

namespace dr {

constexpr uint32_t CLAIM_TREE_WG = 64;

__global__ __launch_bounds__(64) void k_g1_claim_terms(const uint32_t* __restrict__ bases, const uint32_t* __restrict__ idx /* nullable: term t takes point t */,
                                                        const uint32_t* __restrict__ scalars /* n * 8 */, uint32_t n, uint32_t* __restrict__ terms /* n XYZZ */) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t e[8];
    int top = -1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        e[j] = scalars[(size_t)t * 8 + j];
        if (e[j]) top = 32 * j + 31 - __clz(e[j]);
    }
    const G1Affine p = load_affine(bases, idx ? idx[t] : t);
    G1Xyzz acc = g1_inf();
    if (!p.inf) {
#pragma unroll 1
        for (int bit = top; bit >= 0; bit--) {
            acc = g1_dbl(acc);
            if ((e[bit >> 5] >> (bit & 31)) & 1) acc = g1_madd(acc, p);
        }
    }
    store_xyzz(terms, t, acc);
}

// the subtree over `width` (a power of two, <= 64) values held one per lane: every level's nodes go to the tree's heap array; `nblk`
// workgroups stand side by side, so a level with `cur` nodes per workgroup has cur * nblk nodes in all and starts at heap index cur * nblk - 1
DR_DEV void claim_tree_reduce(uint32_t* lds, const G1Xyzz& leaf, uint32_t width, uint32_t t, uint32_t blk, uint32_t nblk, uint32_t* tree) {
    put_raw(lds + t, CLAIM_TREE_WG, leaf);
    __syncthreads();
#pragma unroll 1
    for (uint32_t cur = width >> 1; cur >= 1; cur >>= 1) {
        G1Xyzz s = g1_inf();
        if (t < cur) s = g1_add(get_raw(lds + 2 * t, CLAIM_TREE_WG), get_raw(lds + 2 * t + 1, CLAIM_TREE_WG));
        __syncthreads();
        if (t < cur) {
            put_raw(lds + t, CLAIM_TREE_WG, s);
            store_xyzz(tree, (size_t)cur * nblk - 1 + (size_t)blk * cur + t, s);
        }
        __syncthreads();
    }
}

struct ClaimTreeShape {
    uint32_t groups;        // live leaves
    uint32_t padded;        // Bp
    uint32_t stride;        // terms per leaf over all components
    uint32_t comps;         // 1 or 2
    uint32_t off[2], m[2];  // component c of leaf g: terms [g * stride + off[c], + m[c])
};

// grid: (max(1, Bp / 64), comps).  top = 0: leaves and the levels of each 64-leaf subtree; top = 1 (one workgroup per component, only
// when Bp > 64): the Bp / 64 subtree roots and the levels above them
__global__ __launch_bounds__(64) void k_g1_claim_tree(const uint32_t* __restrict__ terms, ClaimTreeShape sh, uint32_t* __restrict__ nodes, int top) {
    __shared__ uint32_t lds[XYZZ_RAW_WORDS * CLAIM_TREE_WG];
    const uint32_t t = threadIdx.x, c = blockIdx.y;
    uint32_t* tree = nodes + (size_t)c * (2 * (size_t)sh.padded - 1) * 48;
    if (top) {
        const uint32_t width = sh.padded / CLAIM_TREE_WG;                   // 2 .. 64 subtree roots, at heap index width - 1 + t
        const G1Xyzz v = t < width ? load_xyzz(tree, (size_t)width - 1 + t) : g1_inf();
        claim_tree_reduce(lds, v, width, t, 0, 1, tree);
        return;
    }
    const uint32_t width = sh.padded < CLAIM_TREE_WG ? sh.padded : CLAIM_TREE_WG;
    const uint32_t leaf = blockIdx.x * CLAIM_TREE_WG + t;
    G1Xyzz v = g1_inf();
    if (leaf < sh.groups) {
        const size_t first = (size_t)leaf * sh.stride + sh.off[c];
#pragma unroll 1
        for (uint32_t j = 0; j < sh.m[c]; j++) v = g1_add(v, load_xyzz(terms, first + j));
    }
    if (t < width) store_xyzz(tree, (size_t)sh.padded - 1 + leaf, v);
    claim_tree_reduce(lds, v, width, t, blockIdx.x, gridDim.x, tree);
}

}  // namespace dr
