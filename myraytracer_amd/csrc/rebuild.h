// rebuild.h — device side of rt_scene_commit_ex(RT_COMMIT_REBUILD_FIT): the flattened instance
// tree (scene.cpp build_fit, wide.h fit_walk) built again, on the device, for the committed pose.
//
// Why any topology will do.  The fit tree is a superset filter only (wide.h fit header): a candidate
// is accepted after the reference's exact FP64 tests of the TLAS leaf box, the BLAS root box and the
// leaf box, and equal-t ties are re-walked in the reference's order.  So the walk returns the
// reference's hit for every tree in which each (instance, leaf run) pair is one terminal slot and
// every slot box contains what lies below it.  A refit keeps the topology of the pose the scene was
// created at; this builds one for the pose it has now.  The pair array is not touched: terminal
// slot ~p still names pair p, and fit_walk / fit_boxes_exact change nowhere.
//
//   k_rb_pair_boxes  every pair's FP64 world box (refit.h pair_world_box, which k_refit_level calls
//       too) and the union of all of them (refit.h block_box_union, then one block of k_fold_boxes).
//   k_rb_morton     63-bit Morton code, 21 bits per axis, of the pair's centroid normalised by that
//       union in FP64.  An axis of zero extent gives code bits 0 (no division).  The (code, pair)
//       records are then sorted by hipcub's stable device radix sort; equal codes keep pair order.
//   k_rb_hierarchy  the binary radix tree over the sorted codes (Karras 2012): internal node i
//       finds its range and split from common-prefix lengths; equal codes are told apart by their
//       position in the sorted order (prefix 64 + clz(i ^ j)), so stacked instances give balanced
//       subtrees, not a chain.  Every search loop runs at most 32 steps.
//   k_rb_node_boxes the binary nodes' FP64 boxes bottom-up: one thread per leaf climbs; at each node
//       an arrival counter lets the second arriver through (its sibling's box is complete: released
//       by an agent-scope fence before the sibling counted, acquired by one after this thread did),
//       the first one leaves.  No thread waits.
//   k_rb_collapse / k_rb_emit  four-wide nodes top-down, a launch pair per level.  A node opens its
//       child of largest surface area while the children still fit four slots (build_fit's rule);
//       every pair is one terminal slot.  A level's child nodes are numbered by an exclusive scan of
//       the per-node child counts (hipcub), so the node order - and every byte of the tree - depends
//       on the input only.  Levels are contiguous index ranges: RefitLevels follows from the offsets.
//       Slot boxes: a terminal slot is down / up of its pair box; an inner slot down / up of the
//       binary node's box, which equals the float union of the child node's slots (down and up are
//       monotone); empty slots are +inf in all six rows with ref 0; pad is zero.
// The octant copies are then written by refit.h k_octant_copies.  All stores are vector stores.
// RT_COMMIT_REBUILD_FIT_CLUSTERED replaces k_rb_hierarchy + k_rb_node_boxes by the clustered builder
// (k_pc_*, below); k_fit_cost is the tree cost of rt_scene_fit_cost.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>

#include "layout.h"
#include "refit.h"

namespace myrt {
namespace dev {

constexpr int kRbBlock = 256;
constexpr int kRbParts = 1024;            // blocks of k_rb_pair_boxes at the most
constexpr int kRbMaxClimb = 128;          // a radix tree over 63 + 32 prefix bits is shallower
constexpr int32_t kRbEmpty = INT32_MIN;   // an empty slot of k_rb_collapse (pairs stay below 2^30)

// ---- the live pairs (rtcore.h "instance visibility"): a rebuild holds the pairs of the visible
// instances only.  A pair is live when the device copy of its instance's DInstance has a root box
// (a hidden one has NaNs there, commit.h).  k_rb_live_flags writes the flags (n + 1 entries, the last
// 0), an exclusive scan (hipcub) gives every live pair its place and, in entry n, their number, and
// k_rb_live_scatter writes live[place] = pair: ascending pair order, from the input only.  The
// builder then works on the n_live compact indices i; only k_rb_pair_boxes (pair live[i]) and
// k_rb_emit (terminal slot ~live[i]) translate.  With every instance visible the host passes
// live == nullptr: i is the pair, and every byte is what it was before visibility.
__global__ __launch_bounds__(kRbBlock) void k_rb_live_flags(const DFitPair* fpairs, const DInstance* insts, int64_t n,
                                                            int32_t* flag) {
    const int64_t p = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (p > n) return;
    if (p == n) { flag[p] = 0; return; }
    const double r = insts[fpairs[p].inst].root_lo[0];
    flag[p] = r == r ? 1 : 0;
}
__global__ __launch_bounds__(kRbBlock) void k_rb_live_scatter(const int32_t* flag, const int32_t* place, int64_t n,
                                                              int64_t n_live, int32_t* live) {
    const int64_t p = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (p >= n || !flag[p]) return;
    const int64_t at = place[p];
    if (at >= 0 && at < n_live) live[at] = (int32_t)p;     // n_live is the host's count: never past the array
}

// Grid-stride over the (live) pairs: pbox[6 i] and one partial union per block (partial[6 * blockIdx.x]).
__global__ __launch_bounds__(kRbBlock) void k_rb_pair_boxes(const DFitPair* fpairs, const double* lbox,
                                                            const DInstance* insts, const int32_t* live, int64_t n,
                                                            double* pbox, double* partial) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    const int64_t stride = (int64_t)gridDim.x * kRbBlock;
    for (int64_t p = (int64_t)blockIdx.x * kRbBlock + threadIdx.x; p < n; p += stride) {
        double wlo[3], whi[3];
        pair_world_box(fpairs[live ? live[p] : p], lbox, insts, wlo, whi);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pbox[6 * p + k] = wlo[k]; pbox[6 * p + 3 + k] = whi[k];
            lo[k] = fmin(lo[k], wlo[k]); hi[k] = fmax(hi[k], whi[k]);
        }
    }
    const double v = block_box_union<kRbBlock>(lo, hi);
    if (threadIdx.x < 6) partial[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
}

// 21 bits -> every third bit of 63
__device__ __forceinline__ unsigned long long rb_spread21(unsigned long long x) {
    x &= 0x1fffffull;
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// One thread per pair: its Morton code and its index as the sort's value.
__global__ __launch_bounds__(kRbBlock) void k_rb_morton(const double* pbox, const double* ubox, int64_t n,
                                                        unsigned long long* keys, uint32_t* vals) {
    const int64_t p = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (p >= n) return;
    unsigned long long code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = 0.5 * pbox[6 * p + a] + 0.5 * pbox[6 * p + 3 + a];   // build_fit's centroid
        const double lo = ubox[a], ext = ubox[3 + a] - ubox[a];
        unsigned long long q = 0;
        if (ext > 0.0) {                                   // zero extent (or a NaN): bits 0, no division
            const double x = (c - lo) / ext * 2097152.0;
            q = x >= 2097151.0 ? 2097151ull : (x > 0.0 ? (unsigned long long)x : 0ull);
        }
        code |= rb_spread21(q) << a;
    }
    keys[p] = code;
    vals[p] = (uint32_t)p;
}

// Binary radix tree over n sorted keys: internal nodes 0 .. n - 2 (0 is the root), leaves by sorted
// position.  A child ref >= 0 is an internal node, < 0 the leaf ~position.
struct RbTree {
    const unsigned long long* keys;   // sorted
    int32_t n;
    int32_t* left;                    // per internal node
    int32_t* right;
    int32_t* parent;                  // per internal node (-1: the root)
    int32_t* leaf_parent;             // per leaf
};
__device__ __forceinline__ int rb_delta(const RbTree& T, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)T.n) return -1;
    const unsigned long long a = T.keys[i], b = T.keys[j];
    if (a == b) return 64 + __clz((unsigned)(i ^ j));
    return __clzll((long long)(a ^ b));
}
__global__ __launch_bounds__(kRbBlock) void k_rb_hierarchy(RbTree T) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i >= (int64_t)T.n - 1) return;
    const int64_t d = rb_delta(T, i, i + 1) - rb_delta(T, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = rb_delta(T, i, i - d);
    int64_t lmax = 2;
    for (int it = 0; it < 32 && rb_delta(T, i, i + lmax * d) > dmin; ++it) lmax <<= 1;
    int64_t l = 0;
    for (int it = 0; it < 33; ++it) {
        lmax >>= 1;
        if (lmax < 1) break;
        if (rb_delta(T, i, i + (l + lmax) * d) > dmin) l += lmax;
    }
    const int64_t j = i + l * d;
    const int dnode = rb_delta(T, i, j);
    int64_t s = 0, t = l;
    for (int it = 0; it < 33; ++it) {
        t = (t + 1) >> 1;
        if (rb_delta(T, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const bool lleaf = first == g, rleaf = last == g + 1;
    T.left[i] = lleaf ? ~(int32_t)g : (int32_t)g;
    T.right[i] = rleaf ? ~(int32_t)(g + 1) : (int32_t)(g + 1);
    if (lleaf) T.leaf_parent[g] = (int32_t)i; else T.parent[g] = (int32_t)i;
    if (rleaf) T.leaf_parent[g + 1] = (int32_t)i; else T.parent[g + 1] = (int32_t)i;
    if (i == 0) T.parent[0] = -1;
}

// One thread per leaf climbs towards the root; `arrive` holds zeros at the start.
__global__ __launch_bounds__(kRbBlock) void k_rb_node_boxes(RbTree T, const uint32_t* sorted, const double* pbox,
                                                            unsigned* arrive, double* nbox) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i >= (int64_t)T.n) return;
    int32_t node = T.leaf_parent[i];
    for (int step = 0; step < kRbMaxClimb; ++step) {
        // Release what this thread stored below (the XCDs' L2s are not coherent with each other: the
        // write-back must have completed before the counter moves, hence the explicit wait behind the
        // fence), count, and - as the second arriver - acquire what the sibling's thread stored.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned seen = __hip_atomic_fetch_add(&arrive[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0u) return;                            // the sibling's subtree is not complete yet
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int32_t c[2] = {T.left[node], T.right[node]};
        double lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double* b = c[k] >= 0 ? nbox + 6 * (size_t)c[k] : pbox + 6 * (size_t)sorted[~c[k]];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = k == 0 ? b[a] : fmin(lo[a], b[a]);
                hi[a] = k == 0 ? b[3 + a] : fmax(hi[a], b[3 + a]);
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { nbox[6 * (size_t)node + a] = lo[a]; nbox[6 * (size_t)node + 3 + a] = hi[a]; }
        node = T.parent[node];
        if (node < 0) return;
    }
}

// One level of the collapse.  Node i of the level is the subtree of binary node cur[i].
struct RbLevel {
    const int32_t* left;
    const int32_t* right;
    const double* nbox;           // per binary internal node
    const double* pbox;           // per (live) pair
    const uint32_t* sorted;       // sorted position -> (live) pair
    const int32_t* live;          // live pair -> pair (null: the same)
    const int32_t* cur;           // the level's binary roots
    int32_t count;                // nodes of the level
    int32_t* slots;               // 4 per node: a binary ref or kRbEmpty
    int32_t* cnt;                 // count + 1 entries: child nodes of node i (the last one 0)
    const int32_t* off;           // exclusive scan of cnt (count + 1 entries)
    int32_t* next;                // the next level's binary roots
    W4Node* nodes;                // the level's first node (octant copy 0 of the new tree)
    int32_t child_base;           // node index (whole array) of the next level's first node
};

__global__ __launch_bounds__(kRbBlock) void k_rb_collapse(RbLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i > (int64_t)L.count) return;
    if (i == (int64_t)L.count) { L.cnt[i] = 0; return; }
    const int32_t b = L.cur[i];
    int32_t c[4] = {L.left[b], L.right[b], kRbEmpty, kRbEmpty};
    int nc = 2;
    for (int it = 0; it < 2; ++it) {                       // open the largest child while four slots hold
        int best = -1;
        double bestA = -1.0;
        for (int k = 0; k < nc; ++k) {
            if (c[k] < 0) continue;                        // a pair: terminal
            const double* x = L.nbox + 6 * (size_t)c[k];
            const double dx = x[3] - x[0], dy = x[4] - x[1], dz = x[5] - x[2];
            const double ar = dx * dy + dy * dz + dz * dx;
            if (ar > bestA) { bestA = ar; best = k; }
        }
        if (best < 0) break;
        const int32_t o = c[best];
        for (int k = nc; k > best + 1; --k) c[k] = c[k - 1];
        c[best] = L.left[o];
        c[best + 1] = L.right[o];
        ++nc;
    }
    int inner = 0;
    for (int k = 0; k < 4; ++k) {
        L.slots[4 * i + k] = c[k];
        inner += (k < nc && c[k] >= 0) ? 1 : 0;
    }
    L.cnt[i] = inner;
}

// One thread per slot of the level's nodes.
__global__ __launch_bounds__(kRbBlock) void k_rb_emit(RbLevel L) {
    const int64_t t = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (t >= 4 * (int64_t)L.count) return;
    const int64_t i = t >> 2;
    const int c = (int)(t & 3);
    W4Node& n = L.nodes[i];
    const int32_t s = L.slots[4 * i + c];
    float lo[3] = {HUGE_VALF, HUGE_VALF, HUGE_VALF}, hi[3] = {HUGE_VALF, HUGE_VALF, HUGE_VALF};
    int32_t ref = 0;
    if (s != kRbEmpty) {
        const double* b;
        if (s < 0) {
            const uint32_t p = L.sorted[~s];
            b = L.pbox + 6 * (size_t)p;
            ref = ~(L.live ? L.live[p] : (int32_t)p);
        } else {
            int rank = 0;
            for (int k = 0; k < c; ++k) rank += L.slots[4 * i + k] >= 0 ? 1 : 0;
            const int32_t child = L.off[i] + rank;
            L.next[child] = s;
            b = L.nbox + 6 * (size_t)s;
            ref = L.child_base + child;
        }
        for (int k = 0; k < 3; ++k) { lo[k] = refit_down(b[k]); hi[k] = refit_up(b[3 + k]); }
    }
    for (int k = 0; k < 3; ++k) { n.pnear[k][c] = lo[k]; n.pfar[k][c] = hi[k]; }
    n.ref[c] = ref;
    n.pad[c] = 0;
}

// ---- the clustered builder (RT_COMMIT_REBUILD_FIT_CLUSTERED): parallel locally-ordered
// clustering (Meister & Bittner 2018) over the Morton-sorted pairs.  It stands in for k_rb_hierarchy +
// k_rb_node_boxes and fills what the collapse reads: left, right, nbox (binary node 0 the root) over
// the same `sorted`.  The clusters live in two ping-pong arrays in Morton order: a ref (>= 0 a binary
// node, < 0 the leaf ~sorted position) and an FP64 box.  An iteration is
//   k_pc_neighbour  every cluster picks, among the kPcRadius clusters on either side, the one whose
//       union box with it has the smallest surface area; equal areas go to the smaller i ^ j of the
//       two positions.  For a fixed i that key is unique per j and the whole key is symmetric, so a
//       pair of globally smallest key names each other: every iteration merges at least once.  Equal
//       boxes pair up as (0, 1), (2, 3), ... - halving, not chaining.  (The boxes are finite, so no
//       area is a NaN; an area compares the same whichever way round fmin / fmax saw a -0.0.)
//   k_pc_merge      a cluster whose neighbour's neighbour is itself merges: the lower position lives
//       on as the new binary node, the higher one dies; everyone else is copied.  One 64-bit word per
//       cluster: alive in the low half, "creates a node" in the high half.
//   an exclusive scan of the words (hipcub): new position in the low half, rank among the
//       iteration's merges in the high half; entry `count` holds the totals.
//   k_pc_compact    writes the next array and the new nodes.  Node ids are handed out downward from
//       next_id (n - 2 at first), so the last merge is node 0.
// Positions and ids come from the scan, never from a counter: every byte depends on the input only.
// Kernel boundaries order everything; nothing is handed from block to block inside a kernel.
constexpr int kPcRadius = 16;
constexpr int kPcTile = kRbBlock + 2 * kPcRadius;

__global__ __launch_bounds__(kRbBlock) void k_pc_init(const uint32_t* sorted, const double* pbox, int64_t n,
                                                      int32_t* cref, double* cbox) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i >= n) return;
    const double* b = pbox + 6 * (size_t)sorted[i];
    cref[i] = ~(int32_t)i;
#pragma unroll
    for (int a = 0; a < 6; ++a) cbox[6 * i + a] = b[a];
}

// The block's boxes and kPcRadius more on either side are staged in LDS, one row per component.
__global__ __launch_bounds__(kRbBlock) void k_pc_neighbour(const double* cbox, int32_t count, int32_t* nbr) {
    __shared__ double sm[6][kPcTile];
    const int64_t first = (int64_t)blockIdx.x * kRbBlock - kPcRadius;
    for (int e = threadIdx.x; e < 6 * kPcTile; e += kRbBlock) {
        const int pos = e / 6, a = e - 6 * pos;
        const int64_t g = first + pos;
        sm[a][pos] = (g >= 0 && g < (int64_t)count) ? cbox[6 * g + a] : 0.0;
    }
    __syncthreads();
    const int64_t i = first + kPcRadius + threadIdx.x;
    if (i >= (int64_t)count) return;
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = sm[a][threadIdx.x + kPcRadius];
    int32_t best = -1;
    double bestA = 0.0;
    uint32_t bestX = 0u;
    for (int k = 0; k <= 2 * kPcRadius; ++k) {
        const int64_t j = i - kPcRadius + k;
        if (k == kPcRadius || j < 0 || j >= (int64_t)count) continue;
        const int q = threadIdx.x + k;
        const double dx = fmax(b[3], sm[3][q]) - fmin(b[0], sm[0][q]);
        const double dy = fmax(b[4], sm[4][q]) - fmin(b[1], sm[1][q]);
        const double dz = fmax(b[5], sm[5][q]) - fmin(b[2], sm[2][q]);
        const double ar = dx * dy + dy * dz + dz * dx;
        const uint32_t x = (uint32_t)(i ^ j);
        if (best < 0 || ar < bestA || (ar == bestA && x < bestX)) { best = (int32_t)j; bestA = ar; bestX = x; }
    }
    nbr[i] = best;                                         // count >= 2: there is one
}

__global__ __launch_bounds__(kRbBlock) void k_pc_merge(const int32_t* nbr, int32_t count, unsigned long long* word) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i > (int64_t)count) return;
    if (i == (int64_t)count) { word[i] = 0ull; return; }
    const int32_t j = nbr[i];
    const bool mutual = j >= 0 && j < count && nbr[j] == (int32_t)i;
    word[i] = !mutual ? 1ull : ((int64_t)j > i ? (1ull << 32) | 1ull : 0ull);
}

struct PcStep {
    const int32_t* ref;           // the clusters of this iteration
    const double* box;
    const int32_t* nbr;
    const unsigned long long* word;
    const unsigned long long* scan;   // exclusive scan of word
    int32_t count;
    int32_t next_id;              // the iteration's first merge becomes this binary node
    int32_t nodes;                // binary nodes (n - 1): ids stay below
    int32_t* oref;                // the clusters of the next one
    double* obox;
    int32_t* left;
    int32_t* right;
    double* nbox;
};
__global__ __launch_bounds__(kRbBlock) void k_pc_compact(PcStep P) {
    const int64_t i = (int64_t)blockIdx.x * kRbBlock + threadIdx.x;
    if (i >= (int64_t)P.count) return;
    const unsigned long long w = P.word[i];
    if (!(w & 1ull)) return;                               // merged into the position below
    const unsigned long long s = P.scan[i];
    const int64_t pos = (int64_t)(uint32_t)s;
    if (pos >= (int64_t)P.count) return;
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = P.box[6 * i + a];
    int32_t ref = P.ref[i];
    if (w >> 32) {
        const int32_t j = P.nbr[i];
        const int32_t id = P.next_id - (int32_t)(s >> 32);
        if (id < 0 || id >= P.nodes || j < 0 || j >= P.count) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[a] = fmin(b[a], P.box[6 * (size_t)j + a]);
            b[3 + a] = fmax(b[3 + a], P.box[6 * (size_t)j + 3 + a]);
        }
        P.left[id] = ref;
        P.right[id] = P.ref[j];
#pragma unroll
        for (int a = 0; a < 6; ++a) P.nbox[6 * (size_t)id + a] = b[a];
        ref = id;
    }
    P.oref[pos] = ref;
#pragma unroll
    for (int a = 0; a < 6; ++a) P.obox[6 * pos + a] = b[a];
}

// ---- the cost of a fit tree (rt_scene_fit_cost): the sum, over the non-empty slots of the nodes
// given (octant copy 0's fit nodes, the root first), of the slot box's surface area ex ey + ey ez +
// ez ex with the extents formed in FP64 from the float rows, over the same area of the union of the
// root's slots.  A fixed grid, each block's sum in a fixed order (lanes by shuffle-xor 32 down to 1,
// then the waves in order), then one wave folds the blocks' sums: the value depends on the tree only.
constexpr int kFcBlocks = 64;
__device__ __forceinline__ double wave_fsum(double v) { for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64); return v; }
__global__ __launch_bounds__(kRbBlock) void k_fit_cost(const W4Node* nodes, int64_t count, double* partial) {
    double sum = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kRbBlock;
    for (int64_t t = (int64_t)blockIdx.x * kRbBlock + threadIdx.x; t < 4 * count; t += stride) {
        const W4Node& n = nodes[t >> 2];
        const int c = (int)(t & 3);
        if (!(n.pnear[0][c] < HUGE_VALF) || refit_slot_hidden(n, c)) continue;   // empty, or nothing visible below
        const double ex = (double)n.pfar[0][c] - (double)n.pnear[0][c];
        const double ey = (double)n.pfar[1][c] - (double)n.pnear[1][c];
        const double ez = (double)n.pfar[2][c] - (double)n.pnear[2][c];
        sum += ex * ey + ey * ez + ez * ex;
    }
    sum = wave_fsum(sum);
    __shared__ double sm[kRbBlock / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = sm[0];
        for (int w = 1; w < kRbBlock / 64; ++w) v += sm[w];
        partial[blockIdx.x] = v;
    }
}
// One wave: partial[0 .. parts) folded, divided by the root's area -> out[0]
__global__ __launch_bounds__(64) void k_fit_cost_fold(const double* partial, int parts, const W4Node* root, double* out) {
    double sum = 0.0;
    for (int p = threadIdx.x; p < parts; p += 64) sum += partial[p];
    sum = wave_fsum(sum);
    if (threadIdx.x != 0) return;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int c = 0; c < 4; ++c) {
        if (!(root->pnear[0][c] < HUGE_VALF) || refit_slot_hidden(*root, c)) continue;
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], (double)root->pnear[a][c]); hi[a] = fmax(hi[a], (double)root->pfar[a][c]); }
    }
    const double rx = hi[0] - lo[0], ry = hi[1] - lo[1], rz = hi[2] - lo[2];
    out[0] = sum / (rx * ry + ry * rz + rz * rx);
}

}  // namespace dev
}  // namespace myrt
