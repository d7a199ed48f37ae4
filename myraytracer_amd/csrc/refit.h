// refit.h — device side of rt_scene_commit (dynamic scenes): what depends on the instances'
// transforms and can only be recomputed where the data lives, because rt_scene_create drops the
// host's triangles, leaf boxes and four-wide nodes after upload.
//
//   k_inst_bounds (+ k_fold_boxes)  Instance.worldBounds of every moved triangle-mesh
//       instance: the union over its BLAS's triangles of AABB.transformed(by: localToWorld) of the
//       triangle's local box (refitTLAS step 1, RTContext.swift:889-900; scene.cpp
//       aabb_transformed, restated term for term: the build uses -ffp-contract=off on host and
//       device, so a box equals the host's bit for bit).  min / max are order-independent, so the
//       reduction (FP64, wave shuffles, one partial per block, a final pass) gives the host loop's
//       values; -0 and +0 compare equal and no box test sees the sign of a zero.  The reductions
//       (block_box_union, k_fold_boxes) are shared with rebuild.h and deform.h.
//   k_refit_level  one level of a four-wide tree, bottom-up (a launch per level, deepest first;
//       scene.h RefitLevels): a terminal slot takes its box again, rounded outward to float - by
//       TreeSlotBox the TLAS's instance markers their TLAS leaf box (DWideInst::tbox) and the
//       flattened instance tree's pairs pair_world_box; by LeafRunBox a deformed BLAS's leaf runs
//       their lbox (deform.h) - an inner slot takes the union of its child node's slots; empty
//       slots stay +inf; the slot of a hidden instance takes the hidden encoding (kHiddenNear).  Works on octant copy 0, whose slots are in sorted order: a child is found
//       by its ref, and a union does not depend on the order.
//   k_octant_copies  the eight octant copies of the refit nodes again (scene.cpp
//       wide_octant_copies' rule: near / far rows per octant, slots stable-sorted by centre
//       projection, empties last; MYRT_WIDE_ORDER honoured).
//
// Topology is kept (the reference's refit semantics): every slot box still contains its children's,
// so the trees remain superset filters and the walks' exactness argument (wide.h) holds unchanged.
// All stores are ordinary vector stores; the kernels are deterministic, so replicas end identical.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "layout.h"

#ifndef MYRT_WIDE_ORDER
#define MYRT_WIDE_ORDER 0
#endif

namespace myrt {
namespace dev {

struct RefitMove {            // one moved triangle-mesh instance
    double m[16];             // its new localToWorld (column-major)
    double motion[3];         // the mesh's motion-blur vector (Triangle.motionBlur)
    int32_t tri_first, tri_end;   // its BLAS's TriRec run
    int32_t blur, pad;
};
constexpr int kBoundsBlock = 256;

// ---- reductions shared by the commit kernels (refit.h, deform.h, rebuild.h).  The order of the
// operations is part of what a commit writes (fmin / fmax of -0.0 and +0.0 may depend on it):
// shuffle-xor offsets 32 down to 1, then a block's waves in order, partials with stride 64.
__device__ __forceinline__ double wave_fmin(double v) { for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64)); return v; }
__device__ __forceinline__ double wave_fmax(double v) { for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64)); return v; }
__device__ __forceinline__ void wave_box_union(double lo[3], double hi[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = wave_fmin(lo[k]); hi[k] = wave_fmax(hi[k]); }
}
// The union of the boxes of a block of BLOCK threads (all of them call): thread k < 6 is returned
// component k of it (lo in 0..2, hi in 3..5) and writes it where the kernel keeps its partials.
template <int BLOCK>
__device__ __forceinline__ double block_box_union(double lo[3], double hi[3]) {
    wave_box_union(lo, hi);
    __shared__ double sm[BLOCK / 64][6];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int k = 0; k < 3; ++k) { sm[wave][k] = lo[k]; sm[wave][3 + k] = hi[k]; }
    __syncthreads();
    double v = 0.0;
    if (threadIdx.x < 6) {
        const bool mn = threadIdx.x < 3;
        v = sm[0][threadIdx.x];
        for (int w = 1; w < BLOCK / 64; ++w) v = mn ? fmin(v, sm[w][threadIdx.x]) : fmax(v, sm[w][threadIdx.x]);
    }
    return v;
}
// One wave per block: block b folds the `parts` partial boxes from partial[6 * parts * b] -> out[6 * b]
// (a moved instance's partials, k_inst_bounds; with one block all of rebuild.h k_rb_pair_boxes')
__global__ __launch_bounds__(64) void k_fold_boxes(const double* partial, int parts, double* out) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int p = threadIdx.x; p < parts; p += 64) {
        const double* b = partial + ((size_t)blockIdx.x * parts + p) * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], b[k]); hi[k] = fmax(hi[k], b[3 + k]); }
    }
    wave_box_union(lo, hi);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) { out[6 * (size_t)blockIdx.x + k] = lo[k]; out[6 * (size_t)blockIdx.x + 3 + k] = hi[k]; }
}

// AABB.transformed(by:) (AABB.swift:71-92) in scene.cpp aabb_transformed's operation order
__device__ __forceinline__ void refit_aabb_transformed(const double lo[3], const double hi[3], const double* M,
                                                        double olo[3], double ohi[3]) {
    const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
    const double ex = 0.5 * (hi[0] - lo[0]), ey = 0.5 * (hi[1] - lo[1]), ez = 0.5 * (hi[2] - lo[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = M[0 * 4 + r] * cx;
        acc = M[1 * 4 + r] * cy + acc;
        acc = M[2 * 4 + r] * cz + acc;
        const double cn = acc + M[12 + r];
        const double en = fabs(M[0 * 4 + r]) * ex + fabs(M[1 * 4 + r]) * ey + fabs(M[2 * 4 + r]) * ez;
        olo[r] = cn - en;
        ohi[r] = cn + en;
    }
}

// Block (x, y): a grid-stride share of moved instance y's triangles -> partial[(y * gridDim.x + x) * 6].
// The triangle's local box needs its three vertices exactly: CTri holds them (float-exact scenes),
// otherwise pbox does (6 doubles per TriRec, uploaded for dynamic scenes without CTri; TriRec's
// v0 + e1 is not v1).  A blurred mesh adds the box moved by the motion vector: min over the three
// v + m equals min(v) + m, rounding being monotone (scene.cpp:1370-1374).
__global__ __launch_bounds__(kBoundsBlock) void k_inst_bounds(const CTri* ctris, const double* pbox,
                                                              const RefitMove* moves, double* partial) {
    const RefitMove& mv = moves[blockIdx.y];
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    const int64_t stride = (int64_t)gridDim.x * kBoundsBlock;
    for (int64_t t = (int64_t)mv.tri_first + (int64_t)blockIdx.x * kBoundsBlock + threadIdx.x; t < (int64_t)mv.tri_end;
         t += stride) {
        double plo[3], phi[3];
        if (ctris) {
            const CTri c = ctris[t];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double a = (double)c.v0[k], b = (double)c.v1[k], d = (double)c.v2[k];
                plo[k] = fmin(a, fmin(b, d));
                phi[k] = fmax(a, fmax(b, d));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { plo[k] = pbox[6 * t + k]; phi[k] = pbox[6 * t + 3 + k]; }
        }
        if (mv.blur) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                plo[k] = fmin(plo[k], plo[k] + mv.motion[k]);
                phi[k] = fmax(phi[k], phi[k] + mv.motion[k]);
            }
        }
        double wlo[3], whi[3];
        refit_aabb_transformed(plo, phi, mv.m, wlo, whi);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], wlo[k]); hi[k] = fmax(hi[k], whi[k]); }
    }
    const double v = block_box_union<kBoundsBlock>(lo, hi);
    if (threadIdx.x < 6) partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v;
}

// scene.cpp WideBuilder::down / up: the nearest float not above / not below x
__device__ __forceinline__ float refit_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = nextafterf(f, -HUGE_VALF);
    return f;
}
__device__ __forceinline__ float refit_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, HUGE_VALF);
    return f;
}

// An empty slot has +inf planes; an inner slot takes the float union of its child node's slots
__device__ __forceinline__ bool refit_slot_empty(const W4Node& n, int c) { return !(n.pnear[0][c] < HUGE_VALF); }
__device__ __forceinline__ void refit_slot_union(const W4Node& ch, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = HUGE_VALF; hi[k] = -HUGE_VALF; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (refit_slot_empty(ch, s)) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], ch.pnear[k][s]); hi[k] = fmaxf(hi[k], ch.pfar[k][s]); }
    }
}

// The world box of an (instance, leaf run) pair of the flattened instance tree: the eight corners
// of the leaf box through the instance's localToWorld, min / max (scene.cpp build_fit's formula,
// term for term)
__device__ __forceinline__ void pair_world_box(const DFitPair p, const double* lbox, const DInstance* insts, double wlo[3],
                                               double whi[3]) {
    const double* x = lbox + 6 * (size_t)p.t0;
    const double* M = insts[p.inst].l2w;
    for (int a = 0; a < 3; ++a) { wlo[a] = HUGE_VAL; whi[a] = -HUGE_VAL; }
    for (int q = 0; q < 8; ++q) {
        const double px = (q & 1) ? x[3] : x[0], py = (q & 2) ? x[4] : x[1], pz = (q & 4) ? x[5] : x[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = M[a] * px + M[4 + a] * py + M[8 + a] * pz + M[12 + a];
            wlo[a] = v < wlo[a] ? v : wlo[a];
            whi[a] = v > whi[a] ? v : whi[a];
        }
    }
}

// What a terminal slot (ref < 0) of a refit tree takes its FP64 box from.  TreeSlotBox: the TLAS's
// tree (marker_base >= 0: slot ~(marker_base + instance), its TLAS leaf's box) or the flattened
// instance tree (marker_base < 0: slot ~pair).  LeafRunBox (a BLAS's nodes, deform.h): the leaf
// run's exact box lbox[~ref].
struct TreeSlotBox {
    int32_t marker_base;
    const DWideInst* winst;
    const DFitPair* fpairs;
    const double* lbox;
    const DInstance* insts;
    // false: the slot's instance is hidden (rtcore.h "instance visibility") - the host gave its
    // marker a tbox of NaNs and the device copy of its DInstance a root box of NaNs (commit.h)
    __device__ __forceinline__ bool operator()(int32_t ref, double lo[3], double hi[3]) const {
        if (marker_base >= 0) {
            const double* b = winst[~ref - marker_base].tbox;
            for (int k = 0; k < 3; ++k) { lo[k] = b[k]; hi[k] = b[3 + k]; }
            return b[0] == b[0];
        }
        const DFitPair p = fpairs[~ref];
        pair_world_box(p, lbox, insts, lo, hi);
        const double r = insts[p.inst].root_lo[0];
        return r == r;
    }
};
struct LeafRunBox {
    const double* lbox;
    __device__ __forceinline__ bool operator()(int32_t ref, double lo[3], double hi[3]) const {
        const double* b = lbox + 6 * (size_t)~ref;
        for (int k = 0; k < 3; ++k) { lo[k] = b[k]; hi[k] = b[3 + k]; }
        return true;
    }
};

// A hidden slot (octant copy 0): near planes +FLT_MAX, far planes -FLT_MAX.  (a) No ray enters it in
// any octant copy: a copy swaps the rows of an axis with d < 0, so along every axis the near-plane
// product is +FLT_MAX |1/d| and the far-plane one -FLT_MAX |1/d|; wide_node adds offsets of
// magnitude at most R (1 + 2^-20) |1/d| with R < 2^27 inside the same FMA (wide.h, set_wide), so
// with 2^-100 <= |1/d| <= 2^100 every entry term is positive (or +inf), every exit term negative
// (or -inf), none a NaN, and max(tn, weps) <= min(tf, lim) fails.  (b) pnear[0] < +inf: it is not
// taken for a structural empty (refit_slot_empty), so k_refit_level visits it again and a later
// show gives it its box back.  (c) fminf / fmaxf unions are left alone by it, and the union of
// hidden slots only is the same encoding: an inner slot with nothing visible below is hidden too.
// k_octant_copies' sort key of such a slot is 0.5 (FLT_MAX - FLT_MAX) = 0 per axis: finite, it sorts
// among the slots whose centre projects to the origin, before the structural empties.
constexpr float kHiddenNear = 3.402823466e+38f, kHiddenFar = -3.402823466e+38f;
__device__ __forceinline__ bool refit_slot_hidden(const W4Node& n, int c) { return n.pnear[0][c] > n.pfar[0][c] && n.pnear[0][c] < HUGE_VALF; }

// One thread per slot of the level's `count` nodes list[0 .. count) (octant copy 0): an inner slot
// takes the union of its child node's slots, a terminal slot its box rounded outward to float.
template <class TerminalBox>
__global__ __launch_bounds__(256) void k_refit_level(W4Node* nodes, const int32_t* list, int32_t count, TerminalBox terminal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * (int64_t)count) return;
    W4Node& n = nodes[list[i >> 2]];
    const int c = (int)(i & 3);
    if (refit_slot_empty(n, c)) return;
    const int32_t ref = n.ref[c];
    float lo[3], hi[3];
    if (ref >= 0) {
        refit_slot_union(nodes[ref], lo, hi);
    } else {
        double wlo[3], whi[3];
        const bool visible = terminal(ref, wlo, whi);
        for (int k = 0; k < 3; ++k) {
            lo[k] = visible ? refit_down(wlo[k]) : kHiddenNear;
            hi[k] = visible ? refit_up(whi[k]) : kHiddenFar;
        }
    }
    for (int k = 0; k < 3; ++k) { n.pnear[k][c] = lo[k]; n.pfar[k][c] = hi[k]; }
}

// One thread per listed node: octant copies 7..1 from copy 0, then copy 0 itself in its own order.
__global__ __launch_bounds__(256) void k_octant_copies(W4Node* nodes, const int32_t* list, int64_t count,
                                                       int64_t copy_nodes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    constexpr int mode = MYRT_WIDE_ORDER;
    const int64_t idx = list[i];
    const W4Node a = nodes[idx];
    for (int o = 7; o >= 0; --o) {
        double key[4];
        int perm[4] = {0, 1, 2, 3};
        for (int c = 0; c < 4; ++c) {
            if (!(a.pnear[0][c] < HUGE_VALF)) { key[c] = HUGE_VAL; continue; }
            double proj = 0.0;
            for (int ax = 0; ax < 3; ++ax) {
                const bool neg = (o >> ax) & 1;
                const double lo = a.pnear[ax][c], hi = a.pfar[ax][c];
                proj += mode == 1 ? (neg ? -hi : lo) : (neg ? -0.5 : 0.5) * (lo + hi);
            }
            key[c] = mode == 2 ? (double)c : proj;
        }
        for (int x = 1; x < 4; ++x)                           // stable insertion sort
            for (int y = x; y > 0 && key[perm[y]] < key[perm[y - 1]]; --y) {
                const int t = perm[y]; perm[y] = perm[y - 1]; perm[y - 1] = t;
            }
        W4Node w;
        for (int s = 0; s < 4; ++s) {
            const int c = perm[s];
            for (int ax = 0; ax < 3; ++ax) {
                const bool neg = (o >> ax) & 1;
                w.pnear[ax][s] = neg ? a.pfar[ax][c] : a.pnear[ax][c];
                w.pfar[ax][s] = neg ? a.pnear[ax][c] : a.pfar[ax][c];
            }
            w.ref[s] = a.ref[c];
            w.pad[s] = 0;
        }
        nodes[(size_t)o * copy_nodes + idx] = w;
    }
}

}  // namespace dev
}  // namespace myrt
