// deform.h — device side of deforming meshes (rt_scene_set_mesh_positions + rt_scene_commit on a
// scene created with RT_SCENE_DEFORMABLE): new vertex positions, the BLAS refit where the triangles
// live.  BVHBuilder.refit(using:) (RayTracer/Accelearion/BVH.swift:254-291, "bottom-up AABB
// update") applied to a BLAS: topology, leaf runs and primitive order are kept, a leaf's box is the
// min / max over its primitives' bounds and an inner node's the union of its children's.
//
//   k_deform_validate (+ _final)  one staged position array -> (all finite, largest |coordinate|):
//       FP64, wave shuffles, one partial per block, a final pass (refit.h's reduction order).
//       The whole array is read: a NaN in a vertex no triangle uses is refused too.
//   k_deform_tris      one thread per TriRec of the BLAS's run: v0, e1 = v1 - v0, e2 = v2 - v0 (the
//       builder's expressions, scene.cpp "independent per triangle"), the triangle's exact box
//       (pbox), flat normals normalize(normalize(cross(e1, e2))) as the builder applies normalize
//       twice, the unit face normal by the mesh's own triangle index for derived smooth normals,
//       and the block's largest |e1||e2| (the pruning margin's constant, scene.cpp blasP).
//   k_vertex_normals   derived smooth normals: one thread per vertex adds the unit face normals of
//       its incident corners in ascending triangle order from (0, 0, 0) - the builder's serial loop
//       seen from one vertex, so the sums and their normalisation have the builder's bits.
//   k_gather_normals   per TriRec the three vertex normals (derived, or newly supplied ones).
//   k_leaf_boxes       lbox[6 * first] of every leaf run (scenes with four-wide trees): the run is
//       walked to its `last` flag (a run can hold more than two triangles).
//   k_refit_recs       one level of the BLAS's WRec records, deepest first: child slot c takes its
//       leaf run's box (ref < 0) or the union of record ref[c]'s two child boxes.  Pure min / max.
//   k_blas_root        the BLAS root box (DInstance::root_lo / root_hi, DWideInst::bcoord) and the
//       reduced |e1||e2|, read back by the host.
//   The BLAS's four-wide nodes are refit level by level by refit.h k_refit_level<LeafRunBox>, its
//       eight copies restated by k_octant_copies.
//
// Why the hits stay the reference's: the four-wide trees only have to be supersets (wide.h), and a
// refit tree is one.  A candidate is accepted only after the reference's exact FP64 tests against
// the leaf boxes (lbox, the WRec leaf boxes), the BLAS root box and the TLAS leaf box, all of which
// are recomputed here and in rt_scene_commit as plain FP64 min / max, i.e. as the values
// BVHBuilder.refit holds for the kept topology.  The premises of the widening (bcoord, wide_coord,
// fit_coord) and of the pruning margin (blasP) are recomputed, not inherited from the build.  What
// differs from a fresh build is the order in which equal-t ties are re-walked: the kept tree's,
// as in the reference's own refit.
//
// Built with -ffp-contract=off like refit.h; sqrt and divide are IEEE correctly rounded, so the
// normals equal the host builder's bit for bit.  All stores are ordinary vector stores and there
// is no floating-point atomic: results are deterministic and replicas end identical.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "layout.h"
#include "refit.h"
#include "scene.h"

namespace myrt {
namespace dev {

constexpr int kDeformBlock = 256;
constexpr int kValidateParts = 256;       // blocks of k_deform_validate (grid-stride)

struct DeformMesh {
    const double* pos;        // staged positions, xyz per vertex
    const int32_t* vid;       // 3 per TriRec (whole scene)
    int32_t tri_first, tri_end;
    int32_t prim_base;
    int32_t normals;          // kNormalsFlat / Supplied / Smooth
};

// scene.cpp dot / cross / normalize, term for term
__device__ __forceinline__ double df_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void df_cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void df_normalize(const double v[3], double o[3]) {
    const double r = 1.0 / sqrt(df_dot(v, v));
    o[0] = v[0] * r; o[1] = v[1] * r; o[2] = v[2] * r;
}

// Block b: a grid-stride share of the n doubles -> partial[2b] = 1.0 if all finite, else 0.0;
// partial[2b + 1] = their largest magnitude
__global__ __launch_bounds__(kDeformBlock) void k_deform_validate(const double* x, int64_t n, double* partial) {
    double ok = 1.0, mx = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kDeformBlock;
    for (int64_t i = (int64_t)blockIdx.x * kDeformBlock + threadIdx.x; i < n; i += stride) {
        const double a = fabs(x[i]);
        if (!(a < HUGE_VAL)) ok = 0.0;                    // NaN or infinite
        mx = fmax(mx, a);
    }
    ok = wave_fmin(ok);
    mx = wave_fmax(mx);
    __shared__ double sm[kDeformBlock / 64][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { sm[wave][0] = ok; sm[wave][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDeformBlock / 64; ++w) { ok = fmin(ok, sm[w][0]); mx = fmax(mx, sm[w][1]); }
        partial[2 * blockIdx.x] = ok;
        partial[2 * blockIdx.x + 1] = mx;
    }
}
__global__ __launch_bounds__(64) void k_deform_validate_final(const double* partial, int parts, double* out) {
    double ok = 1.0, mx = 0.0;
    for (int p = threadIdx.x; p < parts; p += 64) { ok = fmin(ok, partial[2 * p]); mx = fmax(mx, partial[2 * p + 1]); }
    ok = wave_fmin(ok);
    mx = wave_fmax(mx);
    if (threadIdx.x == 0) { out[0] = ok; out[1] = mx; }
}

// One thread per TriRec of the run; ppart[blockIdx.x] = the block's largest |e1||e2|.
__global__ __launch_bounds__(kDeformBlock) void k_deform_tris(DeformMesh M, TriRec* tris, double* pbox, double* normals,
                                                              double* face_n, double* ppart) {
    const int64_t q = (int64_t)M.tri_first + (int64_t)blockIdx.x * kDeformBlock + threadIdx.x;
    double p = 0.0;
    if (q < (int64_t)M.tri_end) {
        double v[3][3], e1[3], e2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t id = M.vid[3 * q + c];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[c][k] = M.pos[3 * id + k];
        }
        TriRec& t = tris[q];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e1[k] = v[1][k] - v[0][k];
            e2[k] = v[2][k] - v[0][k];
            t.v0[k] = v[0][k]; t.e1[k] = e1[k]; t.e2[k] = e2[k];
            pbox[6 * q + k] = fmin(v[0][k], fmin(v[1][k], v[2][k]));
            pbox[6 * q + 3 + k] = fmax(v[0][k], fmax(v[1][k], v[2][k]));
        }
        p = sqrt(df_dot(e1, e1)) * sqrt(df_dot(e2, e2));
        if (M.normals != kNormalsSupplied) {
            double c[3], f[3];
            df_cross(e1, e2, c);
            df_normalize(c, f);
            if (M.normals == kNormalsSmooth) {
                double* o = face_n + 3 * (int64_t)(t.prim - M.prim_base);
                o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
            } else {
                double n[3];
                df_normalize(f, n);
#pragma unroll
                for (int c3 = 0; c3 < 3; ++c3)
#pragma unroll
                    for (int k = 0; k < 3; ++k) normals[9 * q + 3 * c3 + k] = n[k];
            }
        }
    }
    p = wave_fmax(p);
    __shared__ double sm[kDeformBlock / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDeformBlock / 64; ++w) p = fmax(p, sm[w]);
        ppart[blockIdx.x] = p;
    }
}

// One thread per vertex: csr_off[v] .. csr_off[v + 1] index csr_tri (the mesh's own triangle indices)
__global__ __launch_bounds__(kDeformBlock) void k_vertex_normals(const int32_t* csr_off, const int32_t* csr_tri, int64_t verts,
                                                                 const double* face_n, double* vnorm) {
    const int64_t v = (int64_t)blockIdx.x * kDeformBlock + threadIdx.x;
    if (v >= verts) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int32_t e = csr_off[v], end = csr_off[v + 1]; e < end; ++e) {
        const double* f = face_n + 3 * (int64_t)csr_tri[e];
        acc[0] = acc[0] + f[0]; acc[1] = acc[1] + f[1]; acc[2] = acc[2] + f[2];
    }
    double n[3];
    df_normalize(acc, n);
    vnorm[3 * v] = n[0]; vnorm[3 * v + 1] = n[1]; vnorm[3 * v + 2] = n[2];
}

// One thread per TriRec of the run: its normal triple from a per-vertex array
__global__ __launch_bounds__(kDeformBlock) void k_gather_normals(const int32_t* vid, int32_t tri_first, int32_t tri_end,
                                                                 const double* src, double* normals) {
    const int64_t q = (int64_t)tri_first + (int64_t)blockIdx.x * kDeformBlock + threadIdx.x;
    if (q >= (int64_t)tri_end) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t id = vid[3 * q + c];
#pragma unroll
        for (int k = 0; k < 3; ++k) normals[9 * q + 3 * c + k] = src[3 * id + k];
    }
}

struct DeformRun {            // what a leaf run's box needs
    const TriRec* tris;
    const double* pbox;
    int32_t tri_end;          // the BLAS's run end (a guard: `last` always comes first)
    int32_t blur;
    double motion[3];
};
// The box of the leaf run starting at TriRec `first`: min / max over its triangles' bounds, a
// blurred mesh's also covering the triangle moved by the motion vector (scene.cpp "independent per
// triangle": min over the three v + m equals min(v) + m, rounding being monotone)
__device__ __forceinline__ void leaf_run_box(const DeformRun& R, int64_t first, double lo[3], double hi[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = HUGE_VAL; hi[k] = -HUGE_VAL; }
    for (int64_t t = first; t < (int64_t)R.tri_end; ++t) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double a = R.pbox[6 * t + k], b = R.pbox[6 * t + 3 + k];
            if (R.blur) { a = fmin(a, a + R.motion[k]); b = fmax(b, b + R.motion[k]); }
            lo[k] = fmin(lo[k], a);
            hi[k] = fmax(hi[k], b);
        }
        if (R.tris[t].last) break;
    }
}

// One thread per TriRec of the run; the thread of a leaf run's first triangle writes lbox[6 * first]
__global__ __launch_bounds__(kDeformBlock) void k_leaf_boxes(DeformRun R, int32_t tri_first, double* lbox) {
    const int64_t q = (int64_t)tri_first + (int64_t)blockIdx.x * kDeformBlock + threadIdx.x;
    if (q >= (int64_t)R.tri_end) return;
    if (q != (int64_t)tri_first && !R.tris[q - 1].last) return;
    double lo[3], hi[3];
    leaf_run_box(R, q, lo, hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) { lbox[6 * q + k] = lo[k]; lbox[6 * q + 3 + k] = hi[k]; }
}

__device__ __forceinline__ void rec_child_box(const WRec* recs, const DeformRun& R, int32_t ref, double lo[3], double hi[3]) {
    if (ref < 0) { leaf_run_box(R, (int64_t)~ref, lo, hi); return; }
    const WRec& ch = recs[ref];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fmin(ch.lo[0][k], ch.lo[1][k]); hi[k] = fmax(ch.hi[0][k], ch.hi[1][k]); }
}

// One thread per child slot of the level's records
__global__ __launch_bounds__(kDeformBlock) void k_refit_recs(WRec* recs, const int32_t* list, int32_t count, DeformRun R) {
    const int64_t i = (int64_t)blockIdx.x * kDeformBlock + threadIdx.x;
    if (i >= 2 * (int64_t)count) return;
    WRec& r = recs[list[i >> 1]];
    const int c = (int)(i & 1);
    double lo[3], hi[3];
    rec_child_box(recs, R, r.ref[c], lo, hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.lo[c][k] = lo[k]; r.hi[c][k] = hi[k]; }
}

// One wave: out[0..5] = the BLAS root box, out[6] = max of the `parts` |e1||e2| partials
__global__ __launch_bounds__(64) void k_blas_root(const WRec* recs, int32_t root_ref, DeformRun R, const double* ppart, int parts,
                                                  double* out) {
    double p = 0.0;
    for (int q = threadIdx.x; q < parts; q += 64) p = fmax(p, ppart[q]);
    p = wave_fmax(p);
    if (threadIdx.x != 0) return;
    double lo[3], hi[3];
    rec_child_box(recs, R, root_ref, lo, hi);
    for (int k = 0; k < 3; ++k) { out[k] = lo[k]; out[3 + k] = hi[k]; }
    out[6] = p;
    out[7] = 0.0;
}

}  // namespace dev
}  // namespace myrt
