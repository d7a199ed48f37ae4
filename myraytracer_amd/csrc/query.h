// query.h — ray queries (rt_query_closest / rt_query_occluded, rtcore.h): the
// scene's production walks on caller-given rays in device memory, one lane per ray, with full hit
// records.  Included by render.hip after walk_closest / walk_occluded, which are called unchanged:
// a query ray takes exactly the path a render ray of the same scene takes, so the exactness
// argument of the walks (wide.h) carries over with no new term.  What is new is
// where the three per-batch maxima that size the pruning margin and the widening come from:
// k_ray_bounds reduces them on the device (or the caller declares them and every ray is compared
// against the declaration before it is traced).
#pragma once

namespace myrt {
namespace dev {

// QueryBatch::mask: optional inputs resolved once per launch on the host.  The mask is a kernel
// argument (an SGPR), so each test is a scalar branch, not a per-lane load of a pointer.
constexpr uint32_t kQHasTlim = 1u, kQHasTime = 2u, kQCheck = 4u;
// The slot's query words (device, u64): the three maxima of k_ray_bounds as the bits of
// non-negative doubles (which order as unsigned integers), then the counters of the last query.
constexpr int kQWordReach = 0, kQWordCoord = 1, kQWordNorm = 2, kQWordHits = 3, kQWordOob = 4, kQWordNonFinite = 5;
constexpr int kQWords = 8;

struct QueryBatch {
    const double *o, *d, *tlim, *time;        // this launch's rays (tlim / time: see mask)
    double *t, *uv, *point, *normal;          // outputs, each NULL = not written
    int32_t* ids;
    uint8_t* flags;
    uint8_t* occ;                             // k_query_occluded
    const int32_t *face, *inst_obj;           // face table (with ids only)
    unsigned long long* words;
    double center[3];                         // scene centre (origin_reach is measured from it)
    double reach, coord, norm;                // declared bounds (kQCheck)
    int32_t n;
    uint32_t mask;
};

// The masks of a launch (rt_query_*_masked, rt_render_gbuffer_masked), a kernel
// argument of its own next to QueryBatch::mask: the scene's instance-mask table (NULL until masks
// are first set: every instance all-ones) and the rays' masks, one per ray of this launch or `all`.
// at(i) is ray i's policy for the walks (device.h RayMask).
struct QueryMasks {
    const uint32_t *table, *per_ray;
    uint32_t all, pad;
    __device__ __forceinline__ RayMask at(size_t i) const { return RayMask{table, per_ray ? per_ray[i] : all}; }
};

// 0: trace the ray; RT_HIT_NON_FINITE / RT_HIT_OUT_OF_BOUNDS: report it untraced.  The three
// magnitudes are formed term for term as the host forms a camera's (render.hip dist_to_center,
// make_params).
__device__ __forceinline__ bool query_finite(const V3& o, const V3& d) {
    return isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z);
}
__device__ __forceinline__ void query_magnitudes(const V3& o, const V3& d, double cx, double cy, double cz,
                                                 double& reach, double& coord, double& norm) {
    double s = 0.0;
    s += (o.x - cx) * (o.x - cx); s += (o.y - cy) * (o.y - cy); s += (o.z - cz) * (o.z - cz);
    reach = sqrt(s);
    coord = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z)));
    norm = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
}
__device__ __forceinline__ uint32_t query_class(const QueryBatch& B, const V3& o, const V3& d) {
    if (!query_finite(o, d)) return RT_HIT_NON_FINITE;
    if (B.mask & kQCheck) {
        double reach, coord, norm;
        query_magnitudes(o, d, B.center[0], B.center[1], B.center[2], reach, coord, norm);
        if (!(reach <= B.reach) || !(coord <= B.coord) || !(norm <= B.norm)) return RT_HIT_OUT_OF_BOUNDS;
    }
    return 0u;
}
__device__ __forceinline__ void query_count(const QueryBatch& B, bool hit, uint32_t cls) {
    const unsigned long long nh = wave_sum(hit ? 1ull : 0ull), no = wave_sum(cls == RT_HIT_OUT_OF_BOUNDS ? 1ull : 0ull),
                             nf = wave_sum(cls == RT_HIT_NON_FINITE ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0) {
        if (nh) atomicAdd(&B.words[kQWordHits], nh);
        if (no) atomicAdd(&B.words[kQWordOob], no);
        if (nf) atomicAdd(&B.words[kQWordNonFinite], nf);
    }
}

// The record of one traced ray, written at index i of the batch's outputs (each NULL = not written):
// shared by k_query_closest and k_gbuffer (gbuffer.h), whose records are the same by construction.
__device__ __forceinline__ void query_record(const RenderParams& P, const QueryBatch& B, size_t i, const V3& o,
                                             const V3& d, double time, const Hit& h, bool hit, uint32_t cls, Counts& c) {
    const size_t i3 = 3 * i;
    if (B.t) B.t[i] = hit ? h.t : DINF;
    if (B.uv) {
        const bool tri = hit && P.insts[h.inst].kind == kPrimTriangles;
        B.uv[2 * i] = tri ? h.u : 0.0;
        B.uv[2 * i + 1] = tri ? h.v : 0.0;
    }
    if (B.ids) {
        int32_t* q = B.ids + 4 * i;
        q[0] = hit ? B.inst_obj[h.inst] : -1;
        q[1] = hit ? B.face[h.tri] : -1;
        q[2] = hit ? h.inst : -1;
        q[3] = hit ? P.insts[h.inst].material : -1;
    }
    if (B.point || B.normal) {
        V3 p = v3(0, 0, 0), n = v3(0, 0, 0);
        if (hit) hit_geometry<false>(P, o, d, time, h, p, n, c);
        if (B.point) { B.point[i3] = p.x; B.point[i3 + 1] = p.y; B.point[i3 + 2] = p.z; }
        if (B.normal) { B.normal[i3] = n.x; B.normal[i3 + 1] = n.y; B.normal[i3 + 2] = n.z; }
    }
    if (B.flags) B.flags[i] = (uint8_t)((hit ? RT_HIT_VALID : 0u) | cls);
}

// One-wave blocks, as the render kernels (render.hip kRenderBlock): a block's LDS stack slab is
// released when its slowest wave ends, and walk lengths of unrelated rays vary widely.
template <int WALK>
__global__ __launch_bounds__(64) void k_query_closest(RenderParams P, QueryBatch B) {
    extern __shared__ unsigned long long lds_stack[];
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    if (i < B.n) {
        const size_t i3 = 3 * (size_t)i;
        const V3 o = v3(B.o[i3], B.o[i3 + 1], B.o[i3 + 2]), d = v3(B.d[i3], B.d[i3 + 1], B.d[i3 + 2]);
        const double time = (B.mask & kQHasTime) ? B.time[i] : 0.0;
        cls = query_class(B, o, d);
        Hit h;
        h.t = DINF; h.inst = -1; h.tri = -1; h.u = 0; h.v = 0;
        if (cls == 0u && P.has_tlas) {
            const double tlo = (B.mask & kQHasTlim) ? B.tlim[i] : 0.0;
            if (WALK == kWalkGeneral) intersect_closest<false>(P, o, d, rcp(d), tlo, time, h, st, c);
            else walk_closest<false, WALK>(P, o, d, rcp(d), tlo, time, h, st, c);
        }
        hit = h.inst >= 0;
        query_record(P, B, (size_t)i, o, d, time, h, hit, cls, c);
    }
    query_count(B, hit, cls);
}

template <int WALK>
__global__ __launch_bounds__(64) void k_query_occluded(RenderParams P, QueryBatch B) {
    extern __shared__ unsigned long long lds_stack[];
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    if (i < B.n) {
        const size_t i3 = 3 * (size_t)i;
        const V3 o = v3(B.o[i3], B.o[i3 + 1], B.o[i3 + 2]), d = v3(B.d[i3], B.d[i3 + 1], B.d[i3 + 2]);
        cls = query_class(B, o, d);
        if (cls == 0u) {
            const double tmax = (B.mask & kQHasTlim) ? B.tlim[i] : DINF;
            const double time = (B.mask & kQHasTime) ? B.time[i] : 0.0;
            if (WALK == kWalkIdentity) hit = uni_occluded<false>(P, o, d, tmax, st, c);
            else if (WALK == kWalkGeneral) hit = occluded<false>(P, o, d, tmax, time, st, c);
            else hit = walk_occluded<false, WALK, true, false>(P, o, d, tmax, time, st, c);
        }
        B.occ[i] = cls ? (uint8_t)2 : (hit ? (uint8_t)1 : (uint8_t)0);
    }
    query_count(B, hit, cls);
}

// The masked queries (rt_query_closest_masked / rt_query_occluded_masked): the two kernels above with
// ray i's mask handed to the walk.  They are kernels of their own, not a parameter of the ones above,
// so the unmasked kernels stay the code they were: same attributes, same helpers, and a ray whose
// mask is 0 sees nothing and is not walked (a miss, not flagged, counted as traced).
template <int WALK>
__global__ __launch_bounds__(64) void k_query_closest_masked(RenderParams P, QueryBatch B, QueryMasks K) {
    extern __shared__ unsigned long long lds_stack[];
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    if (i < B.n) {
        const size_t i3 = 3 * (size_t)i;
        const V3 o = v3(B.o[i3], B.o[i3 + 1], B.o[i3 + 2]), d = v3(B.d[i3], B.d[i3 + 1], B.d[i3 + 2]);
        const double time = (B.mask & kQHasTime) ? B.time[i] : 0.0;
        cls = query_class(B, o, d);
        const RayMask mk = K.at((size_t)i);
        Hit h;
        h.t = DINF; h.inst = -1; h.tri = -1; h.u = 0; h.v = 0;
        if (cls == 0u && P.has_tlas && mk.any()) {
            const double tlo = (B.mask & kQHasTlim) ? B.tlim[i] : 0.0;
            walk_closest<false, WALK>(P, o, d, rcp(d), tlo, time, h, st, c, mk);
        }
        hit = h.inst >= 0;
        query_record(P, B, (size_t)i, o, d, time, h, hit, cls, c);
    }
    query_count(B, hit, cls);
}
template <int WALK>
__global__ __launch_bounds__(64) void k_query_occluded_masked(RenderParams P, QueryBatch B, QueryMasks K) {
    extern __shared__ unsigned long long lds_stack[];
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    if (i < B.n) {
        const size_t i3 = 3 * (size_t)i;
        const V3 o = v3(B.o[i3], B.o[i3 + 1], B.o[i3 + 2]), d = v3(B.d[i3], B.d[i3 + 1], B.d[i3 + 2]);
        cls = query_class(B, o, d);
        const RayMask mk = K.at((size_t)i);
        if (cls == 0u && mk.any()) {
            const double tmax = (B.mask & kQHasTlim) ? B.tlim[i] : DINF;
            const double time = (B.mask & kQHasTime) ? B.time[i] : 0.0;
            hit = walk_occluded<false, WALK, true, false>(P, o, d, tmax, time, st, c, mk);
        }
        B.occ[i] = cls ? (uint8_t)2 : (hit ? (uint8_t)1 : (uint8_t)0);
    }
    query_count(B, hit, cls);
}

// The three maxima of a batch over its finite rays, one pass: per lane over a grid-stride run of
// rays, then the wave (wave_max on the doubles' bits: non-negative doubles order as unsigned
// integers), the block through LDS, and one integer atomicMax per block and word.  No
// floating-point atomic; max is exact, so the order of the reduction does not show in the result.
constexpr int kRayBoundsBlock = 256;
__global__ __launch_bounds__(kRayBoundsBlock) void k_ray_bounds(const double* o, const double* d, int64_t n, double cx,
                                                             double cy, double cz, unsigned long long* words) {
    __shared__ unsigned long long part[kRayBoundsBlock / 64][3];
    double reach = 0.0, coord = 0.0, norm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kRayBoundsBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRayBoundsBlock) {
        const V3 oo = v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        if (!query_finite(oo, dd)) continue;
        double r, cc, nn;
        query_magnitudes(oo, dd, cx, cy, cz, r, cc, nn);
        reach = fmax(reach, r); coord = fmax(coord, cc); norm = fmax(norm, nn);
    }
    const unsigned long long w0 = wave_max((unsigned long long)__double_as_longlong(reach)),
                             w1 = wave_max((unsigned long long)__double_as_longlong(coord)),
                             w2 = wave_max((unsigned long long)__double_as_longlong(norm));
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = w0; part[wave][1] = w1; part[wave][2] = w2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long m = part[0][threadIdx.x];
        for (int w = 1; w < kRayBoundsBlock / 64; ++w) m = part[w][threadIdx.x] > m ? part[w][threadIdx.x] : m;
        if (m) atomicMax(&words[threadIdx.x], m);
    }
}

}  // namespace dev
}  // namespace myrt
