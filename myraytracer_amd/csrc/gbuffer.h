// gbuffer.h — first-hit buffers (rt_render_gbuffer, rtcore.h): per pixel of the
// selected chunks, the first primary ray the render casts through it and the record
// rt_query_closest returns for that ray.  Included by render.hip after query.h.  The walks are
// called unchanged, exactly as k_query_closest calls them, and the record is written by the same
// helper (query.h query_record), so a pixel's record is the query's record of the exported ray bit
// for bit and the exactness argument of the walks carries over with no new term.
//
// Only a pixel's FIRST sample is stated here: the draws of later samples follow the draws that
// shading consumes (glossy lobes, the lens), which only the render itself knows.
#pragma once

namespace myrt {
namespace dev {

// The outputs of the ray (each NULL = not written; the record's outputs travel in a QueryBatch) and
// the pixel-to-lane mapping of one launch.
struct GBufferBatch {
    double *o, *d, *tmin, *time;
    // tiles != 0: block b is the 8x8 tile xcd_tile(b) of the selected chunks (the render's mapping),
    // outputs at the rows RenderParams::out_first / out_step name.  tiles == 0: block b holds the 64
    // consecutive pixels from first + 64 b of the packed selection, [first, first + n) in all;
    // staged != 0 then indexes the outputs from `first` (a staging pass of a host-array call).
    int32_t tiles, staged;
    int32_t first, n;
    uint32_t centre;                 // RT_GBUFFER_PIXEL_CENTRE
};

// Sample (sx, sy) = (0, 0) of Object+Extension.swift:285-356 for pixel (i, j), term for term in
// render_kernel's operation order (render.hip; pixel_full states the same recipe), with the same
// helpers.  render_kernel and pixel_full keep their own inline copies: their register allocation
// is tuned line by line and they are not edited to call this.  `centre`: the deterministic ray
// through the pixel's centre, no lens offset, time 0, nothing drawn.
__device__ __forceinline__ void first_ray(const RenderParams& P, int i, int j, bool centre, V3& o, V3& d, double& tmin,
                                          double& time) {
    const DCamera& C = P.cam;
    PCG32 rng(pixel_seed(i, j));
    const V3 eye = ld3(C.eye), u = ld3(C.u), v = ld3(C.v), w = ld3(C.w), q00 = ld3(C.q00);
    const int n = C.n;
    double currentI, currentJ;
    if (centre) {
        currentI = (double)i + 0.5;
        currentJ = (double)j + 0.5;
    } else {
        const double xi1 = rng.nextFloat();
        const double xi2 = rng.nextFloat();
        const double iOffset = ((double)0 + xi1) / (double)n;
        const double jOffset = ((double)0 + xi2) / (double)n;
        currentI = (double)i + iOffset;
        currentJ = (double)j + jOffset;
    }
    const V3 vOff = v * (currentJ * C.dv);
    const V3 rowTopLeft = q00 - vOff;
    const V3 uOff = u * (currentI * C.du);
    const V3 sp = rowTopLeft + uOff;
    const V3 dir0 = normalize(sp - eye);
    V3 dir = dir0, camEye = eye;
    if (!centre && C.aperture > 0 && C.focus > 0) {          // DOF (:325-338)
        const V3 forward = -w;
        const double denom = dot(dir0, forward);
        const double tFocus = fabs(denom) < 1e-6 ? C.focus : (C.focus / denom);
        const V3 pFocus = eye + dir0 * tFocus;
        const double uRand = rng.nextFloat() - 0.5;
        const double vRand = rng.nextFloat() - 0.5;
        const V3 lensOffset = ((uRand * u) + (vRand * v)) * C.aperture;
        const V3 a = eye + lensOffset;
        dir = normalize(pFocus - a);
        camEye = a;
    }
    time = centre ? 0.0 : rng.nextFloat();
    const double denom = dot(dir, w);
    const double tImg = dot((eye - w * C.nd) - camEye, w) / (denom == 0.0 ? 4.9406564584124654e-324 : denom);
    tmin = smax(tImg, 0.0);
    o = camEye;
    d = dir;
}

// The lane's pixel and the index of its outputs; false = no pixel (a partial tile, the tail of the
// last block).  Everything but the lane is wave-uniform.
__device__ __forceinline__ bool gbuffer_pixel(const RenderParams& P, const GBufferBatch& G, int& i, int& j, size_t& at) {
    const int W = P.cam.width, lane = (int)(threadIdx.x & 63);
    if (G.tiles) {
        const int gx = (W + kTileW - 1) / kTileW;
        const int tile = xcd_tile((int)blockIdx.x, (int)gridDim.x, P.xcd_remap);
        const int chunk = P.chunk_first + (tile / gx) * P.chunk_step;
        i = (tile % gx) * kTileW + lane % kTileW;
        j = chunk * 8 + lane / kTileW;
        at = out_row_of(P, chunk, lane / kTileW) * (size_t)W + (size_t)i;
        return i < W && j < P.cam.height;
    }
    const int k = (int)(blockIdx.x * 64u) + lane;             // within [0, n)
    const int p = G.first + k, row = p / W;                   // packed selection: every chunk before the last has 8 rows
    const int chunk = P.chunk_first + (row >> 3) * P.chunk_step;
    i = p - row * W;
    j = chunk * 8 + (row & 7);
    at = G.staged ? (size_t)k : out_row_of(P, chunk, row & 7) * (size_t)W + (size_t)i;
    return k < G.n;
}
__device__ __forceinline__ void gbuffer_store_ray(const GBufferBatch& G, size_t at, const V3& o, const V3& d, double tmin,
                                                  double time) {
    if (G.o) { G.o[3 * at] = o.x; G.o[3 * at + 1] = o.y; G.o[3 * at + 2] = o.z; }
    if (G.d) { G.d[3 * at] = d.x; G.d[3 * at + 1] = d.y; G.d[3 * at + 2] = d.z; }
    if (G.tmin) G.tmin[at] = tmin;
    if (G.time) G.time[at] = time;
}

// One lane per pixel, one-wave blocks and the LDS stack slab, as k_query_closest (query.h), whose
// attributes this kernel carries: intersect_closest<false> is an out-of-line function whose
// register budget follows its least constrained caller, and this kernel must not become it.
template <int WALK>
__global__ __launch_bounds__(64) void k_gbuffer(RenderParams P, QueryBatch B, GBufferBatch G) {
    extern __shared__ unsigned long long lds_stack[];
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    int i, j;
    size_t at;
    if (gbuffer_pixel(P, G, i, j, at)) {
        V3 o, d;
        double tlo, time;
        first_ray(P, i, j, G.centre != 0u, o, d, tlo, time);
        gbuffer_store_ray(G, at, o, d, tlo, time);
        cls = query_finite(o, d) ? 0u : (uint32_t)RT_HIT_NON_FINITE;
        Hit h;
        h.t = DINF; h.inst = -1; h.tri = -1; h.u = 0; h.v = 0;
        if (cls == 0u && P.has_tlas) {
            if (WALK == kWalkGeneral) intersect_closest<false>(P, o, d, rcp(d), tlo, time, h, st, c);
            else walk_closest<false, WALK>(P, o, d, rcp(d), tlo, time, h, st, c);
        }
        hit = h.inst >= 0;
        query_record(P, B, at, o, d, time, h, hit, cls, c);
    }
    query_count(B, hit, cls);
}

// rt_render_gbuffer_masked: the kernel above with one ray mask for the whole call (QueryMasks::all),
// a kernel of its own as the masked queries are (query.h), so that k_gbuffer stays the code it was.
template <int WALK>
__global__ __launch_bounds__(64) void k_gbuffer_masked(RenderParams P, QueryBatch B, GBufferBatch G, QueryMasks K) {
    extern __shared__ unsigned long long lds_stack[];
    MYRT_STACK(st, lds_stack);
    Counts c{};
    bool hit = false;
    uint32_t cls = 0u;
    int i, j;
    size_t at;
    if (gbuffer_pixel(P, G, i, j, at)) {
        V3 o, d;
        double tlo, time;
        first_ray(P, i, j, G.centre != 0u, o, d, tlo, time);
        gbuffer_store_ray(G, at, o, d, tlo, time);
        cls = query_finite(o, d) ? 0u : (uint32_t)RT_HIT_NON_FINITE;
        const RayMask mk{K.table, K.all};
        Hit h;
        h.t = DINF; h.inst = -1; h.tri = -1; h.u = 0; h.v = 0;
        if (cls == 0u && P.has_tlas && mk.any()) walk_closest<false, WALK>(P, o, d, rcp(d), tlo, time, h, st, c, mk);
        hit = h.inst >= 0;
        query_record(P, B, at, o, d, time, h, hit, cls, c);
    }
    query_count(B, hit, cls);
}

// Rays only (no record pointer set): no stack, no LDS, none of a walk's registers.
constexpr int kGBufferRaysBlock = 256;
__global__ __launch_bounds__(kGBufferRaysBlock) void k_gbuffer_rays(RenderParams P, GBufferBatch G) {
    const int k = (int)(blockIdx.x * (unsigned)kGBufferRaysBlock + threadIdx.x);
    if (k >= G.n) return;
    const int W = P.cam.width;
    const int p = G.first + k, row = p / W;
    const int chunk = P.chunk_first + (row >> 3) * P.chunk_step;
    const int i = p - row * W, j = chunk * 8 + (row & 7);
    const size_t at = G.staged ? (size_t)k : out_row_of(P, chunk, row & 7) * (size_t)W + (size_t)i;
    V3 o, d;
    double tmin, time;
    first_ray(P, i, j, G.centre != 0u, o, d, tmin, time);
    gbuffer_store_ray(G, at, o, d, tmin, time);
}

}  // namespace dev
}  // namespace myrt
