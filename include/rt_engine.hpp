/*
 * rt_engine.hpp — C++17 host mirror of the reference's public engine API over the C ABI
 * (include/rtcore.h).  Header-only; link with -lmyrt.
 *
 * The reference's host is Swift (`public final class RayTracerEngine`,
 * Sources/RayTracer/RayTracer.swift:25-228), which cannot run on Linux.  This is the same
 * surface for compiled C++ hosts, with the same names, argument meaning and error
 * behaviour:
 *
 *   RayTracerEngine(scene)          <- init(from:data:) after SceneLoader.load      RayTracer.swift:30-49
 *   inspect()                       <- inspect(scene:format:)                       RayTracer.swift:52-67
 *   render(format, cameraIndex, p)  <- render(format:cameraIndex:progress:)         RayTracer.swift:115-131
 *   renderAll(p)                    <- renderAll(progress:)                         RayTracer.swift:70-102
 *   RenderResult / RenderStats / RenderProgress / CameraSpec / SceneInfo            Models/*.swift
 *   RenderError{code}               <- NSError(domain:"Render"/"Ray", code: -10/-20/-21)
 *
 * Differences, all deliberate: RenderResult carries the RGBA8 pixels (and the FP64
 * [Vec3] buffer Renderer.render returns) instead of a CGImage; RenderStats.rays is the
 * number of primary + shadow rays actually cast (the reference always reported 0,
 * RayTracer.swift:167,200) and milliseconds is a double; returning false from the
 * progress callback really cancels (RT_ERR_CANCELLED; the reference's cancel was a
 * no-op on an unstructured task).  Scene files are decoded by the host (ParsingKit's
 * role); this class takes the decoded scene as an rt_scene_desc.
 */
#ifndef MYRT_RT_ENGINE_HPP
#define MYRT_RT_ENGINE_HPP

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rtcore.h"

namespace myrt {

/* NSError equivalent: `code` is the rtcore status (-10 invalid camera, -20 no scene,
 * -21 renderer not initialised, -50 device, -60 cancelled, ...). */
class RenderError : public std::runtime_error {
public:
    RenderError(int32_t code, const std::string& msg)
        : std::runtime_error("[" + std::to_string(code) + "] " + msg), code(code) {}
    int32_t code;
};

inline void check(int32_t rc) {
    if (rc != RT_OK) {
        const char* m = rt_last_error();
        throw RenderError(rc, m ? m : "");
    }
}

enum class SceneFormat { Auto, Json, Xml };           /* Models/SceneFormat.swift:8-10 */

struct RenderProgress {                                 /* Models/RenderProgress.swift:8-14 */
    double fraction;                                    /* 0...1 */
    std::string message;
};

struct RenderStats {                                    /* Models/RenderStats.swift:8-24 */
    int64_t meshes = 0, triangles = 0, spheres = 0, planes = 0;
    int64_t rays = 0;                                   /* primary + shadow */
    int64_t primary_rays = 0, shadow_rays = 0, secondary_rays = 0;
    int64_t shadow_rays_traced = 0;                     /* any-hit walks that ran (<= shadow_rays) */
    int64_t rewalked = 0;                               /* closest-hit rays re-walked in reference order (ties) */
    double milliseconds = 0, kernel_ms = 0;
};

struct CameraSpec {                                     /* Models/RenderConfig.swift:19-25 */
    int32_t index = 0;
    std::string id, imageName;
    int32_t width = 0, height = 0;
};

struct SceneInfo {                                      /* Models/RenderConfig.swift:27-33 */
    std::vector<CameraSpec> cameras;
    int64_t meshes = 0, triangles = 0, spheres = 0, planes = 0;
};

struct RenderResult {                                   /* Models/RenderResult.swift:10-15 */
    std::string fileName;
    std::vector<uint8_t> rgba8;                         /* H*W*4, row 0 = top (RayTracer.swift:186-195) */
    std::vector<double> rgb;                            /* H*W*3, Renderer.render's [Vec3] */
    CameraSpec camera;
    RenderStats stats;
};

/* Camera metadata the C ABI does not carry (Camera.id / imageName). */
struct CameraMeta {
    std::string id, imageName;
};

using ProgressFn = std::function<bool(const RenderProgress&)>;

class RayTracerEngine {
public:
    /* Builds the scene on the host (PLY, flattening, SAH BVH) and uploads a replica to
     * every listed device (empty = device 0).  The descriptor is copied.  dynamic: instances and
     * cameras may move between renders (setTransform / setCamera / commit; RT_SCENE_DYNAMIC). */
    explicit RayTracerEngine(const rt_scene_desc& desc, std::vector<int32_t> devices = {},
                             std::vector<CameraMeta> cameraMeta = {}, bool dynamic = false, bool deformable = false)
        : meta_(std::move(cameraMeta)) {
        for (int32_t i = 0; i < desc.num_cameras; ++i) cams_.push_back(desc.cameras[i]);
        check(rt_scene_create_ex(&desc, devices.empty() ? nullptr : devices.data(), (int32_t)devices.size(),
                                 (dynamic ? RT_SCENE_DYNAMIC : 0u) | (deformable ? RT_SCENE_DEFORMABLE : 0u), &scene_));
    }
    /* RayTracerEngine.init(from: url) / init(data:) (RayTracer.swift:30-49): the scene file is
     * decoded by rt_scene_file_* (JSON or XML, ParsingKit's conventions), then built like the
     * descriptor constructor.  Throws RenderError(RT_ERR_SCENE_FILE) on a decode error. */
    static RayTracerEngine fromFile(const std::string& path, SceneFormat format = SceneFormat::Auto,
                                    std::vector<int32_t> devices = {}) {
        rt_scene_file* f = nullptr;
        if (const int32_t rc = rt_scene_file_load(path.c_str(), fileFormat(format), &f))
            throw RenderError(rc, rt_scene_file_last_error());
        return fromSceneFile(f, std::move(devices));
    }
    static RayTracerEngine fromData(const std::string& data, SceneFormat format = SceneFormat::Auto,
                                    const std::string& baseDir = "", std::vector<int32_t> devices = {}) {
        rt_scene_file* f = nullptr;
        if (const int32_t rc = rt_scene_file_parse(data.data(), data.size(), fileFormat(format),
                                                   baseDir.empty() ? nullptr : baseDir.c_str(), &f))
            throw RenderError(rc, rt_scene_file_last_error());
        return fromSceneFile(f, std::move(devices));
    }
    ~RayTracerEngine() { if (scene_) rt_scene_destroy(scene_); }
    RayTracerEngine(const RayTracerEngine&) = delete;
    RayTracerEngine& operator=(const RayTracerEngine&) = delete;
    RayTracerEngine(RayTracerEngine&& o) noexcept : scene_(o.scene_), cams_(std::move(o.cams_)), meta_(std::move(o.meta_)) {
        o.scene_ = nullptr;
    }

    rt_scene* handle() const { return scene_; }

    /* Render options (rt_scene_set_option; defaults are the production settings). */
    void setOption(const std::string& name, int64_t value) { check(rt_scene_set_option(scene_, name.c_str(), value)); }
    /* Test hooks (rt_scene_set_unsafe_option: not for production, rtcore.h). */
    void setUnsafeOption(const std::string& name, int64_t value) {
        check(rt_scene_set_unsafe_option(scene_, name.c_str(), value));
    }
    int64_t option(const std::string& name) const {
        int64_t v = 0;
        check(rt_scene_get_option(scene_, name.c_str(), &v));
        return v;
    }

    /* Dynamic scenes: RTContext.refitTLAS() (RTContext.swift:883-927).  instanceOf: the instance
     * scene object `objectIndex` produced (-1: none).  setTransform stages a column-major
     * localToWorld for that instance until commit(); setCamera replaces a camera at once; commit()
     * refits every acceleration structure on every replica and blocks until they are updated.
     * commit and setCamera throw RenderError(RT_ERR_BUSY) while a submitted render has not been
     * waited for; setTransform and commit throw RT_ERR_UNSUPPORTED on an engine built without
     * `dynamic`. */
    int32_t instanceOf(int32_t objectIndex) const {
        int32_t k = -1;
        check(rt_scene_instance_of_object(scene_, objectIndex, &k));
        return k;
    }
    void setTransform(int32_t objectIndex, const double m[16]) {
        const int32_t k = instanceOf(objectIndex);
        if (k < 0) throw RenderError(RT_ERR_INVALID_ARG, "the object produced no instance");
        check(rt_scene_set_instance_transform(scene_, k, m));
    }
    void setCamera(int32_t index, const rt_camera& camera) {
        check(rt_scene_set_camera(scene_, index, &camera));
        cams_.at((size_t)index) = camera;
    }
    /* commit(true) also builds the flattened instance tree again on the device for the new pose
     * (RT_COMMIT_REBUILD_FIT); lastRebuildStats() says what the last commit did for it.
     * A commit that throws RT_ERR_INVALID_ARG or RT_ERR_OOM changed nothing (what was staged is
     * dropped, the last*Stats() keep the last successful commit's); without memory for a rebuild it
     * returns normally with lastRebuildStats().reason == RT_REBUILD_NO_MEMORY and the old tree refit;
     * a commit that throws RT_ERR_DEVICE lost the scene: every later render, submit, query, commit,
     * fitCost and read-back of this engine throws RT_ERR_DEVICE too - destroy it and build a new one
     * (rtcore.h "how a commit ends"). */
    rt_commit_stats commit(bool rebuild = false) {
        rt_commit_stats st{};
        check(rebuild ? rt_scene_commit_ex(scene_, RT_COMMIT_REBUILD_FIT, &st) : rt_scene_commit(scene_, &st));
        return st;
    }
    rt_rebuild_stats lastRebuildStats() const {
        rt_rebuild_stats st{};
        check(rt_scene_last_rebuild_stats(scene_, &st));
        return st;
    }
    /* commitEx(RT_COMMIT_REBUILD_FIT_CLUSTERED) rebuilds with the clustered builder; lastRebuildDetail()
     * says which builder made the tree and what it cost before and after; fitCost() is the cost of
     * the tree in use now (lower is better; 0 without such a tree). */
    rt_commit_stats commitEx(uint32_t flags) {
        rt_commit_stats st{};
        check(rt_scene_commit_ex(scene_, flags, &st));
        return st;
    }
    rt_rebuild_detail lastRebuildDetail() const {
        rt_rebuild_detail st{};
        check(rt_scene_last_rebuild_detail(scene_, &st));
        return st;
    }
    double fitCost() {
        double c = 0.0;
        check(rt_scene_fit_cost(scene_, &c));
        return c;
    }
    /* Instance visibility (rtcore.h "instance visibility"): setVisible stages a flag for the instance
     * of scene object `objectIndex` until commit(), which hides or shows it with the instance indices
     * kept; isVisible is the flag as of the last commit; lastVisibilityStats() says what the last
     * commit changed, whether it rebuilt the flattened instance tree on its own and whether the tree
     * in use holds every visible pair. */
    void setVisible(int32_t objectIndex, bool visible) {
        const int32_t k = instanceOf(objectIndex);
        if (k < 0) throw RenderError(RT_ERR_INVALID_ARG, "the object produced no instance");
        check(rt_scene_set_instance_visible(scene_, k, visible ? 1 : 0));
    }
    bool isVisible(int32_t objectIndex) const {
        const int32_t k = instanceOf(objectIndex);
        if (k < 0) throw RenderError(RT_ERR_INVALID_ARG, "the object produced no instance");
        int32_t v = 0;
        check(rt_scene_instance_visible(scene_, k, &v));
        return v != 0;
    }
    rt_visibility_stats lastVisibilityStats() const {
        rt_visibility_stats st{};
        check(rt_scene_last_visibility_stats(scene_, &st));
        return st;
    }
    /* Ray masks (rtcore.h "ray masks"): setMask gives the instance of scene object `objectIndex` 32
     * mask bits, applied at once with no commit, on static scenes too; maskOf reads them back.  A ray
     * of a masked query (queryClosest / queryOccluded with `masks`, firstHitsMasked) sees an instance
     * iff the two masks share a bit and the instance is visible. */
    void setMask(int32_t objectIndex, uint32_t mask) {
        const int32_t k = instanceOf(objectIndex);
        if (k < 0) throw RenderError(RT_ERR_INVALID_ARG, "the object produced no instance");
        check(rt_scene_set_instance_masks(scene_, k, 1, &mask));
    }
    uint32_t maskOf(int32_t objectIndex) const {
        const int32_t k = instanceOf(objectIndex);
        if (k < 0) throw RenderError(RT_ERR_INVALID_ARG, "the object produced no instance");
        uint32_t m = 0;
        check(rt_scene_instance_mask(scene_, k, &m));
        return m;
    }
    /* Deforming meshes (an engine built with `deformable`, which implies `dynamic`): BVHBuilder.refit
     * (BVH.swift:254-291) applied to a BLAS on the device.  setPositions stages xyz triples (and, for a
     * mesh created with per-vertex normals, optionally new normals) for mesh object `objectIndex`
     * until commit(); with RT_POSITIONS_DEVICE in `flags` the pointers are device pointers used in
     * place, which must stay unchanged until commit() returns.  The caller keeps its own copy of the
     * scene description up to date. */
    int64_t vertexCount(int32_t objectIndex) const {
        int64_t n = 0;
        check(rt_scene_mesh_vertex_count(scene_, objectIndex, &n));
        return n;
    }
    void setPositions(int32_t objectIndex, const double* positions, int64_t numPositions,
                      const double* normals = nullptr, uint32_t flags = 0u) {
        check(rt_scene_set_mesh_positions(scene_, objectIndex, positions, numPositions, normals, flags));
    }
    rt_deform_stats lastDeformStats() const {
        rt_deform_stats st{};
        check(rt_scene_last_deform_stats(scene_, &st));
        return st;
    }
    /* Ray queries (rtcore.h "ray queries"): the scene's production walks on caller-given rays, host
     * arrays (xyz triples; tlimit / time empty = none).  queryClosest fills the fields `want` names;
     * `declared` null lets the device find the batch's bounds. */
    struct RayHits {
        std::vector<double> t, uv, point, normal;
        std::vector<int32_t> ids;                           /* object, face, instance, material */
        std::vector<uint8_t> flags;                         /* RT_HIT_* */
    };
    enum : uint32_t { WantT = 1, WantUV = 2, WantIds = 4, WantPoint = 8, WantNormal = 16, WantFlags = 32 };
    RayHits queryClosest(const std::vector<double>& origins, const std::vector<double>& dirs,
                         const std::vector<double>& tmin = {}, const std::vector<double>& time = {},
                         uint32_t want = WantT | WantUV | WantIds, const rt_query_bounds* declared = nullptr,
                         uint32_t flags = 0u, int32_t slot = 0) {
        return queryClosestWith(nullptr, origins, dirs, tmin, time, want, declared, flags, slot);
    }
    /* ... with ray masks: one mask for every ray, or one per ray (rt_query_closest_masked). */
    RayHits queryClosest(uint32_t mask, const std::vector<double>& origins, const std::vector<double>& dirs,
                         const std::vector<double>& tmin = {}, const std::vector<double>& time = {},
                         uint32_t want = WantT | WantUV | WantIds, const rt_query_bounds* declared = nullptr,
                         uint32_t flags = 0u, int32_t slot = 0) {
        const rt_ray_masks m{nullptr, mask, 0u};
        return queryClosestWith(&m, origins, dirs, tmin, time, want, declared, flags, slot);
    }
    RayHits queryClosest(const std::vector<uint32_t>& masks, const std::vector<double>& origins,
                         const std::vector<double>& dirs, const std::vector<double>& tmin = {},
                         const std::vector<double>& time = {}, uint32_t want = WantT | WantUV | WantIds,
                         const rt_query_bounds* declared = nullptr, uint32_t flags = 0u, int32_t slot = 0) {
        if (masks.size() != origins.size() / 3) throw RenderError(RT_ERR_INVALID_ARG, "one mask per ray");
        const rt_ray_masks m{masks.data(), 0u, 0u};
        return queryClosestWith(&m, origins, dirs, tmin, time, want, declared, flags, slot);
    }
    /* Per ray 0 = free, 1 = blocked, 2 = not traced (beyond `declared`, or non-finite). */
    std::vector<uint8_t> queryOccluded(const std::vector<double>& origins, const std::vector<double>& dirs,
                                       const std::vector<double>& tmax = {}, const std::vector<double>& time = {},
                                       const rt_query_bounds* declared = nullptr, uint32_t flags = 0u,
                                       int32_t slot = 0) {
        return queryOccludedWith(nullptr, origins, dirs, tmax, time, declared, flags, slot);
    }
    std::vector<uint8_t> queryOccluded(uint32_t mask, const std::vector<double>& origins,
                                       const std::vector<double>& dirs, const std::vector<double>& tmax = {},
                                       const std::vector<double>& time = {}, const rt_query_bounds* declared = nullptr,
                                       uint32_t flags = 0u, int32_t slot = 0) {
        const rt_ray_masks m{nullptr, mask, 0u};
        return queryOccludedWith(&m, origins, dirs, tmax, time, declared, flags, slot);
    }
    std::vector<uint8_t> queryOccluded(const std::vector<uint32_t>& masks, const std::vector<double>& origins,
                                       const std::vector<double>& dirs, const std::vector<double>& tmax = {},
                                       const std::vector<double>& time = {}, const rt_query_bounds* declared = nullptr,
                                       uint32_t flags = 0u, int32_t slot = 0) {
        if (masks.size() != origins.size() / 3) throw RenderError(RT_ERR_INVALID_ARG, "one mask per ray");
        const rt_ray_masks m{masks.data(), 0u, 0u};
        return queryOccludedWith(&m, origins, dirs, tmax, time, declared, flags, slot);
    }
    rt_query_counts lastQueryStats(int32_t slot = 0) const {
        rt_query_counts st{};
        check(rt_query_stats(scene_, slot, &st));
        return st;
    }
    /* First-hit buffers (rtcore.h "first-hit buffers"): per pixel of the selected chunks the first
     * primary ray the render casts through it (WantRays: origins, dirs xyz triples, tmin, time) and
     * the record queryClosest returns for that ray (`want` as for queryClosest), rows packed in chunk
     * order, `rows` x `width` pixels.  `flags`: RT_GBUFFER_PIXEL_CENTRE (host arrays only here). */
    struct FirstHits {
        int32_t rows = 0, width = 0;
        std::vector<double> origins, dirs, tmin, time;
        RayHits hits;
    };
    enum : uint32_t { WantRays = 64 };
    FirstHits firstHits(int32_t cameraIndex = 0, int32_t chunkFirst = 0, int32_t chunkStep = 1,
                        uint32_t want = WantRays | WantT | WantIds, uint32_t flags = 0u, int32_t slot = 0) {
        return firstHitsWith(nullptr, cameraIndex, chunkFirst, chunkStep, want, flags, slot);
    }
    /* ... with one ray mask for the whole call (rt_render_gbuffer_masked): a camera layer, picking. */
    FirstHits firstHitsMasked(uint32_t mask, int32_t cameraIndex = 0, int32_t chunkFirst = 0, int32_t chunkStep = 1,
                              uint32_t want = WantRays | WantT | WantIds, uint32_t flags = 0u, int32_t slot = 0) {
        return firstHitsWith(&mask, cameraIndex, chunkFirst, chunkStep, want, flags, slot);
    }
    /* Instance.worldBounds of an instance (any scene), as of the last commit. */
    void instanceBounds(int32_t instance, double lo[3], double hi[3]) const {
        check(rt_scene_instance_bounds(scene_, instance, lo, hi));
    }

private:
    /* The bodies of queryClosest / queryOccluded / firstHits and of their masked forms (masks / mask NULL: unmasked). */
    RayHits queryClosestWith(const rt_ray_masks* masks, const std::vector<double>& origins,
                             const std::vector<double>& dirs, const std::vector<double>& tmin,
                             const std::vector<double>& time, uint32_t want, const rt_query_bounds* declared,
                             uint32_t flags, int32_t slot) {
        const int64_t n = (int64_t)origins.size() / 3;
        if (dirs.size() != origins.size() || (!tmin.empty() && (int64_t)tmin.size() != n) ||
            (!time.empty() && (int64_t)time.size() != n))
            throw RenderError(RT_ERR_INVALID_ARG, "ray arrays differ in length");
        RayHits h;
        rt_hit_batch hb{};
        if (want & WantT) { h.t.resize((size_t)n); hb.t = h.t.data(); }
        if (want & WantUV) { h.uv.resize(2 * (size_t)n); hb.uv = h.uv.data(); }
        if (want & WantIds) { h.ids.resize(4 * (size_t)n); hb.ids = h.ids.data(); }
        if (want & WantPoint) { h.point.resize(3 * (size_t)n); hb.point = h.point.data(); }
        if (want & WantNormal) { h.normal.resize(3 * (size_t)n); hb.normal = h.normal.data(); }
        if (want & WantFlags) { h.flags.resize((size_t)n); hb.flags = h.flags.data(); }
        const rt_ray_batch rb{origins.data(), dirs.data(), tmin.empty() ? nullptr : tmin.data(),
                              time.empty() ? nullptr : time.data()};
        if (masks) check(rt_query_closest_masked(scene_, slot, n, &rb, &hb, declared, flags & ~RT_QUERY_DEVICE, nullptr, masks));
        else check(rt_query_closest(scene_, slot, n, &rb, &hb, declared, flags & ~RT_QUERY_DEVICE, nullptr));
        return h;
    }
    std::vector<uint8_t> queryOccludedWith(const rt_ray_masks* masks, const std::vector<double>& origins,
                                           const std::vector<double>& dirs, const std::vector<double>& tmax,
                                           const std::vector<double>& time, const rt_query_bounds* declared,
                                           uint32_t flags, int32_t slot) {
        const int64_t n = (int64_t)origins.size() / 3;
        if (dirs.size() != origins.size() || (!tmax.empty() && (int64_t)tmax.size() != n) ||
            (!time.empty() && (int64_t)time.size() != n))
            throw RenderError(RT_ERR_INVALID_ARG, "ray arrays differ in length");
        std::vector<uint8_t> out((size_t)n);
        const rt_ray_batch rb{origins.data(), dirs.data(), tmax.empty() ? nullptr : tmax.data(),
                              time.empty() ? nullptr : time.data()};
        if (masks) check(rt_query_occluded_masked(scene_, slot, n, &rb, out.data(), declared, flags & ~RT_QUERY_DEVICE, nullptr, masks));
        else check(rt_query_occluded(scene_, slot, n, &rb, out.data(), declared, flags & ~RT_QUERY_DEVICE, nullptr));
        return out;
    }
    FirstHits firstHitsWith(const uint32_t* mask, int32_t cameraIndex, int32_t chunkFirst, int32_t chunkStep,
                            uint32_t want, uint32_t flags, int32_t slot) {
        FirstHits f;
        if (cameraIndex >= 0 && cameraIndex < (int32_t)cams_.size()) {
            f.width = std::max<int32_t>(1, cams_[(size_t)cameraIndex].width);
            f.rows = rt_rows_for_chunks(cams_[(size_t)cameraIndex].height, chunkFirst, chunkStep);
        }
        const size_t n = (size_t)f.rows * (size_t)f.width;
        rt_gbuffer g{};
        if (want & WantRays) {
            f.origins.resize(3 * n); f.dirs.resize(3 * n); f.tmin.resize(n); f.time.resize(n);
            g.origin = f.origins.data(); g.dir = f.dirs.data(); g.tmin = f.tmin.data(); g.time = f.time.data();
        }
        RayHits& h = f.hits;
        if (want & WantT) { h.t.resize(n); g.hits.t = h.t.data(); }
        if (want & WantUV) { h.uv.resize(2 * n); g.hits.uv = h.uv.data(); }
        if (want & WantIds) { h.ids.resize(4 * n); g.hits.ids = h.ids.data(); }
        if (want & WantPoint) { h.point.resize(3 * n); g.hits.point = h.point.data(); }
        if (want & WantNormal) { h.normal.resize(3 * n); g.hits.normal = h.normal.data(); }
        if (want & WantFlags) { h.flags.resize(n); g.hits.flags = h.flags.data(); }
        if (mask) check(rt_render_gbuffer_masked(scene_, slot, cameraIndex, chunkFirst, chunkStep, &g,
                                                 flags & RT_GBUFFER_PIXEL_CENTRE, nullptr, *mask));
        else check(rt_render_gbuffer(scene_, slot, cameraIndex, chunkFirst, chunkStep, &g,
                                     flags & RT_GBUFFER_PIXEL_CENTRE, nullptr));
        return f;
    }
    static int32_t fileFormat(SceneFormat f) {
        return f == SceneFormat::Json ? RT_SCENE_FORMAT_JSON : f == SceneFormat::Xml ? RT_SCENE_FORMAT_XML
                                                                                     : RT_SCENE_FORMAT_AUTO;
    }
    static RayTracerEngine fromSceneFile(rt_scene_file* f, std::vector<int32_t> devices) {
        std::unique_ptr<rt_scene_file, void (*)(rt_scene_file*)> own(f, rt_scene_file_destroy);
        const rt_scene_desc* d = rt_scene_file_desc(f);
        std::vector<CameraMeta> meta;
        for (int32_t k = 0; k < d->num_cameras; ++k) {
            const char* n = rt_scene_file_image_name(f, k);
            meta.push_back(CameraMeta{"", n ? n : ""});
        }
        return RayTracerEngine(*d, std::move(devices), std::move(meta));
    }

public:

    CameraSpec cameraSpec(int32_t index) const {
        CameraSpec c;
        c.index = index;
        if (index >= 0 && index < (int32_t)meta_.size()) { c.id = meta_[index].id; c.imageName = meta_[index].imageName; }
        c.width = cams_.at(index).width;
        c.height = cams_.at(index).height;
        return c;
    }

    SceneInfo inspect() const {
        rt_scene_info i{};
        check(rt_scene_info_get(scene_, &i));
        SceneInfo s;
        for (int32_t k = 0; k < (int32_t)cams_.size(); ++k) s.cameras.push_back(cameraSpec(k));
        s.meshes = i.meshes; s.triangles = i.triangles; s.spheres = i.spheres; s.planes = i.planes;
        return s;
    }

    /* render(format:cameraIndex:progress:).  `format` is accepted for signature parity (the
     * reference ignores it too once the scene is loaded).  Throws RenderError. */
    RenderResult render(SceneFormat /*format*/, int32_t cameraIndex, const ProgressFn& progress = {}) {
        if (!scene_) throw RenderError(RT_ERR_NO_SCENE, "No scene loaded. Can't render.");
        if (cameraIndex < 0 || cameraIndex >= (int32_t)cams_.size())
            throw RenderError(RT_ERR_INVALID_CAMERA, "Invalid camera index");
        RenderResult r;
        r.camera = cameraSpec(cameraIndex);
        r.fileName = r.camera.imageName;
        const int64_t W = std::max<int32_t>(1, r.camera.width), H = std::max<int32_t>(1, r.camera.height);
        r.rgb.resize((size_t)(W * H * 3));
        r.rgba8.resize((size_t)(W * H * 4));
        rt_stats st{};
        struct Ctx { const ProgressFn* fn; };
        Ctx ctx{&progress};
        rt_progress_fn cb = nullptr;
        if (progress) {
            cb = [](void* user, int32_t done, int32_t total) -> int {
                const Ctx* c = static_cast<const Ctx*>(user);
                RenderProgress p{double(done) / double(total > 0 ? total : 1),
                                 "Row " + std::to_string(done) + "/" + std::to_string(total)};
                return (*c->fn)(p) ? 1 : 0;
            };
        }
        check(rt_render(scene_, cameraIndex, 0, 1, r.rgb.data(), r.rgba8.data(), &st, cb, &ctx));
        r.stats = toStats(st);
        return r;
    }

    /* The render is `async` in the reference (renderRGBA8Async, RayTracer.swift:137-205): a
     * caller may keep several in flight.  submit() enqueues a render of camera `cameraIndex`
     * into page-locked buffers (PinnedBuffer; W*H*4 bytes RGBA8, and/or W*H*3 doubles) that
     * must stay alive until wait(ticket) returns; at most RT_MAX_IN_FLIGHT renders may be
     * pending (RenderError RT_ERR_BUSY).  Renders in flight overlap on the GPUs.
     * kernelTime: time the kernels with HIP events (RenderStats::kernel_ms, else 0). */
    int64_t submit(int32_t cameraIndex, uint8_t* pinnedRgba8, double* pinnedRgb = nullptr, bool kernelTime = false) {
        if (!scene_) throw RenderError(RT_ERR_NO_SCENE, "No scene loaded. Can't render.");
        if (cameraIndex < 0 || cameraIndex >= (int32_t)cams_.size())
            throw RenderError(RT_ERR_INVALID_CAMERA, "Invalid camera index");
        int64_t t = -1;
        check(rt_render_submit(scene_, cameraIndex, 0, 1, pinnedRgb, pinnedRgba8,
                               kernelTime ? RT_RENDER_KERNEL_TIME : 0u, &t));
        return t;
    }
    RenderStats wait(int64_t ticket) {
        rt_stats st{};
        check(rt_render_wait(scene_, ticket, &st));
        return toStats(st);
    }

    /* renderAll(progress:): every camera in order, progress as one fraction over all rows. */
    std::vector<RenderResult> renderAll(const ProgressFn& progress = {}) {
        std::vector<RenderResult> out;
        int64_t totalRows = 0, offset = 0;
        for (const auto& c : cams_) totalRows += std::max(1, c.height);
        for (int32_t k = 0; k < (int32_t)cams_.size(); ++k) {
            const int64_t h = std::max(1, cams_[k].height);
            ProgressFn sub;
            if (progress) {
                sub = [&, h](const RenderProgress& p) {
                    return progress(RenderProgress{(double(offset) + p.fraction * double(h)) / double(totalRows),
                                                   "Camera " + std::to_string(k + 1) + "/" + std::to_string(cams_.size())});
                };
            }
            out.push_back(render(SceneFormat::Auto, k, sub));
            offset += h;
        }
        if (progress) progress(RenderProgress{1.0, "Done"});
        return out;
    }

private:
    static RenderStats toStats(const rt_stats& st) {
        RenderStats r;
        r.meshes = st.meshes; r.triangles = st.triangles; r.spheres = st.spheres; r.planes = st.planes;
        r.primary_rays = st.primary_rays; r.shadow_rays = st.shadow_rays; r.secondary_rays = st.secondary_rays;
        r.rays = st.primary_rays + st.shadow_rays;
        r.milliseconds = st.milliseconds; r.kernel_ms = st.kernel_ms;
        r.shadow_rays_traced = st.shadow_rays_traced;
        r.rewalked = st.rewalked;
        return r;
    }
    rt_scene* scene_ = nullptr;
    std::vector<rt_camera> cams_;
    std::vector<CameraMeta> meta_;
};

/* Page-locked output buffer (rt_host_alloc): rt_render writes such buffers directly. */
template <class T>
class PinnedBuffer {
public:
    explicit PinnedBuffer(size_t n) : n_(n) {
        void* p = nullptr;
        check(rt_host_alloc((uint64_t)(n * sizeof(T)), &p));
        p_ = static_cast<T*>(p);
    }
    ~PinnedBuffer() { rt_host_free(p_); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    T* data() { return p_; }
    const T* data() const { return p_; }
    size_t size() const { return n_; }
    T& operator[](size_t i) { return p_[i]; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace myrt

#endif /* MYRT_RT_ENGINE_HPP */
