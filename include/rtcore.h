/*
 * rtcore.h — C ABI of the MI355X-native renderer core (libmyrt.so).
 *
 * This is the drop-in boundary for the reference's per-pixel trace path
 * (erndmrcn/MyRayTracer).  A host (the Swift `RayTracerEngine`, or the Python
 * mirror in myraytracer_amd/engine.py) describes a scene with plain C structs,
 * creates a device-resident scene once, and renders cameras from it.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to Sources/ of the reference):
 *
 *   rt_scene_create   <- RayTracerEngine.init(from:data:)  RayTracer/RayTracer.swift:30-49
 *                        + RTContext.init(scene:)         RayTracer/Models/RTContext.swift:94-418
 *   rt_render         <- RayTracerEngine.render(format:cameraIndex:progress:)
 *                                                          RayTracer/RayTracer.swift:115-131
 *                        -> renderRGBA8Async               RayTracer/RayTracer.swift:137-205
 *                        -> Renderer.render(scene:cameraIndex:progressRow:)
 *                                                          RayTracer/Extensions/Object+Extension.swift:52-379
 *   rt_render_device  <- same path, output left in device memory (bench / multi-GPU)
 *   rt_scene_info     <- RayTracerEngine.inspect / sceneMeshAndTriangleCounts
 *                                                          RayTracer/RayTracer.swift:52-67,208-227
 *   rt_scene_file_*   <- SceneLoader.load (ParsingKit) in RayTracerEngine.init(from:data:)
 *                                                          RayTracer/RayTracer.swift:30-49
 *   rt_ply_load       <- PLYLoader.load(from:)             RayTracer/Helpers/PLYReader.swift:54-210
 *                        (which drives CPly's ply_reader_* C ABI, CPly/include/PLYReaderWrapper.h:26-69)
 *
 * Conventions mirror the reference's only C ABI (CPly/include/PLYReaderWrapper.h:22-69,
 * CPly/wrapper.cpp:17-27): opaque handle + create/destroy pair, caller-allocated
 * outputs, no C++ exception ever crosses the boundary.  Status codes: 0 = OK,
 * negative = error; the reference's NSError codes are reused (-10, -20, -21,
 * RayTracer.swift:121,141-154).  rt_last_error() returns a thread-local message.
 *
 * All arithmetic is IEEE binary64 (the reference's Vec3 = SIMD3<Double>,
 * RTContext.swift:13-16).  Matrices are column-major 4x4 (simd_double4x4 layout:
 * m[c*4 + r] = column c, row r).
 */
#ifndef MYRT_RTCORE_H
#define MYRT_RTCORE_H

#include <stdint.h>

/* ABI version of this header (rt_version() reports it).
 *   1: round-1/2 layout.
 *   2: rt_object gained `num_normals` (sizeof(rt_object), the stride of rt_scene_desc.objects,
 *      changed: callers built against version 1 must be rebuilt).  A non-NULL `normals` now
 *      requires num_normals == num_positions; version-1 callers that left it 0 get
 *      RT_ERR_INVALID_ARG instead of an unchecked read.
 *   3: rt_stats gained `rewalked` and rt_scene_info `scratch_bytes` (both appended: the
 *      structs grew); rt_scene_set_option / rt_scene_get_option replace the MYRT_*
 *      environment switches (the library reads no environment variable on the render path).
 *   4: the test hooks debug_fail_replica / wide_delta_scale moved behind the non-production
 *      rt_scene_set_unsafe_option; rt_scene_set_option refuses them.
 *   5: dynamic scenes (appended, nothing existing changed): rt_scene_create_ex with
 *      RT_SCENE_DYNAMIC, rt_scene_instance_of_object, rt_scene_set_instance_transform,
 *      rt_scene_set_camera, rt_scene_instance_bounds, rt_scene_commit.
 *      Appended later without moving the version, as the rt_debug_wide_* pair was (callers detect
 *      them by symbol): deforming meshes - RT_SCENE_DEFORMABLE, rt_scene_mesh_vertex_count,
 *      rt_scene_set_mesh_positions, rt_scene_last_deform_stats; ray queries - rt_query_closest,
 *      rt_query_occluded, rt_query_stats; the flattened instance tree rebuilt at a commit -
 *      rt_scene_commit_ex with RT_COMMIT_REBUILD_FIT, rt_scene_last_rebuild_stats; first-hit
 *      buffers - rt_render_gbuffer. */
#define RT_ABI_VERSION 5

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define RT_OK                    0
#define RT_ERR_INVALID_CAMERA  (-10)  /* RayTracer.swift:151-154 "Invalid camera index" */
#define RT_ERR_NO_SCENE        (-20)  /* RayTracer.swift:141-144 "No scene loaded"      */
#define RT_ERR_NO_RENDERER     (-21)  /* RayTracer.swift:145-148 "Renderer not initialized" */
#define RT_ERR_INVALID_ARG     (-30)
#define RT_ERR_UNSUPPORTED     (-31)  /* feature outside the implemented hot path      */
#define RT_ERR_PLY             (-40)  /* PLYReader.swift:24-40 PlyError                */
#define RT_ERR_SCENE_FILE      (-41)  /* SceneLoader / PKDecodingError (scene file decode) */
#define RT_ERR_DEVICE          (-50)  /* HIP runtime failure                           */
#define RT_ERR_OOM             (-51)
#define RT_ERR_CANCELLED       (-60)  /* progress callback returned 0                  */
#define RT_ERR_STACK           (-61)  /* BVH deeper than the traversal stack           */
#define RT_ERR_BUSY            (-32)  /* RT_MAX_IN_FLIGHT renders submitted and not waited for */

/* ---- scene description (ParsingKit Scene stand-in) ----------------------- */
typedef struct rt_vec3 { double x, y, z; } rt_vec3;

/* Material.type strings of the reference (Object+Extension.swift:189,207,252) */
#define RT_MAT_DEFAULT     0
#define RT_MAT_MIRROR      1   /* "mirror"     */
#define RT_MAT_DIELECTRIC  2   /* "dielectric" */
#define RT_MAT_CONDUCTOR   3   /* "conductor"  */

typedef struct rt_material {   /* ParsingKit Material, fields read in trace() */
    rt_vec3 ambient, diffuse, specular, mirror, absorption;
    double  phong;              /* Phong exponent, clamped to >= 1 (:131)      */
    double  ior;                /* refraction index; > 0 disables direct light on back faces (:112-115) */
    double  absorption_index;   /* conductor k (:254)                           */
    double  roughness;          /* glossy perturbation (:191-197)               */
    int32_t type;               /* RT_MAT_*                                     */
    int32_t _pad;
} rt_material;

typedef struct rt_point_light { rt_vec3 position, intensity; } rt_point_light;

typedef struct rt_area_light {  /* Object+Extension.swift:145-186 */
    rt_vec3 position, normal, radiance;
    double  size;
} rt_area_light;

#define RT_CAM_LOOKAT     0     /* cam.type == "lookAt" (Object+Extension.swift:394)   */
#define RT_CAM_NEARPLANE  1     /* explicit nearPlane + gaze (:415-426)                */

typedef struct rt_camera {      /* ParsingKit Camera */
    int32_t type;               /* RT_CAM_*                                            */
    int32_t width, height;      /* imageResolution                                     */
    int32_t num_samples;        /* numSamples                                          */
    rt_vec3 position, gaze_point, gaze, up;
    double  fovy;               /* degrees; NaN = absent (Camera.fovy: Double?)        */
    double  near_distance;
    double  near_plane[4];      /* l, r, b, t                                          */
    double  aperture_size, focus_distance;
} rt_camera;

#define RT_OBJ_MESH           0
#define RT_OBJ_TRIANGLE       1
#define RT_OBJ_SPHERE         2
#define RT_OBJ_PLANE          3
#define RT_OBJ_MESH_INSTANCE  4

/* One entry of Scene.objects, in scene order (RTContext.swift:120-378). */
typedef struct rt_object {
    int32_t kind;               /* RT_OBJ_*                                            */
    int32_t material_id;        /* materialIndex(for:) = Int(id) or -1 (RTContext.swift:423-426), 1-based */
    int32_t smooth;             /* Mesh.shadingMode == "smooth" (RTContext.swift:245)  */
    int32_t id;                 /* object id (MeshInstance.baseMeshID refers to it)    */
    int32_t base_mesh_id;       /* RT_OBJ_MESH_INSTANCE only                           */
    int32_t indices_one_based;  /* inline faces.data are 1-based (RTContext.swift:300-301) */
    double  transform[16];      /* composed localToWorld (Scene.composeTransform result), column-major */
    rt_vec3 motion_blur;        /* Mesh.motionBlur / MeshInstance.motionBlur           */
    /* mesh payload: either a PLY path or inline arrays                               */
    const char*    ply_path;
    const double*  positions;   int64_t num_positions;   /* xyz triples               */
    const int32_t* indices;     int64_t num_indices;     /* triangle list             */
    const double*  normals;     /* optional per-vertex normals (PLY branch, RTContext.swift:267-297);
                                 * length in num_normals below                            */
    /* analytic payloads (RT_OBJ_TRIANGLE / SPHERE / PLANE)                           */
    rt_vec3 v[3];               /* triangle vertices                                   */
    rt_vec3 center;             /* sphere / plane center                               */
    rt_vec3 normal;             /* plane normal                                        */
    double  radius;             /* sphere radius                                       */
    int64_t num_normals;        /* xyz triples behind `normals`; must equal num_positions */
} rt_object;

typedef struct rt_scene_desc {
    rt_vec3 background_color;
    rt_vec3 ambient_light;             /* scene.lights.ambient                         */
    double  shadow_ray_epsilon;
    double  intersection_test_epsilon;
    int32_t max_recursion_depth;
    int32_t num_materials;
    const rt_material*    materials;
    int32_t num_point_lights;
    int32_t num_area_lights;
    const rt_point_light* point_lights;
    const rt_area_light*  area_lights;
    int32_t num_objects;
    int32_t num_cameras;
    const rt_object*      objects;
    const rt_camera*      cameras;
} rt_scene_desc;

/* ---- results -------------------------------------------------------------- */
typedef struct rt_stats {       /* RenderStats (Models/RenderStats.swift:8-24) + ray counts */
    int64_t meshes, triangles, spheres, planes;
    int64_t primary_rays;       /* W*H*n^2 actually cast                               */
    int64_t shadow_rays;        /* one per point light per directly-lit hit            */
    int64_t secondary_rays;     /* reflection rays                                     */
    double  milliseconds;       /* wall time of the render call                        */
    double  kernel_ms;          /* device time of the render kernels                   */
    int64_t shadow_rays_traced; /* shadow rays whose any-hit walk actually ran: the walk is
                                 * skipped when !(N.L > 0), where the reference discards the
                                 * occlusion result (Object+Extension.swift:123-141)      */
    int64_t rewalked;           /* closest-hit rays the four-wide walk handed to the reference-
                                 * order walk because two candidates met their final t    */
} rt_stats;

typedef struct rt_scene_info {
    int64_t meshes, triangles, spheres, planes, instances;
    int64_t blas_nodes, tlas_nodes, max_depth;
    double  build_ms;           /* PLY load + flatten + BVH build + layout            */
    double  upload_ms;          /* host -> device copies                               */
    int64_t device_bytes;       /* per-device resident scene bytes                     */
    int64_t scratch_bytes;      /* device scratch held now by replica 0 (render outputs, pass
                                 * scratch of full trace() renders, queues, deep frames) */
} rt_scene_info;

typedef struct rt_scene rt_scene;   /* opaque */

/* progress: rows finished so far; return 0 to cancel (RayTracer.swift:172-181). */
typedef int (*rt_progress_fn)(void* user, int32_t rows_done, int32_t rows_total);

/* ---- lifecycle ------------------------------------------------------------- */
/* Builds the scene on the host (PLY load, flattening, SAH BVH) and uploads a full
 * replica to each listed device (HIP ordinals; n_devices <= 0 means device 0). */
int32_t rt_scene_create(const rt_scene_desc* desc, const int32_t* devices, int32_t n_devices,
                        rt_scene** out);
void    rt_scene_destroy(rt_scene* scene);
int32_t rt_scene_info_get(const rt_scene* scene, rt_scene_info* out);

/* ---- dynamic scenes (ABI 5) ------------------------------------------------------
 * RTContext.refitTLAS() (RayTracer/Models/RTContext.swift:883-927, "for animation frames") and
 * BVHBuilder.refit (RayTracer/Accelearion/BVH.swift:254-291).  A scene created with
 * RT_SCENE_DYNAMIC accepts new localToWorld matrices for its instances between renders;
 * rt_scene_commit then brings every acceleration structure up to date with the reference's refit
 * semantics: the TLAS keeps its topology and its bounds are recomputed bottom-up from the
 * instances' new world bounds.  No PLY is parsed again and no BLAS rebuilt.  The instances a scene
 * is created with can be hidden and shown again at a commit ("instance visibility" below), so a
 * pool created up front spawns and despawns; instances that did not exist at rt_scene_create_ex
 * can not be added.  Vertices move only in a scene created with RT_SCENE_DEFORMABLE as well
 * ("deforming meshes" below).  A dynamic scene always uses the transformed
 * layout (also while every matrix is the identity); scenes created without the flag behave
 * exactly as before.
 *   rt_scene_create_ex               rt_scene_create with flags (rt_scene_create == flags 0).
 *   rt_scene_instance_of_object      the instance scene object `object_index` produced
 *                                    (*instance = -1: none, e.g. an empty mesh).
 *   rt_scene_set_instance_transform  stages a matrix (column-major) until the next commit; renders
 *                                    before the commit see the old pose.  RT_ERR_UNSUPPORTED on a
 *                                    scene without RT_SCENE_DYNAMIC; RT_ERR_INVALID_ARG (and nothing
 *                                    staged) for a non-finite entry or an upper 3x3 determinant that
 *                                    is 0 or non-finite.
 *   rt_scene_set_camera              replaces camera `camera_index` of any scene, at once.
 *   rt_scene_instance_bounds         Instance.worldBounds of any scene's instance (as of the last
 *                                    commit).
 *   rt_scene_commit                  applies the staged transforms on every device replica and
 *                                    blocks until all are updated.  With nothing staged it is legal
 *                                    and changes nothing.  RT_ERR_UNSUPPORTED without
 *                                    RT_SCENE_DYNAMIC; RT_ERR_INVALID_ARG (nothing changed, the
 *                                    staged transforms dropped) when a transform puts an instance
 *                                    beyond 1e30.  Every tree keeps the topology of the pose the
 *                                    scene was created at; rt_scene_commit_ex (below, "rebuilding
 *                                    the flattened instance tree") can build the one tree whose
 *                                    topology is free again for the committed pose.
 * rt_scene_commit and rt_scene_set_camera return RT_ERR_BUSY, and change nothing, while a render
 * submitted with rt_render_submit has not been waited for.  Renders enqueued with rt_render_device
 * on caller streams are the caller's to order: synchronise those streams before a commit or a
 * camera change.  Both calls drop the measured tile orders (option tile_order) they make stale.
 *
 * How a commit ends.  rt_scene_commit / rt_scene_commit_ex end in exactly one of four ways:
 *   1  Done: RT_OK.
 *   2  Refused, or out of memory, before anything changed: RT_ERR_INVALID_ARG, or RT_ERR_OOM for
 *      every host or device allocation (every device allocation the commit needs short of a
 *      rebuild, on every replica, is made before the first kernel that writes scene memory).  Every
 *      replica and the host are exactly what they were; everything staged is dropped;
 *      rt_scene_last_deform_stats, rt_scene_last_rebuild_stats, rt_scene_last_rebuild_detail and
 *      rt_scene_last_visibility_stats keep reporting the last SUCCESSFUL commit.  (RT_ERR_BUSY,
 *      RT_ERR_UNSUPPORTED and unknown flags return before the staging is touched: it is kept.)
 *   3  The pose committed, the flattened instance tree not rebuilt for want of memory: RT_OK with
 *      rt_rebuild_stats.rebuilt = 0 and reason = RT_REBUILD_NO_MEMORY, for every allocation of the
 *      rebuild, the tree-cost scratch included.  The old tree is refit for the new pose; when the
 *      rebuild was forced by showing an instance the tree lacks, fit_complete stays 0 and the walks
 *      stay on the TLAS's marker tree until a later rebuild succeeds.
 *   4  The scene lost: a HIP runtime error (a failed launch, copy or synchronisation), or any
 *      failure once the commit has begun to write.  The commit returns RT_ERR_DEVICE, and from then
 *      on every render, submit, query, commit, rt_scene_fit_cost and debug read-back of that scene
 *      returns RT_ERR_DEVICE with a message that names the failed commit; the scene never returns a
 *      frame again.  No rollback is attempted (the host keeps no old vertex positions).
 *      rt_scene_destroy and the rt_scene_last_* getters still work; other scenes are unaffected. */
#define RT_SCENE_DYNAMIC 1u
int32_t rt_scene_create_ex(const rt_scene_desc* desc, const int32_t* devices, int32_t n_devices,
                           uint32_t flags, rt_scene** out);
int32_t rt_scene_instance_of_object(const rt_scene* scene, int32_t object_index, int32_t* instance);
int32_t rt_scene_set_instance_transform(rt_scene* scene, int32_t instance, const double m[16]);
int32_t rt_scene_set_camera(rt_scene* scene, int32_t camera_index, const rt_camera* camera);
int32_t rt_scene_instance_bounds(const rt_scene* scene, int32_t instance, double lo[3], double hi[3]);
typedef struct rt_commit_stats {
    int64_t instances_moved;
    double  bounds_ms;          /* instance world bounds (device reduction + host)     */
    double  refit_ms;           /* host TLAS refit + uploads + device tree refit        */
    double  total_ms;
} rt_commit_stats;
int32_t rt_scene_commit(rt_scene* scene, rt_commit_stats* stats /* may be NULL */);

/* ---- deforming meshes (appended under ABI 5; detect by symbol) ---------------------------------
 * BVHBuilder.refit(using:) (RayTracer/Accelearion/BVH.swift:254-291, "bottom-up AABB update")
 * applied to a BLAS: a scene created with RT_SCENE_DEFORMABLE (which implies RT_SCENE_DYNAMIC)
 * accepts new vertex positions for its meshes (skinning, cloth, morph targets) between renders.
 * rt_scene_commit then rewrites the mesh's triangles, normals and boxes on the device and refits
 * its BLAS with the topology kept (myraytracer_amd/csrc/deform.h): no rt_scene_create, no host
 * round trip for positions that already live on the device.  Every instance of the mesh (the base
 * mesh and every MeshInstance of it) follows.  A deformable scene keeps the FP64 layouts
 * (compact_records / compact_tris are not used); scenes without the flag behave exactly as before.
 *   rt_scene_mesh_vertex_count   the vertex count of RT_OBJ_MESH object `object_index` (inline
 *                                num_positions, or the PLY's).
 *   rt_scene_set_mesh_positions  stages xyz triples for that mesh until the next commit; renders
 *       before the commit see the old pose, and staging is legal while renders are in flight.  A
 *       second call for the same mesh replaces the first.  A host array is copied at the call.  With
 *       RT_POSITIONS_DEVICE `positions` (and `normals`) are device pointers used in place: they must
 *       stay valid and unchanged until the commit returns, and every replica of the scene must be on
 *       the device that owns them (else RT_ERR_UNSUPPORTED).  RT_ERR_UNSUPPORTED without
 *       RT_SCENE_DEFORMABLE.  RT_ERR_INVALID_ARG for an object that is not a mesh with at least one
 *       triangle (another kind, an empty mesh, a PLY that failed to load) or a num_positions that is
 *       not the mesh's vertex count.
 *       Normals: a mesh created with per-vertex normals (inline or from its PLY) keeps them when
 *       `normals` is NULL and takes the new ones (same count) otherwise.  A mesh created without
 *       them derives flat or smooth normals from the new positions exactly as the build does;
 *       non-NULL `normals` for such a mesh is RT_ERR_INVALID_ARG.
 *   rt_scene_commit              applies staged positions and staged transforms together.  Before it
 *       changes anything it checks every staged position array on the device - the whole array, so a
 *       NaN in a vertex no triangle references is refused too: every value must be finite, and for
 *       every instance of the mesh reach * (3 * c + 1) < 1e30 must hold (reach: the largest |entry| of
 *       its staged or current matrix; c: the largest |coordinate| plus the largest |motionBlur|
 *       component).  On failure: RT_ERR_INVALID_ARG, everything staged is dropped, nothing changed
 *       ("how a commit ends" above).
 *   rt_scene_last_deform_stats   what the last successful rt_scene_commit did for deformations
 *                                (zeros when it had none staged).  rt_commit_stats keeps its meaning; its total_ms
 *                                includes this work.
 * After a deformation rt_debug_bvh_hash still reports the build's hash. */
#define RT_SCENE_DEFORMABLE 2u      /* rt_scene_create_ex flag; implies RT_SCENE_DYNAMIC */
#define RT_POSITIONS_DEVICE 1u      /* positions / normals are device pointers */
int32_t rt_scene_mesh_vertex_count(const rt_scene* scene, int32_t object_index, int64_t* num_positions);
int32_t rt_scene_set_mesh_positions(rt_scene* scene, int32_t object_index,
                                    const double* positions, int64_t num_positions,
                                    const double* normals /* may be NULL */, uint32_t flags);
typedef struct rt_deform_stats {
    int64_t meshes_deformed, triangles, instances_rebounded;
    double validate_ms;         /* staging copies to the device + the position check    */
    double deform_ms;           /* triangles, triangle boxes, normals, leaf boxes       */
    double blas_refit_ms;       /* BLAS records, four-wide BLAS nodes, root box read-back */
} rt_deform_stats;
int32_t rt_scene_last_deform_stats(const rt_scene* scene, rt_deform_stats* out);   /* of the last successful commit */

/* ---- rebuilding the flattened instance tree (appended under ABI 5; detect by symbol) -----------
 * A commit keeps the topology of every tree, chosen for the pose the scene was created at.  For the
 * reference-form TLAS and the BLASes that topology is the reference's semantics (refitTLAS: it
 * decides tie order and which exact boxes are tested) and stays.  The flattened instance tree that
 * renders and ray queries of transformed scenes walk by default (option fit) is a superset filter
 * only (myraytracer_amd/csrc/wide.h): any topology that holds every (instance, leaf run) pair once
 * gives the reference's hits, frames and ray counts bit for bit.  Its quality falls as instances
 * travel; rt_scene_commit_ex with RT_COMMIT_REBUILD_FIT builds it again on the device for the
 * committed pose (Morton order of the pairs' world boxes, a binary radix tree, collapsed to
 * four-wide nodes: myraytracer_amd/csrc/rebuild.h).  The caller decides when: there is no automatic
 * policy; rt_scene_fit_cost gives the number to decide by.  Measured on C3i:
 * a plain commit takes 0.37 ms, a rebuilding one 4.7 ms with the Morton builder and 4.9 ms with the
 * clustered one (54 to 60 iterations over 562,033 pairs), a new rt_scene_create 510 to 580 ms.  The
 * Morton tree is worth 0.67 to 0.79 of the host's SAH tree there, the clustered one 0.82 to 0.89.  A
 * rebuilt tree of EITHER builder still renders SLOWER than the refit one while the instances have
 * moved by up to four of their own diameters: Morton 0.86 and 0.89 of it at one and four diameters,
 * clustered 0.96 and 0.99.  From eight diameters a rebuild pays: Morton 1.20 times at eight and 2.28
 * times at sixteen, clustered 1.32 and 2.79 times.  rt_rebuild_detail's costs tell the cases apart
 * roughly, not exactly: at one diameter the clustered rebuild raised the cost (18.5 to 20.0), at four
 * it lowered it by 2 % and still rendered 1.5 % slower, at sixteen it lowered it from 31.6 to 7.5.
 * Two builders make the binary tree that is collapsed: RT_COMMIT_REBUILD_FIT takes the radix tree
 * over the Morton codes; RT_COMMIT_REBUILD_FIT_CLUSTERED (alone or together with it) clusters the
 * Morton-sorted pairs instead (parallel locally-ordered clustering: every cluster merges with the
 * neighbour, up to 16 positions away, whose union box with it is smallest, while both agree - DESIGN.md
 * §13).  Both are deterministic: the tree depends on the committed pose only.  A clustering that has
 * not finished after 4 ceil(log2 pairs) + 32 iterations (or the test hook rebuild_cluster_iter_cap)
 * is given up and the Morton tree built instead: no error, rt_rebuild_detail.fell_back = 1.
 *   rt_scene_commit_ex   rt_scene_commit with flags (rt_scene_commit == flags 0).  Staged transforms
 *       and positions are validated and applied exactly as by rt_scene_commit - a refused commit
 *       rebuilds nothing and leaves the last rebuild's stats as they were - then the tree is rebuilt
 *       from the new pose on every replica; with nothing staged a rebuild still rebuilds.  A later
 *       plain commit refits the new topology.  RT_ERR_UNSUPPORTED without RT_SCENE_DYNAMIC,
 *       RT_ERR_BUSY as rt_scene_commit, RT_ERR_INVALID_ARG for unknown flag bits.
 *       Nothing to rebuild is no error: RT_OK with rebuilt = 0 and a reason when the scene has no such
 *       tree (spheres or planes, motion blur, fewer than two pairs), when the tree is blocked by an
 *       instance whose transform exceeds the conditioning bound, when the new tree would be deeper
 *       than the traversal stack allows (or than the test hook rebuild_depth_cap), when its node
 *       array would reach 4 GB, or when an allocation of the rebuild fails (RT_REBUILD_NO_MEMORY: the
 *       tree-cost scratch, the live-pair buffer, the arena, the new nodes and levels, on any replica).
 *       The old tree then stays in place, refit as by a plain commit.
 *   rt_scene_last_rebuild_stats   what the last successful commit did for a rebuild (zeros when it
 *       asked for none).  rt_commit_stats.total_ms includes the rebuild; build_ms includes the clustering.
 *   rt_scene_last_rebuild_detail  which builder made the tree of that commit (zeros when it asked for
 *       no rebuild; builder = 0 and cost_after = cost_before when the old tree stayed), how many
 *       iterations the clustering took, and the tree's cost before and after.
 *   rt_scene_fit_cost    the cost of the tree in use now, on replica 0: the sum, over the non-empty
 *       slots of its nodes, of the slot box's surface area, over the area of the union of the root's
 *       slots (lower is better; what a ray pays grows with it).  Summed in a fixed order: the value
 *       depends on the tree only.  RT_OK with cost 0 when the scene has no such tree;
 *       RT_ERR_UNSUPPORTED without RT_SCENE_DYNAMIC, RT_ERR_BUSY as rt_scene_commit, RT_ERR_OOM when
 *       its scratch cannot be allocated.
 * Not rebuilt: the reference-form TLAS, the BLASes, the TLAS's four-wide marker tree (option fit = 0).
 * A rebuild holds the pairs of the visible instances only ("instance visibility" below); instances
 * that did not exist at rt_scene_create_ex can still not be added. */
#define RT_COMMIT_REBUILD_FIT 1u
#define RT_COMMIT_REBUILD_FIT_CLUSTERED 8u   /* rebuild with the clustered builder (bits 2 and 4 stay unknown) */
#define RT_REBUILD_NONE        0    /* rt_rebuild_stats.reason: rebuilt, or no rebuild asked for */
#define RT_REBUILD_NO_TREE     1
#define RT_REBUILD_BLOCKED     2
#define RT_REBUILD_TOO_DEEP    3
#define RT_REBUILD_TOO_LARGE   4
#define RT_REBUILD_NO_MEMORY   5
typedef struct rt_rebuild_stats {
    int32_t rebuilt;            /* 1: the new tree is in use                               */
    int32_t reason;             /* RT_REBUILD_*: why the old tree stayed                   */
    int64_t pairs;              /* (instance, leaf run) pairs of the tree                  */
    int64_t nodes_before, nodes_after;   /* four-wide nodes per octant copy                */
    int64_t depth_before, depth_after;   /* levels                                         */
    double  sort_ms;            /* pair boxes, Morton codes, radix sort                    */
    double  build_ms;           /* hierarchy, node boxes, collapse, octant copies, swap    */
    double  total_ms;
} rt_rebuild_stats;
int32_t rt_scene_commit_ex(rt_scene* scene, uint32_t flags, rt_commit_stats* stats /* may be NULL */);
int32_t rt_scene_last_rebuild_stats(const rt_scene* scene, rt_rebuild_stats* out);
typedef struct rt_rebuild_detail {
    int32_t builder;            /* 0: none, 1: Morton radix tree, 2: clustered             */
    int32_t iterations;         /* of the clustering                                       */
    int32_t fell_back;          /* 1: the clustering was given up, the Morton tree built   */
    int32_t pad;
    double  cluster_ms;         /* the clustering (part of rt_rebuild_stats.build_ms)      */
    double  cost_before, cost_after;   /* rt_scene_fit_cost around the rebuild             */
} rt_rebuild_detail;
int32_t rt_scene_last_rebuild_detail(const rt_scene* scene, rt_rebuild_detail* out);
int32_t rt_scene_fit_cost(rt_scene* scene, double* cost);

/* ---- instance visibility (appended under ABI 5; detect by symbol) -------------------------------
 * Every instance of a scene created with RT_SCENE_DYNAMIC can be hidden and shown again at a commit;
 * instance indices never change.  After the commit the scene behaves as the reference's refitTLAS()
 * would on a context that holds only the visible instances, with the TLAS topology kept: a hidden
 * instance is there for no ray (renders, shadow rays, bounces, queries) and counts towards no bound
 * or constant (TLAS boxes, the scene's extent and centre, the pruning and widening constants, the
 * conditioning check of the flattened instance tree).  With every instance hidden a frame is the
 * one of a scene without objects and every query ray misses.  A hidden instance still takes staged
 * transforms and deformations of its mesh: shown later it has the pose it would have had, and
 * rt_scene_instance_bounds keeps reporting the box it has or would have.  What is NOT possible:
 * instances (or meshes) that did not exist at rt_scene_create_ex, and masks in renders.  Per-ray masks
 * for ray queries and first-hit buffers need no commit: "ray masks" at the end of this header.
 *   rt_scene_set_instance_visible   stages a flag (non-zero: visible) until the next commit, like
 *       rt_scene_set_instance_transform: legal while renders are in flight, a second call for the
 *       same instance replaces the first.  RT_ERR_UNSUPPORTED without RT_SCENE_DYNAMIC,
 *       RT_ERR_INVALID_ARG (nothing staged) for a bad index.
 *   rt_scene_set_instances_visible  the same for instances [first, first + count), one byte each;
 *       RT_ERR_INVALID_ARG (nothing staged) for a range that is not inside the scene's instances.
 *   rt_scene_instance_visible       the flag as of the last commit.
 *   rt_scene_commit / _ex           apply staged visibility together with transforms and positions;
 *       a commit with only visibility staged is a real commit.  A refused commit drops staged
 *       visibility too and changes nothing.
 * The flattened instance tree: a plain commit gives the slots of hidden pairs boxes no ray enters;
 * a rebuilding commit builds the tree over the visible pairs only.  A commit that shows an instance
 * the tree in use does not hold rebuilds the tree on its own (Morton builder unless the clustered
 * flag is given; forced_rebuild = 1, rt_scene_last_rebuild_stats filled as for a requested rebuild).
 * If that rebuild's guards trip the tree is incomplete (fit_complete = 0) and renders and queries
 * walk the TLAS's marker tree, which always holds every instance, until a later rebuild succeeds. */
int32_t rt_scene_set_instance_visible(rt_scene* scene, int32_t instance, int32_t visible);
int32_t rt_scene_set_instances_visible(rt_scene* scene, int32_t first, int32_t count, const uint8_t* visible);
int32_t rt_scene_instance_visible(const rt_scene* scene, int32_t instance, int32_t* visible);
typedef struct rt_visibility_stats {
    int64_t instances, visible;              /* after the commit                                    */
    int64_t shown, hidden;                   /* changed by it                                       */
    int64_t pairs, pairs_visible, pairs_in_tree;   /* (instance, leaf run) pairs: all, of visible
                                                instances, held by the tree in use               */
    int32_t forced_rebuild;                  /* 1: the commit rebuilt the tree on its own           */
    int32_t fit_complete;                    /* 1: the tree in use holds every visible pair         */
} rt_visibility_stats;
int32_t rt_scene_last_visibility_stats(const rt_scene* scene, rt_visibility_stats* out);   /* of the last successful commit */

/* Render options: tuning and test switches, each default being the production setting.
 *   wide (1)             conservative FP32 four-wide walk of identity scenes (exact: wide.h)
 *   unified (1)          one-stack TLAS+BLAS walks; 0 = the nested walk of intersectTLAS
 *   unified_transformed (1)  one-stack walk of instanced scenes (device.h ut_walk)
 *   compact_records (1), compact_tris (1)   float32 records / triangles when exact
 *   xcd_group (0 = auto) tiles per XCD run      queue (1)  compacted bounce render (0 = megakernel)
 *   queue_levels (-1)    timing probe           hitlog (-1 = auto) logged hits per pixel
 *   nodeshade (1), levels (1), tree_ppw (4),
 *   node_lists (1)                              full trace() pass structure
 *   full_flights (4)     full trace() renders overlapping on slot streams
 *   deep_cap_mb (8192)   deep trace() frames per launch batch
 *   batches (0 = auto), zerocopy (1)            rt_render delivery
 *   submit_events (1), submit_counters (1), submit_dma (0)   rt_render_submit delivery
 *   tile_order (0)       % of tile groups dispatched slowest first
 *   fit (1)              transformed scenes: the flattened instance tree (wide.h fit_walk);
 *                        0 = the TLAS / per-BLAS four-wide walk (tw_walk)
 *   queue_tail (2)       compacted bounce render: levels >= this one traced depth-first in one
 *                        launch (render.hip k_bounce_tail); 0 = one launch per level
 *   query_batch (4194304)  ray queries: rays per launch and per host staging pass (64 .. 2^30)
 *   gbuffer_tiles (1)    rt_render_gbuffer on device arrays: 1 = the render's 8x8 tiles per wave,
 *                        0 = 64 consecutive pixels of a row per wave (the results are the same)
 * Unknown names and out-of-range values return RT_ERR_INVALID_ARG.  Set options between
 * renders (not while renders of the scene are in flight).  The test hooks below are refused
 * here (RT_ERR_INVALID_ARG); rt_scene_get_option reads every option. */
int32_t rt_scene_set_option(rt_scene* scene, const char* name, int64_t value);
int32_t rt_scene_get_option(const rt_scene* scene, const char* name, int64_t* value);

/* NOT FOR PRODUCTION (ABI 4).  Sets any option, including the test hooks that
 * rt_scene_set_option refuses because they void the library's guarantees:
 *   debug_fail_replica (-1)   inject a launch failure on that replica
 *   wide_delta_scale (1000)   the four-wide walk's widening in 1/1000 of the proven bound
 *                             (wide.h); below 1000 exactness is no longer guaranteed
 *   rebuild_depth_cap (42)    levels a rebuilt flattened instance tree may have (1 .. 42, the cap
 *                             that follows from the traversal stack; it can only be lowered): lets a
 *                             small scene exercise the depth guard of RT_COMMIT_REBUILD_FIT
 *   rebuild_cluster_iter_cap (152)  iterations the clustered builder may take: the smaller of this
 *                             and 4 ceil(log2 pairs) + 32 holds (152 is that cap at 2^30 pairs; it can
 *                             only be lowered): lets a small scene exercise the fall-back to Morton
 *   debug_fail_commit_alloc (0)  n > 0: the n-th device allocation the next commit attempts reports
 *                             failure and nothing is allocated for it; counted from 1 over every
 *                             replica and every allocation the commit has to make (scratch it already
 *                             holds is not allocated again)
 *   debug_fail_commit_step (0)   k > 0: the next commit returns as for a HIP runtime error before its
 *                             step k runs (1 position check, 2 moved bounds, 3 range check, 4 triangles,
 *                             5 BLAS refit, 6 bounds of the deformed, 7 visibility, 8 host refit,
 *                             9 upload and tree refit, 10 the rebuild): the scene is lost
 *                             Both are host-side early returns that launch nothing, are read by the
 *                             commit alone and clear themselves when it returns.
 * Used only by the parity tests that show the exactness proof has teeth. */
int32_t rt_scene_set_unsafe_option(rt_scene* scene, const char* name, int64_t value);

/* ---- rendering -------------------------------------------------------------- */
/* Renders 8-row chunks chunk_first, chunk_first+chunk_step, ... of camera
 * `camera_index` (chunk c covers rows [8c, min(8c+8, H)) as in
 * Object+Extension.swift:75-82; row 0 = top).  Outputs are caller-owned HOST
 * buffers holding the selected chunks' rows packed in chunk order:
 * out_rgb = rows*W*3 doubles (the [Vec3] of Renderer.render), out_rgba8 =
 * rows*W*4 bytes (RayTracer.swift:186-195).  Either may be NULL.  chunk_step = 1,
 * chunk_first = 0 renders the whole image.  Work is spread over all devices of
 * the scene. */
int32_t rt_render(rt_scene* scene, int32_t camera_index, int32_t chunk_first, int32_t chunk_step,
                  double* out_rgb, uint8_t* out_rgba8, rt_stats* stats,
                  rt_progress_fn progress, void* user);

/* rt_render with flags.  RT_RENDER_FRAME_LAYOUT: out_rgb / out_rgba8 are whole W x H
 * frames (W*H*3 doubles / W*H*4 bytes) and the selected chunks' rows are written at
 * their image rows; other rows are left untouched.  Several renders of disjoint chunk
 * selections (other devices, other processes sharing one registered buffer) thereby
 * gather one image with no copy.  rt_render(...) == rt_render_ex(..., 0, ...). */
#define RT_RENDER_FRAME_LAYOUT  1u
/* rt_render_submit: time the render kernels with HIP events (rt_stats.kernel_ms of
 * rt_render_wait; 0 without the flag).  rt_render / rt_render_ex always time them. */
#define RT_RENDER_KERNEL_TIME   2u
int32_t rt_render_ex(rt_scene* scene, int32_t camera_index, int32_t chunk_first, int32_t chunk_step,
                     double* out_rgb, uint8_t* out_rgba8, uint32_t flags, rt_stats* stats,
                     rt_progress_fn progress, void* user);

/* Asynchronous render: RayTracerEngine.render is `async` (RayTracer.swift:115-131, 137-205),
 * so a Swift caller may keep several renders in flight (renderAll, BatchRender).
 * rt_render_submit enqueues the render rt_render_ex(..., flags, ...) would do into PAGE-LOCKED
 * outputs (rt_host_alloc / rt_host_register; RT_ERR_INVALID_ARG otherwise), returns at once
 * with *ticket, and the kernels store the image straight into the buffers.  At most
 * RT_MAX_IN_FLIGHT renders per scene may be submitted and not yet waited for (RT_ERR_BUSY).
 * Renders in flight overlap on the GPUs: the next frame's tiles fill the compute units the
 * previous frame's slowest tiles leave idle.  rt_render_wait blocks until that render's
 * image is complete in the buffers and fills stats (milliseconds from submit to completion).
 * Scenes with dielectrics, area lights or maxRecursionDepth > 16 are rendered in submission
 * order.  rt_render_ex with page-locked outputs and no progress callback is submit + wait. */
#define RT_MAX_IN_FLIGHT 16
int32_t rt_render_submit(rt_scene* scene, int32_t camera_index, int32_t chunk_first, int32_t chunk_step,
                         double* out_rgb, uint8_t* out_rgba8, uint32_t flags, int64_t* ticket);
int32_t rt_render_wait(rt_scene* scene, int64_t ticket, rt_stats* stats);

/* Page-locked host buffers for rt_render outputs (hipHostMalloc, mapped + portable).
 * When out_rgb / out_rgba8 lie inside one such allocation (or a range registered with
 * rt_host_register), the render kernels of every device replica store their rows
 * straight into them over PCIe; other host memory goes through pinned staging and a
 * host memcpy.  rt_host_register pins existing host memory (e.g. a shared-memory
 * framebuffer mapped by several processes); unregister before unmapping it. */
int32_t rt_host_alloc(uint64_t bytes, void** out);
void    rt_host_free(void* ptr);
int32_t rt_host_register(void* ptr, uint64_t bytes);
int32_t rt_host_unregister(void* ptr);

/* Same as rt_render on ONE device slot, but outputs are DEVICE pointers on that
 * device and the work is enqueued on `stream` (a hipStream_t, NULL = default)
 * without host synchronisation.  Ray counters are only valid after rt_stats_collect()
 * once the stream has drained.  Device renders have their own counters, pass scratch and
 * queues, so they may overlap rt_render / rt_render_submit renders of the same scene;
 * exception: scenes with maxRecursionDepth > 16 share one deep-frame buffer per replica,
 * and a device render of such a scene must not overlap another render of it.
 * Device renders of ONE slot share those counters and scratch among themselves: issue them
 * on one stream (or order them externally); two concurrent device renders of a slot on
 * different streams race.  Scratch that grows is never freed under a render still queued
 * (the old buffer is retired until rt_scene_destroy), and the call itself reads the scene's
 * options under the scene's lock. */
int32_t rt_render_device(rt_scene* scene, int32_t device_slot, int32_t camera_index,
                         int32_t chunk_first, int32_t chunk_step,
                         double* d_out_rgb, uint8_t* d_out_rgba8, void* stream);
int32_t rt_stats_collect(rt_scene* scene, int32_t device_slot, rt_stats* stats);

/* Number of output rows rt_render writes for a chunk selection. */
int32_t rt_rows_for_chunks(int32_t height, int32_t chunk_first, int32_t chunk_step);

/* Traversal work counters of the last rt_render_device on a slot (instrumented
 * kernel variant; used to price algorithmic bytes for the roofline). */
typedef struct rt_work_counters {
    int64_t records_fetched;    /* 128-B two-child node records loaded                */
    int64_t tri_tests;          /* 80-B triangle records tested                       */
    int64_t normal_fetches;     /* 72-B smooth-normal triples loaded (final hits)     */
    int64_t instance_entries;   /* world->local transforms                            */
    int64_t pixels;             /* pixels written                                     */
    /* The same frame walked in the REFERENCE's order (no t-pruning; any-hit visits L
     * before R and stops at the first occluder; RTContext.swift:544-829), tallied as
     * SURVEY.md §8(d) defines algorithmic work: B = 56*N_nodeFetch + 72*N_triTest +
     * 72*N_smoothHit + 24*N_pixelWrite.  Equal to the oracle's counts (tests/test_gpu_parity.py). */
    int64_t ref_node_fetches;   /* node bounds loaded (roots + both children of each popped inner node; every any-hit pop) */
    int64_t ref_tri_tests;      /* Moeller-Trumbore tests                             */
    int64_t ref_smooth_hits;    /* closer smooth hits (normal triple interpolated)    */
    int64_t ref_pixels;         /* pixels written                                     */
    /* SIMD efficiency of the traversal loops (megakernel, identity scenes): iterations run
     * by lanes vs iterations run by their waves (64 x the max over the wave's lanes).     */
    int64_t lane_steps_closest, wave_steps_closest;
    int64_t lane_steps_shadow, wave_steps_shadow;
    /* Vector-memory redundancy of the inner steps that take per-lane loads (the wave's lanes
     * at more than one record): active lanes vs distinct records among them.             */
    int64_t divergent_lane_loads, divergent_distinct_records;
    /* Per-iteration divergence of the unified walks ([0] closest hit, [1] any hit): wave
     * iterations in which some lane took an inner step / a leaf run / the wave-uniform
     * scalar-cache inner step, and lane iterations that took an inner step / a leaf run.  */
    int64_t iter_wave_inner[2], iter_wave_leaf[2], iter_wave_scalar[2];
    int64_t iter_lane_inner[2], iter_lane_leaf[2];
} rt_work_counters;
int32_t rt_render_device_counted(rt_scene* scene, int32_t device_slot, int32_t camera_index,
                                 int32_t chunk_first, int32_t chunk_step,
                                 double* d_out_rgb, void* stream, rt_work_counters* out);

const char* rt_last_error(void);
const char* rt_version(void);

/* ---- PLY (host) --------------------------------------------------------------- */
typedef struct rt_ply_mesh {            /* PlyMesh (PLYReader.swift:14-19)           */
    double*  positions;  int64_t num_positions;   /* float32 widened to double (:96-102) */
    double*  normals;    int64_t num_normals;     /* normalized (:105-123), 0 if absent  */
    float*   texcoords;  int64_t num_texcoords;
    int32_t* indices;    int64_t num_indices;     /* triangulated, 0-based (:149-198)    */
} rt_ply_mesh;
int32_t rt_ply_load(const char* path, rt_ply_mesh* out);
void    rt_ply_free(rt_ply_mesh* mesh);

/* ---- scene files (host) --------------------------------------------------------
 * RayTracerEngine.init(from: url) / init(data:)  RayTracer/RayTracer.swift:30-49, which read
 * the scene through ParsingKit's SceneLoader.load(.url / .data(format:)) (SceneFormat
 * Models/SceneFormat.swift:8-10).  The decoded scene owns every array rt_scene_file_desc()
 * points into; pass that descriptor to rt_scene_create, then destroy the file.  JSON and XML
 * follow ParsingKit's flexible conventions (myraytracer_amd/csrc/sceneio.cpp); a mesh's PLY
 * path resolves against the scene file's directory (base_dir for in-memory data; NULL = the
 * current directory).  Errors: RT_ERR_SCENE_FILE with rt_scene_file_last_error().           */
#define RT_SCENE_FORMAT_AUTO  0
#define RT_SCENE_FORMAT_JSON  1
#define RT_SCENE_FORMAT_XML   2
typedef struct rt_scene_file rt_scene_file;   /* opaque */
int32_t rt_scene_file_load(const char* path, int32_t format, rt_scene_file** out);
int32_t rt_scene_file_parse(const void* data, uint64_t size, int32_t format, const char* base_dir,
                            rt_scene_file** out);
const rt_scene_desc* rt_scene_file_desc(const rt_scene_file* file);
const char* rt_scene_file_image_name(const rt_scene_file* file, int32_t camera_index);  /* Camera.imageName */
const char* rt_scene_file_last_error(void);
void    rt_scene_file_destroy(rt_scene_file* file);

/* ---- debug / test hooks (not part of the reference surface) -------------------- */
/* Canonical hash of instance `instance`'s BLAS (instance = -1: the TLAS); equal to the
 * oracle's oracle_bvh_hash when the topology, bounds and leaf order match BVH.swift. */
uint64_t rt_debug_bvh_hash(const rt_scene* scene, int32_t instance);
/* Host-only build (no device): hashes[0..n) per instance, hashes[n] = TLAS. */
int32_t  rt_debug_host_build(const rt_scene_desc* desc, uint64_t* hashes, int32_t max_hashes,
                             int32_t* n_instances, rt_scene_info* info);
/* Host-only build of a transformed scene's flattened instance tree (wide.h fit_walk): out[0] =
 * pairs (0: no tree), out[1] = nodes, out[2] = depth, out[3] = leaf runs over all instances,
 * out[4] = a hash of the pairs and the nodes (octant copy 0). */
int32_t  rt_debug_fit_build(const rt_scene_desc* desc, int64_t* out);

/* The four-wide trees themselves (wide.h: the identity tree, or the TLAS / per-BLAS trees and the
 * flattened instance tree of a transformed scene), as plain copies, for the structural tests
 * (tests/wide_tree_check.py).  Like every hook of this section the pair is not part of the
 * versioned surface: it was added without moving RT_ABI_VERSION, as rt_debug_fit_build was.
 *   rt_debug_wide_build   builds on the host like rt_debug_fit_build (no device is touched) with
 *                         rt_scene_create_ex's flags, and copies from the host arrays before they
 *                         are dropped.
 *   rt_debug_wide_read    copies back from device replica `slot` after a device synchronisation
 *                         (hipMemcpy, no kernel); RT_ERR_BUSY while a submitted render has not been
 *                         waited for.
 * Every call fills the counts and scalars.  A buffer pointer that is NULL is skipped; one that is
 * not must hold what its count says, and the caller states what it allocated in the cap_* fields
 * (RT_ERR_INVALID_ARG when a buffer is too small): call once with every pointer NULL, size the
 * buffers, call again.  A scene without a four-wide tree reports wide_root = -1 and zero counts. */
typedef struct rt_wide_dump {
    /* ---- out: counts */
    int64_t wnodes;           /* 128-byte node records over all eight octant copies (8 * wide_copy) */
    int64_t wide_copy;        /* nodes per octant copy                                              */
    int64_t tris;             /* TriRecs (lbox, tri_prim and tri_last have one entry per TriRec)    */
    int64_t pairs;            /* (leaf run, instance) pairs of the flattened instance tree          */
    int64_t instances;        /* instances (tbox, wroot and bcoord are zero for an identity tree)   */
    int64_t tw_tlas_nodes;    /* nodes [0, this) of a copy are the TLAS's (transformed scenes)      */
    int64_t fit_nodes;
    int64_t marker_base;      /* terminal slot ~(marker_base + k) is instance k's marker            */
    int64_t tlas_leaf_base;   /* terminal slots ~t with t below this are leaf runs                  */
    /* ---- out: scalars */
    int32_t wide_root, fit_root;          /* -1: none */
    int32_t identity;                     /* the identity layout (build_wide) */
    int32_t fit_blocked;
    double  wide_coord, fit_coord;
    /* ---- in: capacities of the buffers below, in the units of the counts above */
    int64_t cap_wnodes, cap_tris, cap_pairs, cap_instances;
    /* ---- out: caller-sized buffers (NULL = skipped) */
    void*    nodes;           /* wnodes raw records: float near[3][4], int32 ref[4], float far[3][4], int32 pad[4] */
    double*  lbox;            /* 6 per TriRec: the exact box of the leaf run that starts there      */
    int32_t* fpairs;          /* 2 per pair: first TriRec of the run, instance                      */
    double*  l2w;             /* 16 per instance, column-major                                      */
    double*  tbox;            /* 6 per instance: DWideInst::tbox                                    */
    int32_t* wroot;           /* per instance: DWideInst::wroot (< 0: a BLAS of one leaf run)       */
    double*  bcoord;          /* per instance: DWideInst::bcoord                                    */
    double*  inst_bounds;     /* 6 per instance: Instance.worldBounds                               */
    int32_t* tri_prim;        /* per TriRec: the caller's triangle (index over the scene's meshes and
                               * triangle objects in object order).  An identity scene's TriRec holds
                               * its owning instance instead: rt_debug_wide_build still reports the
                               * triangle, rt_debug_wide_read (the device's copy) the instance     */
    uint8_t* tri_last;        /* per TriRec: 1 = last of its leaf run                               */
} rt_wide_dump;
int32_t rt_debug_wide_build(const rt_scene_desc* desc, uint32_t flags, rt_wide_dump* io);
int32_t rt_debug_wide_read(rt_scene* scene, int32_t slot, rt_wide_dump* io);

/* Explicit-ray queries on device `slot` through the render kernels' traversal (host
 * arrays, n rays; o/d: 3 doubles per ray).  rt_debug_trace_rays = intersectTLAS
 * (RTContext.swift:619-720) with tMin: out_t (+inf on a miss), world hit point, world
 * geometric normal (before facing), materialOverride (-1 on a miss).
 * rt_debug_occluded_rays = occludedTLAS (:724-781) with tMax: out[i] = 1 if blocked.
 * Both are host-array ray queries (below) with declared == NULL on the replica's own stream:
 * rt_query_closest asking for t, point, normal and ids, of which the material column is returned,
 * and rt_query_occluded with its byte mapped to out[i] = (byte == 1).  So a ray with a non-finite
 * origin or direction component is not walked and comes back as a miss (t = +inf, zero point and
 * normal, material -1; occlusion 0); a call counts as the slot's last query for rt_query_stats;
 * the first rt_debug_trace_rays on a slot uploads the face table, as any query asking for ids
 * (rt_scene_info.device_bytes grows once); and a scene without a camera is refused
 * (RT_ERR_UNSUPPORTED), as by the queries.  n == 0 returns RT_OK and touches nothing.       */
int32_t rt_debug_trace_rays(rt_scene* scene, int32_t slot, int32_t n, const double* o, const double* d,
                            const double* tmin, const double* time, double* out_t, double* out_p,
                            double* out_n, int32_t* out_mat);
int32_t rt_debug_occluded_rays(rt_scene* scene, int32_t slot, int32_t n, const double* o, const double* d,
                               const double* tmax, const double* time, uint8_t* out);
/* Reciprocals on device 0 (host arrays, n values): out_fast[i] = the traversal's 1/x
 * (device.h rcp_rn, used when RenderParams::fast_rcp holds), out_div[i] = IEEE 1.0/x.
 * Equal bit for bit for 2^-700 <= |x| <= 2^1000 (tests/test_gpu_rays.py).  No scene. */
int32_t rt_debug_rcp(int32_t n, const double* x, double* out_fast, double* out_div);
/* Per-wave timeline of one megakernel launch (identity scenes without dielectrics or area
 * lights) into device buffer d_out_rgb: out[3*k..3*k+2] = {start, end, tile} of wave k in
 * 100 MHz ticks (s_memrealtime); the tile word also holds the wave's largest lane iteration
 * counts of the closest-hit walks (bits 24-43) and the any-hit walks (bits 44-63).  *n_waves = waves launched; at most max_waves are copied.
 * Returns RT_ERR_UNSUPPORTED unless the library was built with -DMYRT_WAVE_TIMES=1. */
int32_t rt_debug_wave_times(rt_scene* scene, int32_t slot, int32_t camera_index, int32_t chunk_first,
                            int32_t chunk_step, double* d_out_rgb, uint64_t* out, int64_t max_waves,
                            int64_t* n_waves);

/* ---- ray queries ------------------------------------------------
 * The scene's production walks on caller-given rays, from host or device arrays, with full hit
 * records.  Added without moving RT_ABI_VERSION: detect the entry points by symbol, as the
 * deformation entry points are.  A ray means what it means to rt_debug_trace_rays /
 * rt_debug_occluded_rays: rt_query_closest = intersectTLAS (RTContext.swift:619-720) with tMin,
 * rt_query_occluded = occludedTLAS (:724-781) with tMax, through the walk the scene's options
 * select (wide, unified, unified_transformed, fit).
 *
 *   ids       4 per ray: [0] the scene object the geometry belongs to (a MeshInstance: the instance
 *             object; rt_scene_instance_of_object gives the other direction; -1 for a mesh whose id
 *             a MeshInstance took over), [1] the triangle's index in its own object's face list as
 *             the scene was given (a PLY: the order rt_ply_load returns; RT_OBJ_TRIANGLE: 0; spheres
 *             and planes: -1), [2] the flattened instance, [3] the instance's material.  All -1 on a
 *             miss.  The first query that asks for ids uploads a face table to the replica (4 bytes
 *             per triangle record plus 4 per instance, rt_scene_info.device_bytes from then on).
 *   flags     RT_QUERY_DEVICE: every pointer of the batches (and `out`) is a device pointer on the
 *             slot's device (else RT_ERR_UNSUPPORTED); the work is enqueued on `stream` (a
 *             hipStream_t, NULL = default).  Without it the arrays are host arrays, staged through
 *             the slot's query scratch, and the call returns with the results in them.
 *   declared  NULL: one reduction kernel finds the batch's largest origin distance to the scene
 *             centre, largest |origin coordinate| and largest |d|, which size the pruning margin and
 *             the four-wide walk's widening through the functions every render uses;
 *             the call synchronises `stream` once to read them.  Not NULL: the caller's bounds are
 *             used instead and a device query only enqueues (no synchronisation, nothing read back).
 *             A ray beyond any declared bound is NOT traced: its record is a miss with
 *             RT_HIT_OUT_OF_BOUNDS (rt_query_occluded: out = 2).  A ray with a non-finite origin or
 *             direction component is never traced either way: RT_HIT_NON_FINITE (out = 2), and it
 *             does not enter the reduction.
 *             Forming safe bounds: origin_coord and dir_norm are the batch's own largest |origin
 *             coordinate| and |d|.  origin_reach is measured from the centre of the scene's world
 *             box, which moves with rt_scene_commit; the centre lies inside the union of the boxes
 *             rt_scene_instance_bounds returns, so the largest distance from an origin to the
 *             farthest corner of that union is always enough.  rt_query_counts.bounds of a query
 *             with declared == NULL reports the exact maxima of that batch at the current pose.
 *             Any bound above the true maximum is safe (larger bounds only widen the margins).
 *
 * Large batches run as several launches (render option query_batch, rays per launch) under one
 * set of constants.  Queries of ONE slot share its scratch and statistics: issue them on one stream
 * (or order them externally).  A query holds the scene's lock only while it is prepared, not while
 * it runs: ordering it against rt_scene_commit is the caller's job, as for rt_render_device.
 * Scratch that grows is retired, not freed, under queries still queued.
 * RT_ERR_INVALID_ARG: a bad slot, n < 0, NULL origin / dir with n > 0, unknown flags, a negative
 * or non-finite member of `declared`; after a refusal nothing has been enqueued. */
typedef struct rt_ray_batch {       /* n rays; arrays of doubles */
    const double *origin, *dir;     /* 3 per ray */
    const double *tlimit;           /* closest: tMin, NULL = 0; occluded: tMax, NULL = +inf */
    const double *time;             /* NULL = 0 */
} rt_ray_batch;
typedef struct rt_hit_batch {       /* every pointer optional (NULL = not written) */
    double  *t;                     /* +inf on a miss */
    double  *uv;                    /* 2 per ray: Moeller-Trumbore u, v (0 for spheres / planes and misses) */
    int32_t *ids;                   /* 4 per ray: object, face within that object, instance, material */
    double  *point, *normal;        /* 3 per ray, as rt_debug_trace_rays returns them */
    uint8_t *flags;                 /* RT_HIT_* bits */
} rt_hit_batch;
typedef struct rt_query_bounds { double origin_reach, origin_coord, dir_norm; } rt_query_bounds;
#define RT_QUERY_DEVICE       1u
#define RT_HIT_VALID          1u    /* the ray hit something */
#define RT_HIT_OUT_OF_BOUNDS  2u    /* beyond a declared bound: not traced */
#define RT_HIT_NON_FINITE     4u    /* non-finite origin or direction: not traced */
/* (the statistics record is rt_query_counts: in C a struct typedef and a function cannot share
 * the name rt_query_stats) */
typedef struct rt_query_counts {
    int64_t rays, hits, out_of_bounds, non_finite;
    int64_t launches;               /* query kernel launches of the call */
    int32_t reduced;                /* 1: the bounds came from the device reduction */
    int32_t walk;                   /* 0 general, 1 unified identity, 2 unified transformed, 3 flattened instance tree */
    rt_query_bounds bounds;         /* the bounds the constants were formed from */
} rt_query_counts;
int32_t rt_query_closest(rt_scene* scene, int32_t device_slot, int64_t n, const rt_ray_batch* rays,
                         const rt_hit_batch* hits, const rt_query_bounds* declared, uint32_t flags, void* stream);
int32_t rt_query_occluded(rt_scene* scene, int32_t device_slot, int64_t n, const rt_ray_batch* rays, uint8_t* out,
                          const rt_query_bounds* declared, uint32_t flags, void* stream);
/* Of the last query on the slot, once its stream has drained (the call waits for nothing). */
int32_t rt_query_stats(rt_scene* scene, int32_t device_slot, rt_query_counts* out);
/* Host-only build (no device, as rt_debug_wide_build): the face table, the per-instance object
 * indices and the triangle records' v0, e1, e2 (9 doubles each).  Call with NULL buffers for the
 * counts; a buffer that is not NULL must hold what the counts say.  tri_object: per triangle
 * record the object whose face list it comes from. */
typedef struct rt_query_tables {
    int64_t tris, instances;                     /* out */
    int32_t *face, *tri_object;                  /* per triangle record */
    double  *verts;                              /* 9 per triangle record */
    int32_t *inst_object;                        /* per instance */
} rt_query_tables;
int32_t rt_debug_query_tables(const rt_scene_desc* desc, uint32_t flags, rt_query_tables* io);

/* ---- first-hit buffers --------------------------------------------
 * Per pixel of the selected chunks: the first primary ray the render casts through that pixel, and
 * the record rt_query_closest returns for that ray (picking, depth / id / normal buffers, a correct
 * ray set for the ray queries).  Added without moving RT_ABI_VERSION: detect the entry point by
 * symbol, as the ray queries are.
 *
 * A pixel's first ray is sample (sx, sy) = (0, 0) of Object+Extension.swift:285-356 exactly as the
 * render forms it: the pixel's PCG32, two draws for the jitter in sub-cell (0, 0) of the
 * n x n = floor(sqrt(numSamples))^2 grid, the lens draw when apertureSize > 0 and focusDistance > 0,
 * one draw for `time`, and tmin = max(distance to the image plane, 0).  For a camera with one sample
 * it is the pixel's only ray.  Samples after the first are NOT available: their draws follow the
 * draws shading consumes.  With RT_GBUFFER_PIXEL_CENTRE the ray is the deterministic one through
 * (i + 0.5, j + 0.5): no lens offset, time = 0, the same tmin formula, nothing drawn.
 * The record is rt_query_closest's of that ray with its tmin and time (rt_hit_batch above), bit for
 * bit: the same walk (the one the scene's options select for the render), the scene as of the last
 * commit.  A ray with a non-finite component (a degenerate camera) is not traced: a miss flagged
 * RT_HIT_NON_FINITE.
 *
 *   layout    chunks are selected and rows packed as by rt_render: chunk c covers rows
 *             [8c, min(8c + 8, H)), packed in chunk order, rt_rows_for_chunks rows of W pixels.  With
 *             RT_GBUFFER_FRAME_LAYOUT every array is a whole W x H array and the selected rows are
 *             written at their image rows (as RT_RENDER_FRAME_LAYOUT); other rows are not touched.
 *   arrays    without RT_GBUFFER_DEVICE host arrays, staged through the slot's query scratch in
 *             passes of at most query_batch pixels; the call returns with the results in them.  With
 *             it every pointer is a device pointer on the slot's device (else RT_ERR_UNSUPPORTED), the
 *             work is enqueued on `stream` (a hipStream_t, NULL = default) and nothing synchronises:
 *             the constants are the render's of that camera, so nothing is reduced or read back.
 *             When no pointer of `hits` is set a small kernel writes the rays alone.  A call with
 *             every pointer NULL returns RT_OK and launches nothing.
 *   ids       asking for them uploads the face table on first use, exactly as a query does.
 *   stats     the call counts as the slot's last query for rt_query_stats: rays = pixels,
 *             reduced = 0, walk, hits, non_finite, and bounds = the camera's (the largest lens
 *             origin's reach and coordinate, |d| <= 1 + 2^-50): they may be declared to a query of the
 *             exported rays.  It shares the slot's query scratch and the queries' ordering rule.
 *
 * Refusals (nothing enqueued, outputs untouched): RT_ERR_NO_SCENE; RT_ERR_DEVICE after a failed
 * commit (the scene was lost); RT_ERR_INVALID_CAMERA; RT_ERR_INVALID_ARG for a bad slot, unknown
 * flag bits, out == NULL, chunk_first < 0 or chunk_step < 1; RT_ERR_UNSUPPORTED for a pointer that
 * is not on the slot's device under RT_GBUFFER_DEVICE.  Render option gbuffer_tiles (1) picks the
 * pixel-to-lane mapping of a device call; the results do not depend on it. */
typedef struct rt_gbuffer {      /* every pointer optional (NULL = not written) */
    double *origin, *dir;        /* 3 per pixel: the first ray; same layout as rt_ray_batch */
    double *tmin, *time;         /* 1 per pixel */
    rt_hit_batch hits;           /* the record of that ray, as rt_query_closest writes it */
} rt_gbuffer;
#define RT_GBUFFER_DEVICE        1u  /* device pointers on the slot's device; enqueue on `stream`, no sync */
#define RT_GBUFFER_PIXEL_CENTRE  2u
#define RT_GBUFFER_FRAME_LAYOUT  4u  /* whole W x H arrays, rows written at their image rows (as RT_RENDER_FRAME_LAYOUT) */
int32_t rt_render_gbuffer(rt_scene* scene, int32_t device_slot, int32_t camera_index,
                          int32_t chunk_first, int32_t chunk_step,
                          const rt_gbuffer* out, uint32_t flags, void* stream);

/* ---- ray masks (appended under ABI 5; detect by symbol) ------------------------------
 * Every instance carries 32 mask bits (0xFFFFFFFF at creation) and a masked query gives every ray 32
 * mask bits: ray r sees instance k iff (instance_mask[k] & ray_mask[r]) != 0 and k is visible as of
 * the last commit.  The walk skips an instance the ray does not see where it would enter it, so the
 * answer is, bit for bit, the unmasked answer for the scene that holds only the instances the ray sees
 * (a hit on a masked-out instance never hides the hit behind it), and the instance's BLAS is never
 * entered.  No commit is involved: masks work on static, dynamic and deformable scenes alike, beside
 * renders in flight.
 *
 *   rt_scene_set_instance_masks  masks of instances [first, first + count), applied at once on every
 *       replica (host side plus one copy per replica).  Masks belong to the scene, not to a commit:
 *       they survive commits of every kind, instance indices never change, and renders never read
 *       them.  Ordering the change against queries already enqueued on the caller's streams is the
 *       caller's job, as for rt_scene_commit.  The per-replica table (4 bytes per instance, counted
 *       in rt_scene_info.device_bytes) is allocated by the first call, on every replica before any is
 *       written; until then a masked query treats every instance mask as all-ones.  Refusals, with
 *       nothing changed: RT_ERR_NO_SCENE; RT_ERR_DEVICE after a failed commit; RT_ERR_INVALID_ARG
 *       for a range that is not inside the scene's instances or masks == NULL with count > 0;
 *       RT_ERR_OOM.
 *   rt_scene_instance_mask       reads one back (0xFFFFFFFF until it was set).
 *   rt_ray_masks                 the rays' masks of one call: per_ray == NULL gives every ray `all`;
 *       otherwise one uint32 per ray - a device pointer on the slot's device under RT_QUERY_DEVICE
 *       (else RT_ERR_UNSUPPORTED), a host array otherwise, staged with the rays in the same passes.
 *   rt_query_closest_masked / rt_query_occluded_masked   rt_query_closest / rt_query_occluded with
 *       masks.  masks == NULL is the unmasked call: it ignores instance masks entirely and runs the
 *       kernels it always ran, as the unmasked entry points do.  A ray with mask 0 misses; it is not
 *       flagged and counts as a traced ray.  Everything else is the unmasked call's: tMin / tMax and
 *       time, declared and reduced bounds with their flags, ids / uv / point / normal, query_batch
 *       launches, rt_query_stats, the walk the scene's options select, equal-t ties re-walked in the
 *       reference's order (under the same mask), the refusals.
 *   rt_render_gbuffer_masked     rt_render_gbuffer with ONE mask for the whole call (camera layers,
 *       picking against selectable objects); the record is rt_query_closest_masked's of the exported
 *       ray with that mask.
 * Out of scope: masks in renders (shadow-caster flags, camera layers for rt_render and its
 * siblings), a tMax for closest-hit queries, ids from occlusion queries. */
typedef struct rt_ray_masks {
    const uint32_t* per_ray;        /* NULL: every ray has `all` */
    uint32_t all;
    uint32_t pad;
} rt_ray_masks;
int32_t rt_scene_set_instance_masks(rt_scene* scene, int32_t first, int32_t count, const uint32_t* masks);
int32_t rt_scene_instance_mask(const rt_scene* scene, int32_t instance, uint32_t* mask);
int32_t rt_query_closest_masked(rt_scene* scene, int32_t device_slot, int64_t n, const rt_ray_batch* rays,
                                const rt_hit_batch* hits, const rt_query_bounds* declared, uint32_t flags,
                                void* stream, const rt_ray_masks* masks);
int32_t rt_query_occluded_masked(rt_scene* scene, int32_t device_slot, int64_t n, const rt_ray_batch* rays,
                                 uint8_t* out, const rt_query_bounds* declared, uint32_t flags, void* stream,
                                 const rt_ray_masks* masks);
int32_t rt_render_gbuffer_masked(rt_scene* scene, int32_t device_slot, int32_t camera_index,
                                 int32_t chunk_first, int32_t chunk_step,
                                 const rt_gbuffer* out, uint32_t flags, void* stream, uint32_t mask);

#ifdef __cplusplus
}
#endif
#endif /* MYRT_RTCORE_H */
