// scene.h — host-side scene construction for the MI355X renderer core.
//
// Restates what RTContext.init(scene:) (RT/Models/RTContext.swift:94-418) and
// BVHBuilder (RT/Accelearion/BVH.swift:67-250) produce, then re-lays the result
// into the device layout of layout.h.  BVH topology, node bounds and leaf
// primitive order are bit-identical to the reference builder (they decide the
// traversal order); node numbering is free.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rtcore.h"
#include "layout.h"

namespace myrt {

// Reference-form BVH (BVH.swift:16-30): node bounds, leftFirst/primitiveCount,
// primitiveIdx permutation.  Nodes are numbered exactly as the Swift builder does.
struct RefBVH {
    std::vector<double> lo, hi;            // 3 per node
    std::vector<int64_t> leftFirst, count; // count > 0 => leaf
    std::vector<int64_t> primIdx;
    int64_t nodesUsed = 0;
    bool isLeaf(int64_t n) const { return count[n] > 0; }
};

// Primitive set handed to the builder (PrimitiveInfo bounds + centroid).
struct PrimSet {
    int64_t n = 0;
    std::vector<double> bmin, bmax, cen;   // 3 per prim, xyz interleaved
};

RefBVH build_ref_bvh(const PrimSet& prims, int maxLeaf = 2, int binCount = 12);
uint64_t ref_bvh_hash(const RefBVH& b, const std::vector<int64_t>& primIndexOf);
int64_t ref_bvh_depth(const RefBVH& b);   // max number of inner nodes on a root-to-leaf path

struct HostCamera { rt_camera c; };

// ---- dynamic scenes (rt_scene_create_ex with RT_SCENE_DYNAMIC; scene.cpp refit_host_scene) -----
// What a commit needs after the large host arrays are gone: per BLAS its TriRec run, kind, the
// bounds of a sphere / plane, the motion vector and the pruning-margin constant; per instance its
// BLAS; the TLAS in reference form (topology and primIdx are kept, bounds are refit bottom-up as
// BVHBuilder.refit does, BVH.swift:254-291); and, for the four-wide TLAS nodes and the flattened
// instance tree, the nodes of every level, deepest level first (the device refits a level per
// launch, refit.h).  fit_levels is replaced when a commit rebuilds the flattened instance tree
// (commit.h rebuild_fit): the next plain commit refits the new topology.
struct DynBlas {
    int64_t tri_first = 0, tri_end = 0;
    int32_t kind = kPrimTriangles;
    double pmin[3] = {0, 0, 0}, pmax[3] = {0, 0, 0};   // spheres / planes: the primitive's bounds
    double motion[3] = {0, 0, 0};
    double P = 0.0;                                    // pruning margin constant (scene.cpp blasP)
};
struct RefitLevels {
    std::vector<int32_t> nodes;            // node indices (octant copy 0), deepest level first
    std::vector<int64_t> off;              // level l is nodes[off[l], off[l + 1])
};
struct DynScene {
    std::vector<DynBlas> blas;
    std::vector<int32_t> inst_blas;
    RefBVH tlas;
    std::vector<WRec> tlas_recs;           // host image of the TLAS records (re-laid by a commit)
    RefitLevels tlas_levels, fit_levels;
    std::vector<double> pbox;              // 6 per TriRec: the triangle's exact local box (when the
                                           // scene has no CTri; dropped after upload)
    bool fit_blocked = false;              // an instance exceeds kFitKappa: tw_walk until a commit passes
    // instance visibility (rtcore.h "instance visibility").  A hidden instance keeps
    // its real DInstance, inst_bounds and bcoord here; refit_host_scene leaves it out of every union
    // and constant, and the device copy of its DInstance carries a NaN root box (commit.h).
    std::vector<uint8_t> visible;          // per instance, as of the last commit (empty: all visible)
    std::vector<uint8_t> in_tree;          // per instance: the flattened instance tree in use holds its pairs
    int64_t n_visible = 0;
    bool fit_incomplete = false;           // a visible instance is not in the tree: tw_walk until a rebuild succeeds
    bool is_visible(size_t i) const { return visible.empty() || visible[i] != 0; }
};

// ---- deformable scenes (rt_scene_create_ex with RT_SCENE_DEFORMABLE; deform.h) ---------------------
// What rt_scene_set_mesh_positions / rt_scene_commit need to bring a BLAS up to date with new
// vertex positions on the device, the topology kept (BVHBuilder.refit, BVH.swift:254-291): per
// TriRec its three mesh-local vertex ids; per BLAS its vertex count, how its normals were made, its
// WRec records and its four-wide nodes by level (deepest first) and, for derived smooth normals,
// the vertex -> incident triangle adjacency (CSR; a vertex's entries in ascending triangle order,
// one per corner, so that a vertex's sum runs in the builder's order, scene.cpp "normals").
constexpr int32_t kNormalsFlat = 0, kNormalsSupplied = 1, kNormalsSmooth = 2;
struct DeformBlas {
    int64_t verts = 0;                     // 0: not a mesh (a triangle object, a sphere, a plane)
    int32_t normals = kNormalsFlat;
    int32_t prim_base = 0;                 // TriRec::prim - prim_base = the mesh's own triangle index
    int32_t root_ref = 0;                  // BLAS root (layout.h ref encoding)
    int32_t wroot = -1;                    // its four-wide root (DWideInst::wroot); < 0: no node
    std::vector<int64_t> rec_off;          // level l: DeformScene::rec_list[rec_off[l], rec_off[l + 1])
    std::vector<int64_t> wide_off;         // ... wide_list
    int64_t csr_off_first = 0;             // kNormalsSmooth: csr_off[csr_off_first + v], verts + 1 entries,
    int64_t csr_first = 0;                 //   counting from csr_tri[csr_first]
};
struct DeformScene {
    std::vector<DeformBlas> blas;
    std::vector<int32_t> vid;              // 3 per TriRec, leaf order (dropped after upload)
    std::vector<int32_t> rec_list, wide_list, csr_off, csr_tri;   // (dropped after upload)
};

struct HostScene {
    // ---- scene-level parameters
    double eps = 0, shadow_eps = 0;
    double background[3] = {0, 0, 0}, ambient[3] = {0, 0, 0};
    int32_t max_depth = 0;
    std::vector<DMaterial> mats;
    std::vector<DPointLight> plights;
    std::vector<DAreaLight> alights;
    std::vector<double> jitter;            // 2 x kJitterCells (buildStratifiedJitter)
    int32_t num_area_lights = 0;
    bool has_special = false;              // sphere / plane objects present
    std::vector<rt_camera> cams;
    bool has_dielectric = false;
    // ---- device layout (host copies)
    std::vector<WRec> recs;
    std::vector<CRec> crecs;               // float32-bound copy of the BLAS records (if exact)
    int64_t compact_records = 0;           // crecs.size() (kept after the host copy is dropped)
    std::vector<TriRec> tris;
    std::vector<CTri> ctris;               // float32-vertex copy of tris (if every vertex is exact)
    bool compact_tris = false;
    std::vector<double> normals;           // 9 per TriRec
    std::vector<DInstance> insts;
    std::vector<DTlasLeafEntry> tlas_leaf;
    double tlas_root_lo[3] = {0, 0, 0}, tlas_root_hi[3] = {0, 0, 0};
    int32_t tlas_root_ref = 0;
    int64_t tlas_leaf_base = 0;            // TLAS leaf refs are ~(tlas_leaf_base + entry)
    bool has_tlas = false;
    bool identity = false;                 // all instances identity & static (unified walk)
    bool dynamic = false;                  // set before build_host_scene: identity stays false, dyn is filled
    DynScene dyn;
    bool deformable = false;               // set before build_host_scene (implies dynamic): FP64 layouts only
    DeformScene def;
    std::vector<int32_t> object_blas;      // per scene object: the BLAS an RT_OBJ_MESH produced, or -1
    std::vector<double> inst_bounds;       // 6 per instance: Instance.worldBounds (lo, hi)
    std::vector<int32_t> object_inst;      // per scene object: the instance it produced, or -1
    // ray queries (query.h): per TriRec, leaf order, the triangle's index in its own object's face
    // list (-1: a sphere / plane), and per instance the object it came from (-1: a mesh whose id a
    // MeshInstance took over).  Kept on the host: a replica takes them on its first ids query.
    std::vector<int32_t> face;
    std::vector<int32_t> inst_obj;
    std::vector<int32_t> tri_obj;          // keep_tri_src only: per TriRec the object that gave the face
    int64_t blas_records = 0, tlas_records = 0;
    int64_t max_stack = 0;                 // traversal stack entries the general walk needs
    int64_t max_stack_unified = 0;         // ... and the unified identity walk
    double scene_extent = 1.0;             // world bounds diagonal (pruning margin scale)
    double scene_center[3] = {0, 0, 0};    // world bounds center
    double prune_k = 0.0;                  // MT t-error constant (scene.cpp, "pruning margin")
    double max_motion = 0.0;               // largest instance + triangle motion-blur offset
    double det_scale = 0.0;                // >= |e1||e2| * ||A||_F over triangle instances: every
                                           // Moeller-Trumbore |det| <= det_scale * |d_world|
    // ---- conservative FP32 four-wide walk (identity scenes, scene.cpp build_wide)
    std::vector<W4Node> wnodes;
    std::vector<double> lbox;              // 6 per TriRec index: exact box of the leaf run starting there
    int64_t wide_leaves = 0;               // reference leaves under the wide tree
    int32_t wide_root = -1;                // -1: no wide tree
    int64_t wide_copy = 0;                 // nodes per octant copy (wnodes holds eight, layout.h W4Node)
    double wide_coord = 0.0;               // largest |coordinate| of any box (wdelta scale; TLAS boxes
                                           // for transformed scenes)
    // transformed scenes (static, triangles only): TLAS nodes first, then every BLAS's nodes
    std::vector<DWideInst> winst;          // per instance (layout.h DWideInst); empty: identity tree
    int64_t tw_tlas_nodes = 0;
    // flattened instance tree (scene.cpp build_fit): world-space nodes over (leaf run, instance)
    // pairs, appended to wnodes; fit_root < 0: none (tw_walk only)
    std::vector<DFitPair> fpairs;
    int32_t fit_root = -1;
    int64_t fit_nodes = 0, fit_depth = 0;
    double fit_coord = 0.0;                // bound on every magnitude the fit widening covers
    double fit_ms = 0.0;                   // host time of build_fit
    // ---- bookkeeping / debug
    int64_t n_meshes = 0, n_tris = 0, n_spheres = 0, n_planes = 0;
    std::vector<uint64_t> inst_bvh_hash;   // per instance: canonical hash of its BLAS
    bool keep_tri_src = false;             // set before build_host_scene by rt_debug_wide_build only
    std::vector<int32_t> tri_src;          // ... then, identity scenes: per TriRec the reference `triangles[]`
                                           // index its prim held before it became the owning instance
    uint64_t tlas_hash = 0;
    double build_ms = 0;
};

// Returns RT_OK or a negative status with `err` set.
int32_t build_host_scene(const rt_scene_desc* desc, HostScene& out, std::string& err);

// Dynamic scenes.  set_instance_matrix: instance k's DInstance fields that depend on localToWorld
// (l2w, w2l, nmat, det_neg).  special_instance_bounds: world bounds of a sphere / plane instance
// (one primitive: AABB.transformed of its box).  refit_host_scene: after inst_bounds and insts are
// current, everything else a render derives from the transforms - the TLAS bounds bottom-up, the
// TLAS records (dyn.tlas_recs), tlas_root_lo/hi, DWideInst::tbox, scene_extent / scene_center,
// prune_k, det_scale, wide_coord, fit_coord and the kFitKappa check (dyn.fit_blocked).
bool matrix_ok(const double m[16]);        // finite, upper 3x3 determinant finite and non-zero
void set_instance_matrix(HostScene& S, int32_t k, const double m[16]);
void special_instance_bounds(const HostScene& S, int32_t k, const double m[16], double lo[3], double hi[3]);
int32_t refit_host_scene(HostScene& S, std::string& err);

// PLY loading (ply.cpp).  Mirrors PLYLoader.load (RT/Helpers/PLYReader.swift:54-210).
int32_t ply_load(const char* path, std::vector<double>& positions, std::vector<double>& normals,
                 std::vector<float>& texcoords, std::vector<int32_t>& indices, std::string& err);

}  // namespace myrt
