// commit.h — host side of rt_scene_commit / rt_scene_commit_ex (dynamic and deformable scenes,
// rtcore.h) and of what stages for them; the kernels are in refit.h, deform.h and rebuild.h.
// Included into render.hip after the scene, replica and option types (one translation unit, like
// query.h).  commit_impl is a short driver over the commit_* steps, which share one CommitPlan;
// rebuild_fit is the RT_COMMIT_REBUILD_FIT / RT_COMMIT_REBUILD_FIT_CLUSTERED step.  A commit runs under the scene lock with no render
// in flight; its scratch lives in the replica's DevArrays, a rebuild's in one RebuildScratch.
#pragma once

using CommitClock = std::chrono::steady_clock;
static double ms_since(CommitClock::time_point t) {
    return std::chrono::duration<double, std::milli>(CommitClock::now() - t).count();
}

// Blocks of 256 threads (kBoundsBlock, kDeformBlock, kRbBlock) for `items` threads, one at least
static dim3 blocks_for(int64_t items) { return dim3((unsigned)std::max<int64_t>(1, (items + 255) / 256)); }
static_assert(dev::kBoundsBlock == 256 && dev::kDeformBlock == 256 && dev::kRbBlock == 256, "blocks_for");

#define COMMIT_TRY(expr) do { const int32_t _rc = (expr); if (_rc != RT_OK) return _rc; } while (0)

// Every replica's stream has run dry
static int32_t sync_replicas(rt_scene* s) {
    for (DeviceReplica& r : s->devs) {
        HIP_TRY(hipSetDevice(r.device));
        HIP_TRY(hipStreamSynchronize(r.stream));
    }
    return RT_OK;
}

// A launch per level of a list of nodes by level, deepest first (off: level l is list[off[l],
// off[l + 1])): launch(grid, the level's nodes, their count), per_node threads for each node
template <class Launch>
static void launch_levels(const std::vector<int64_t>& off, const int32_t* list, int per_node, Launch launch) {
    for (size_t l = 0; l + 1 < off.size(); ++l) {
        const int32_t count = (int32_t)(off[l + 1] - off[l]);
        if (count > 0) launch(blocks_for(per_node * (int64_t)count), list + off[l], count);
    }
}

// The level lists of a tree whose levels are contiguous node ranges, the root level at first_node:
// deepest level first, as the device refits them
static RefitLevels levels_from_counts(int64_t first_node, const std::vector<int64_t>& level_count) {
    RefitLevels L;
    int64_t end = first_node;
    for (const int64_t c : level_count) end += c;
    for (size_t l = level_count.size(); l-- > 0;) {
        L.off.push_back((int64_t)L.nodes.size());
        for (int64_t k = end - level_count[l]; k < end; ++k) L.nodes.push_back((int32_t)k);
        end -= level_count[l];
    }
    L.off.push_back((int64_t)L.nodes.size());
    return L;
}

// ---- staging and getters ----------------------------------------------------------------------------
int32_t rt_scene_instance_of_object(const rt_scene* s, int32_t object_index, int32_t* instance) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!instance) return fail(RT_ERR_INVALID_ARG, "instance is NULL");
    if (object_index < 0 || object_index >= (int32_t)s->host.object_inst.size())
        return fail(RT_ERR_INVALID_ARG, "bad object index");
    *instance = s->host.object_inst[(size_t)object_index];
    return RT_OK;
}

int32_t rt_scene_set_instance_transform(rt_scene* s, int32_t instance, const double m[16]) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!s->host.dynamic) return fail(RT_ERR_UNSUPPORTED, "not a dynamic scene (rt_scene_create_ex, RT_SCENE_DYNAMIC)");
    if (instance < 0 || instance >= (int32_t)s->host.insts.size()) return fail(RT_ERR_INVALID_ARG, "bad instance index");
    if (!m || !matrix_ok(m))
        return fail(RT_ERR_INVALID_ARG, "localToWorld must be finite with a non-zero, finite upper 3x3 determinant");
    std::array<double, 16> a;
    std::memcpy(a.data(), m, sizeof(double) * 16);
    std::lock_guard<std::mutex> lock(s->mu);
    for (auto& e : s->staged)
        if (e.first == instance) { e.second = a; return RT_OK; }
    s->staged.push_back({instance, a});
    return RT_OK;
}

int32_t rt_scene_instance_bounds(const rt_scene* s, int32_t instance, double lo[3], double hi[3]) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!lo || !hi) return fail(RT_ERR_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lock(const_cast<rt_scene*>(s)->mu);
    if (instance < 0 || 6 * (size_t)instance + 6 > s->host.inst_bounds.size())
        return fail(RT_ERR_INVALID_ARG, "bad instance index");
    const double* b = &s->host.inst_bounds[6 * (size_t)instance];
    for (int k = 0; k < 3; ++k) { lo[k] = b[k]; hi[k] = b[3 + k]; }
    return RT_OK;
}

// Instance visibility (rtcore.h "instance visibility"): staged like a transform, applied by a commit
// visible: one byte per instance of [first, first + count), or null: `one` for all of them
static int32_t stage_visible(rt_scene* s, int32_t first, int32_t count, const uint8_t* visible, int32_t one) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!s->host.dynamic) return fail(RT_ERR_UNSUPPORTED, "not a dynamic scene (rt_scene_create_ex, RT_SCENE_DYNAMIC)");
    const int64_t n = (int64_t)s->host.insts.size();
    if (first < 0 || count < 0 || (int64_t)first + count > n) return fail(RT_ERR_INVALID_ARG, "bad instance index or range");
    try {
        std::lock_guard<std::mutex> lock(s->mu);
        if (s->staged_vis.empty()) s->staged_vis.assign((size_t)n, -1);      // -1: nothing staged for the instance
        for (int32_t k = 0; k < count; ++k) s->staged_vis[(size_t)(first + k)] = (int8_t)((visible ? visible[k] : one) ? 1 : 0);
        return RT_OK;
    } catch (const std::bad_alloc&) {
        return fail(RT_ERR_OOM, "host allocation failed");
    }
}
int32_t rt_scene_set_instance_visible(rt_scene* s, int32_t instance, int32_t visible) {
    return stage_visible(s, instance, 1, nullptr, visible ? 1 : 0);
}
int32_t rt_scene_set_instances_visible(rt_scene* s, int32_t first, int32_t count, const uint8_t* visible) {
    if (s && s->host.dynamic && !visible) return fail(RT_ERR_INVALID_ARG, "visible is NULL");
    return stage_visible(s, first, count, visible, 0);
}
int32_t rt_scene_instance_visible(const rt_scene* s, int32_t instance, int32_t* visible) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!visible) return fail(RT_ERR_INVALID_ARG, "visible is NULL");
    std::lock_guard<std::mutex> lock(const_cast<rt_scene*>(s)->mu);
    if (instance < 0 || instance >= (int32_t)s->host.insts.size()) return fail(RT_ERR_INVALID_ARG, "bad instance index");
    *visible = s->host.dyn.is_visible((size_t)instance) ? 1 : 0;
    return RT_OK;
}
// The pairs of the flattened instance tree whose instance `flag` marks (null: all of them)
static int64_t pairs_flagged(const HostScene& S, const std::vector<uint8_t>* flag) {
    if (!flag || flag->empty()) return (int64_t)S.fpairs.size();
    int64_t c = 0;
    for (const DFitPair& p : S.fpairs) c += (*flag)[(size_t)p.inst] ? 1 : 0;
    return c;
}
static bool has_fit_tree(const HostScene& S) { return S.fit_root >= 0 && S.wide_copy > 0 && !S.winst.empty(); }
// The counts as the host holds them now (they change at a commit only); shown, hidden and
// forced_rebuild are the last commit's
int32_t rt_scene_last_visibility_stats(const rt_scene* s, rt_visibility_stats* out) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!out) return fail(RT_ERR_INVALID_ARG, "out is NULL");
    std::lock_guard<std::mutex> lock(const_cast<rt_scene*>(s)->mu);
    const HostScene& S = s->host;
    rt_visibility_stats v = s->last_vis;
    v.instances = (int64_t)S.insts.size();
    v.visible = S.dynamic ? S.dyn.n_visible : v.instances;
    const bool tree = has_fit_tree(S);
    v.pairs = tree ? (int64_t)S.fpairs.size() : 0;
    v.pairs_visible = tree ? pairs_flagged(S, &S.dyn.visible) : 0;
    v.pairs_in_tree = tree ? pairs_flagged(S, &S.dyn.in_tree) : 0;
    v.fit_complete = tree && !S.dyn.fit_incomplete ? 1 : 0;
    *out = v;
    return RT_OK;
}

// The BLAS an RT_OBJ_MESH object produced, through the retained object -> BLAS map (a mesh whose id
// a MeshInstance took over has no instance of its own, but its BLAS is still used); -1: none
static int32_t deform_blas_of(const rt_scene* s, int32_t object_index) {
    const HostScene& S = s->host;
    if (object_index < 0 || object_index >= (int32_t)S.object_blas.size()) return -1;
    const int32_t b = S.object_blas[(size_t)object_index];
    if (b < 0 || (size_t)b >= S.def.blas.size() || S.def.blas[(size_t)b].verts <= 0) return -1;
    return b;
}

int32_t rt_scene_mesh_vertex_count(const rt_scene* s, int32_t object_index, int64_t* num_positions) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!num_positions) return fail(RT_ERR_INVALID_ARG, "num_positions is NULL");
    if (!s->host.deformable) return fail(RT_ERR_UNSUPPORTED, "not a deformable scene (rt_scene_create_ex, RT_SCENE_DEFORMABLE)");
    const int32_t b = deform_blas_of(s, object_index);
    if (b < 0) return fail(RT_ERR_INVALID_ARG, "object is not a mesh with triangles");
    *num_positions = s->host.def.blas[(size_t)b].verts;
    return RT_OK;
}

int32_t rt_scene_set_mesh_positions(rt_scene* s, int32_t object_index, const double* positions, int64_t num_positions,
                                    const double* normals, uint32_t flags) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!s->host.deformable) return fail(RT_ERR_UNSUPPORTED, "not a deformable scene (rt_scene_create_ex, RT_SCENE_DEFORMABLE)");
    if (flags & ~RT_POSITIONS_DEVICE) return fail(RT_ERR_INVALID_ARG, "unknown flags");
    const int32_t b = deform_blas_of(s, object_index);
    if (b < 0) return fail(RT_ERR_INVALID_ARG, "object is not a mesh with triangles");
    const DeformBlas& f = s->host.def.blas[(size_t)b];
    if (!positions || num_positions != f.verts) return fail(RT_ERR_INVALID_ARG, "num_positions must equal the mesh's vertex count");
    if (normals && f.normals != kNormalsSupplied)
        return fail(RT_ERR_INVALID_ARG, "the mesh derives its normals from its positions: normals must be NULL");
    try {
        rt_scene::StagedDeform sd;
        sd.blas = b;
        sd.has_nrm = normals != nullptr;
        if (flags & RT_POSITIONS_DEVICE) {
            for (const double* p : {positions, normals}) {
                if (!p) continue;
                hipPointerAttribute_t at{};
                const bool known = hipPointerGetAttributes(&at, p) == hipSuccess;
                if (!known) (void)hipGetLastError();
                if (!known || at.type != hipMemoryTypeDevice) return fail(RT_ERR_UNSUPPORTED, "RT_POSITIONS_DEVICE: not a device pointer");
                for (const DeviceReplica& r : s->devs)
                    if (r.device != at.device)
                        return fail(RT_ERR_UNSUPPORTED, "RT_POSITIONS_DEVICE: every replica must be on the device that owns the buffer");
            }
            sd.dpos = positions;
            sd.dnrm = normals;
        } else {
            sd.pos.assign(positions, positions + 3 * num_positions);
            if (normals) sd.nrm.assign(normals, normals + 3 * num_positions);
        }
        std::lock_guard<std::mutex> lock(s->mu);
        for (auto& e : s->staged_deform)
            if (e.blas == b) { e = std::move(sd); return RT_OK; }
        s->staged_deform.push_back(std::move(sd));
        return RT_OK;
    } catch (const std::bad_alloc&) {
        return fail(RT_ERR_OOM, "host allocation failed");
    }
}

template <class Stats>
static int32_t last_stats(const rt_scene* s, Stats rt_scene::*which, Stats* out) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!out) return fail(RT_ERR_INVALID_ARG, "out is NULL");
    std::lock_guard<std::mutex> lock(const_cast<rt_scene*>(s)->mu);
    *out = s->*which;
    return RT_OK;
}
int32_t rt_scene_last_deform_stats(const rt_scene* s, rt_deform_stats* out) { return last_stats(s, &rt_scene::last_deform, out); }
int32_t rt_scene_last_rebuild_stats(const rt_scene* s, rt_rebuild_stats* out) { return last_stats(s, &rt_scene::last_rebuild, out); }
int32_t rt_scene_last_rebuild_detail(const rt_scene* s, rt_rebuild_detail* out) { return last_stats(s, &rt_scene::last_detail, out); }

// ---- shared by the steps ------------------------------------------------------------------------------
// World bounds of the moved triangle-mesh instances, on replica 0 (refit.h k_inst_bounds)
// Partial unions k_inst_bounds writes per instance when the largest mesh among them has `most` triangles
static int bounds_parts(int64_t most) {
    return (int)std::min<int64_t>(64, (std::max<int64_t>(most, 1) + dev::kBoundsBlock * 8 - 1) / (dev::kBoundsBlock * 8));
}
// Replica 0's scratch for the bounds of n instances.  A commit reserves it for both of its
// reductions before it writes anything (commit_reserve); device_instance_bounds then finds it there.
static int32_t reserve_instance_bounds(rt_scene* s, int64_t n, int64_t part_doubles) {
    if (n == 0) return RT_OK;
    DeviceReplica& r = s->devs[0];
    HIP_TRY(hipSetDevice(r.device));
    AllocGate& g = s->gate;
    if (!r.moves.grow(g, n) || !r.bounds_out.grow(g, 6 * n) || !r.bounds_part.grow(g, part_doubles))
        return fail(RT_ERR_OOM, "device allocation failed (instance bounds scratch)");
    return RT_OK;
}
static int32_t device_instance_bounds(rt_scene* s, const std::vector<dev::RefitMove>& moves, std::vector<double>& out) {
    DeviceReplica& r = s->devs[0];
    const int64_t n = (int64_t)moves.size();
    out.assign(6 * (size_t)n, 0.0);
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(r.device));
    int64_t most = 1;
    for (const dev::RefitMove& m : moves) most = std::max<int64_t>(most, m.tri_end - m.tri_first);
    const int parts = bounds_parts(most);
    COMMIT_TRY(reserve_instance_bounds(s, n, 6 * n * parts));
    HIP_TRY(hipMemcpy(r.moves, moves.data(), (size_t)n * sizeof(dev::RefitMove), hipMemcpyHostToDevice));
    const CTri* ct = s->host.compact_tris ? r.ctris : nullptr;
    if (!ct && !r.pbox) return fail(RT_ERR_DEVICE, "dynamic scene without triangle boxes");
    constexpr int64_t kBatch = 32768;                       // gridDim.y
    for (int64_t b = 0; b < n; b += kBatch) {
        const int64_t nb = std::min(kBatch, n - b);
        hipLaunchKernelGGL(dev::k_inst_bounds, dim3((unsigned)parts, (unsigned)nb), dim3(dev::kBoundsBlock), 0, r.stream, ct,
                           r.pbox, r.moves + b, r.bounds_part + (size_t)b * parts * 6);
    }
    hipLaunchKernelGGL(dev::k_fold_boxes, dim3((unsigned)n), dim3(64), 0, r.stream, r.bounds_part.p, parts, r.bounds_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r.stream));
    HIP_TRY(hipMemcpy(out.data(), r.bounds_out, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

// Listed nodes' eight octant copies again (refit.h k_octant_copies)
static void octant_copies(const DeviceReplica& r, W4Node* wnodes, const int32_t* list, int64_t count, int64_t copy_nodes) {
    hipLaunchKernelGGL(dev::k_octant_copies, blocks_for(count), dim3(256), 0, r.stream, wnodes, list, count, copy_nodes);
}

// One four-wide tree of a replica brought up to date: a launch per level, deepest first, then the
// eight octant copies of its nodes (refit.h).  marker_base >= 0: the TLAS's tree; < 0: the fit tree
static void refit_tree(const HostScene& S, DeviceReplica& r, const RefitLevels& L, const int32_t* list, int32_t marker_base) {
    if (L.nodes.empty() || !list) return;
    const dev::TreeSlotBox box{marker_base, r.winst, r.fpairs, r.lbox, r.insts};
    launch_levels(L.off, list, 4, [&](dim3 grid, const int32_t* nodes, int32_t count) {
        hipLaunchKernelGGL(dev::k_refit_level<dev::TreeSlotBox>, grid, dim3(256), 0, r.stream, r.wnodes, nodes, count, box);
    });
    octant_copies(r, r.wnodes, list, (int64_t)L.nodes.size(), S.wide_copy);
}

static bool blurred(const DynBlas& y) { return !(y.motion[0] == 0 && y.motion[1] == 0 && y.motion[2] == 0); }

// ---- the flattened instance tree rebuilt for the committed pose (rtcore.h RT_COMMIT_REBUILD_FIT;
// rebuild.h).  Every replica builds the new tree beside the old one on its own
// stream; only when all of them hold a valid tree are the node arrays swapped, so a guard that
// trips (depth, the 4 GB offset limit, an allocation) leaves every replica with the old tree.
// Scratch of one rebuild: one allocation carved into 256-byte aligned parts, freed on every path.
// n pairs, n - 1 binary nodes, at most n - 1 four-wide nodes (each takes the subtree of a binary
// node of its own).
struct RebuildScratch {                           // RebuildScratch m{}: every pointer null
    char* base = nullptr;
    size_t sort_bytes = 0, scan_bytes = 0;        // hipcub's temporary storage
    double *pbox, *partial, *ubox, *nbox;
    unsigned long long *keys0, *keys1;
    uint32_t *vals0, *vals1;
    unsigned* arrive;
    int32_t *left, *right, *parent, *leaf_parent, *cur, *next, *slots, *cnt, *off;
    W4Node* wn;
    char *sort_tmp, *scan_tmp;
    // the clustered builder's (rebuild.h k_pc_*): two cluster arrays, neighbours, flag words and their scan
    int32_t *cref[2], *nbr;
    double* cbox[2];
    unsigned long long *word, *wscan;
    // Points every part into the allocation at `at` and returns the bytes they take together
    // (called with nullptr first, for the size); nc = n for the clustered builder, else 0
    size_t carve(char* at, int64_t n, int parts, int64_t nc) {
        size_t total = 0;
        auto take = [&](auto*& p, int64_t count) {
            p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(at) + total);
            total += ((size_t)std::max<int64_t>(count, 1) * sizeof(*p) + 255) & ~size_t(255);
        };
        take(pbox, 6 * n); take(partial, 6 * (int64_t)parts); take(ubox, 6); take(nbox, 6 * n);
        take(keys0, n); take(keys1, n); take(vals0, n); take(vals1, n); take(arrive, n);
        take(left, n); take(right, n); take(parent, n); take(leaf_parent, n);
        take(cur, n); take(next, n); take(slots, 4 * n); take(cnt, n + 1); take(off, n + 1);
        take(wn, n); take(sort_tmp, (int64_t)sort_bytes); take(scan_tmp, (int64_t)scan_bytes);
        take(cref[0], nc); take(cref[1], nc); take(nbr, nc); take(cbox[0], 6 * nc); take(cbox[1], 6 * nc);
        take(word, nc + 1); take(wscan, nc + 1);
        return total;
    }
    ~RebuildScratch() { (void)hipFree(base); }
};
struct RebuiltTree {                              // what one replica built
    W4Node* wnodes = nullptr;                     // eight copies of main nodes + new fit nodes
    int32_t* levels = nullptr;                    // the new fit_levels list on the device
    std::vector<int64_t> level_count;             // nodes per level, root first
    int64_t nodes = 0;
    int32_t reason = RT_REBUILD_NONE;
    double sort_ms = 0.0, build_ms = 0.0, cluster_ms = 0.0;
    int32_t iterations = 0, fell_back = 0;        // of the clustered builder
    const int32_t* live = nullptr;                // while it is built: live pair -> pair (null: the same)
    void drop() { (void)hipFree(wnodes); (void)hipFree(levels); wnodes = nullptr; levels = nullptr; }
};

// Four-wide nodes from the binary tree, a level per pass: the level's nodes are wn[base, base + count).
// A guard that trips sets R.reason.
static int32_t rebuild_collapse(const HostScene& S, DeviceReplica& r, int64_t n, int64_t depth_cap, RebuildScratch& m,
                                RebuiltTree& R) {
    const int64_t n_main = S.fit_root;
    hipStream_t st = r.stream;
    HIP_TRY(hipMemsetAsync(m.cur, 0, sizeof(int32_t), st));                 // the root: binary node 0
    int64_t base = 0, count = 1;
    for (;;) {
        if ((int64_t)R.level_count.size() + 1 > depth_cap) { R.reason = RT_REBUILD_TOO_DEEP; return RT_OK; }
        if (8 * (size_t)(n_main + base + count) * sizeof(W4Node) >= (size_t(1) << 32)) { R.reason = RT_REBUILD_TOO_LARGE; return RT_OK; }
        if (base + count > n - 1) return fail(RT_ERR_DEVICE, "rebuild: more four-wide nodes than binary nodes");
        dev::RbLevel L{};
        L.left = m.left; L.right = m.right; L.nbox = m.nbox; L.pbox = m.pbox; L.sorted = m.vals1; L.live = R.live; L.cur = m.cur;
        L.count = (int32_t)count; L.slots = m.slots; L.cnt = m.cnt; L.off = m.off; L.next = m.next; L.nodes = m.wn + base;
        L.child_base = (int32_t)(n_main + base + count);
        hipLaunchKernelGGL(dev::k_rb_collapse, blocks_for(count + 1), dim3(dev::kRbBlock), 0, st, L);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(m.scan_tmp, m.scan_bytes, m.cnt, m.off, (int)(count + 1), st));
        hipLaunchKernelGGL(dev::k_rb_emit, blocks_for(4 * count), dim3(dev::kRbBlock), 0, st, L);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        int32_t total = 0;
        HIP_TRY(hipMemcpy(&total, m.off + count, sizeof(total), hipMemcpyDeviceToHost));
        R.level_count.push_back(count);
        base += count;
        if (total <= 0) break;
        count = total;
        std::swap(m.cur, m.next);
    }
    R.nodes = base;
    return RT_OK;
}

// The binary tree over the sorted pairs by clustering (rebuild.h k_pc_*): an iteration ends with one
// synchronise and a four-byte read-back of the new cluster count, as a collapse level does.  false
// in `built`: more than iter_cap iterations - the caller builds the Morton tree instead.
static int32_t rebuild_cluster(DeviceReplica& r, int64_t n, int64_t iter_cap, RebuildScratch& m, RebuiltTree& R, bool& built) {
    const auto t0 = CommitClock::now();
    hipStream_t st = r.stream;
    built = false;
    hipLaunchKernelGGL(dev::k_pc_init, blocks_for(n), dim3(dev::kRbBlock), 0, st, (const uint32_t*)m.vals1, (const double*)m.pbox, n,
                       m.cref[0], m.cbox[0]);
    HIP_TRY(hipGetLastError());
    int64_t count = n, next_id = n - 2;
    int at = 0;
    while (count > 1) {
        if (R.iterations >= iter_cap) { R.cluster_ms = ms_since(t0); return RT_OK; }
        const dim3 grid = blocks_for(count + 1), block(dev::kRbBlock);
        hipLaunchKernelGGL(dev::k_pc_neighbour, grid, block, 0, st, (const double*)m.cbox[at], (int32_t)count, m.nbr);
        hipLaunchKernelGGL(dev::k_pc_merge, grid, block, 0, st, (const int32_t*)m.nbr, (int32_t)count, m.word);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(m.scan_tmp, m.scan_bytes, m.word, m.wscan, (int)(count + 1), st));
        dev::PcStep P{};
        P.ref = m.cref[at]; P.box = m.cbox[at]; P.nbr = m.nbr; P.word = m.word; P.scan = m.wscan;
        P.count = (int32_t)count; P.next_id = (int32_t)next_id; P.nodes = (int32_t)(n - 1);
        P.oref = m.cref[at ^ 1]; P.obox = m.cbox[at ^ 1]; P.left = m.left; P.right = m.right; P.nbox = m.nbox;
        hipLaunchKernelGGL(dev::k_pc_compact, grid, block, 0, st, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t alive = 0;                                  // the low half of the totals: the clusters left
        HIP_TRY(hipMemcpy(&alive, m.wscan + count, sizeof(alive), hipMemcpyDeviceToHost));
        if (alive < 1u || (int64_t)alive >= count) return fail(RT_ERR_DEVICE, "rebuild: a clustering iteration merged nothing");
        next_id -= count - (int64_t)alive;
        count = (int64_t)alive;
        at ^= 1;
        ++R.iterations;
    }
    if (next_id != -1) return fail(RT_ERR_DEVICE, "rebuild: the clustering did not end at the root");
    R.cluster_ms = ms_since(t0);
    built = true;
    return RT_OK;
}

// The live pairs of one replica in ascending order (rebuild.h k_rb_live_*): flags, their exclusive
// scan, the scatter.  One allocation, freed with the struct; live stays null when it failed.
struct LivePairs {
    char* base = nullptr;
    int32_t* live = nullptr;
    ~LivePairs() { (void)hipFree(base); }
};
static int32_t rebuild_live_pairs(const HostScene& S, DeviceReplica& r, AllocGate& gate, int64_t n_live, LivePairs& lp,
                                  RebuiltTree& R) {
    const int64_t n_all = (int64_t)S.fpairs.size();
    hipStream_t st = r.stream;
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int32_t*)nullptr, (int32_t*)nullptr, (int)(n_all + 1), st));
    const size_t words = pad((size_t)(n_all + 1) * sizeof(int32_t));
    if (!gate.alloc((void**)&lp.base, 3 * words + pad(scan_bytes))) {
        R.reason = RT_REBUILD_NO_MEMORY;
        return RT_OK;
    }
    int32_t* flag = (int32_t*)lp.base;
    int32_t* place = (int32_t*)(lp.base + words);
    int32_t* live = (int32_t*)(lp.base + 2 * words);
    hipLaunchKernelGGL(dev::k_rb_live_flags, blocks_for(n_all + 1), dim3(dev::kRbBlock), 0, st, (const DFitPair*)r.fpairs,
                       (const DInstance*)r.insts, n_all, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(lp.base + 3 * words, scan_bytes, flag, place, (int)(n_all + 1), st));
    hipLaunchKernelGGL(dev::k_rb_live_scatter, blocks_for(n_all), dim3(dev::kRbBlock), 0, st, (const int32_t*)flag,
                       (const int32_t*)place, n_all, n_live, live);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    int32_t total = -1;
    HIP_TRY(hipMemcpy(&total, place + n_all, sizeof(total), hipMemcpyDeviceToHost));
    if ((int64_t)total != n_live) return fail(RT_ERR_DEVICE, "rebuild: the device and the host count different live pairs");
    lp.live = live;
    return RT_OK;
}

// n_live: the pairs of the visible instances (the host's count); fewer than all of them: the tree is
// built over those alone
static int32_t rebuild_fit_on(const HostScene& S, DeviceReplica& r, AllocGate& gate, int64_t depth_cap, bool clustered,
                              int64_t iter_cap, int64_t n_live, RebuiltTree& R) {
    HIP_TRY(hipSetDevice(r.device));
    const auto t0 = CommitClock::now();
    const int64_t n = n_live;
    hipStream_t st = r.stream;
    LivePairs lp;
    if (n_live < (int64_t)S.fpairs.size()) {
        const int32_t rc = rebuild_live_pairs(S, r, gate, n_live, lp, R);
        if (rc != RT_OK || R.reason != RT_REBUILD_NONE) return rc;
    }
    R.live = lp.live;
    const int parts = (int)std::min<int64_t>(dev::kRbParts, (n + dev::kRbBlock - 1) / dev::kRbBlock);
    RebuildScratch m{};                                      // null pointers: hipcub only says what it needs
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, m.sort_bytes, m.keys0, m.keys1, m.vals0, m.vals1, (int)n, 0, 63, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, m.scan_bytes, m.cnt, m.off, (int)n, st));
    if (clustered) {
        size_t words = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, words, m.word, m.wscan, (int)(n + 1), st));
        m.scan_bytes = std::max(m.scan_bytes, words);
    }
    const size_t total = m.carve(nullptr, n, parts, clustered ? n : 0);
    if (!gate.alloc((void**)&m.base, total)) {
        R.reason = RT_REBUILD_NO_MEMORY;
        return RT_OK;
    }
    m.carve(m.base, n, parts, clustered ? n : 0);
    // 1. pair boxes and their union, Morton codes, the stable sort
    hipLaunchKernelGGL(dev::k_rb_pair_boxes, dim3((unsigned)parts), dim3(dev::kRbBlock), 0, st, (const DFitPair*)r.fpairs,
                       (const double*)r.lbox, (const DInstance*)r.insts, (const int32_t*)lp.live, n, m.pbox, m.partial);
    hipLaunchKernelGGL(dev::k_fold_boxes, dim3(1), dim3(64), 0, st, (const double*)m.partial, parts, m.ubox);
    hipLaunchKernelGGL(dev::k_rb_morton, blocks_for(n), dim3(dev::kRbBlock), 0, st, (const double*)m.pbox, (const double*)m.ubox, n,
                       m.keys0, m.vals0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(m.sort_tmp, m.sort_bytes, m.keys0, m.keys1, m.vals0, m.vals1, (int)n, 0, 63, st));
    HIP_TRY(hipStreamSynchronize(st));
    R.sort_ms = ms_since(t0);
    const auto t1 = CommitClock::now();
    // 2. the binary tree and its boxes: clustered, or the radix tree (also when the clustering gave up)
    bool built = false;
    if (clustered) {
        const int32_t rc = rebuild_cluster(r, n, iter_cap, m, R, built);
        if (rc != RT_OK) return rc;
        R.fell_back = built ? 0 : 1;
    }
    if (!built) {
        dev::RbTree T{};
        T.keys = m.keys1; T.n = (int32_t)n; T.left = m.left; T.right = m.right; T.parent = m.parent; T.leaf_parent = m.leaf_parent;
        HIP_TRY(hipMemsetAsync(m.arrive, 0, (size_t)n * sizeof(unsigned), st));
        hipLaunchKernelGGL(dev::k_rb_hierarchy, blocks_for(n - 1), dim3(dev::kRbBlock), 0, st, T);
        hipLaunchKernelGGL(dev::k_rb_node_boxes, blocks_for(n), dim3(dev::kRbBlock), 0, st, T, (const uint32_t*)m.vals1,
                           (const double*)m.pbox, m.arrive, m.nbox);
        HIP_TRY(hipGetLastError());
    }
    // 3. four-wide nodes level by level
    const int32_t rc = rebuild_collapse(S, r, n, depth_cap, m, R);
    if (rc != RT_OK || R.reason != RT_REBUILD_NONE) return rc;
    // 4. the new node array: the eight main parts as they are, the new fit nodes behind copy 0's,
    //    then their octant copies (over the level list, deepest level first)
    const int64_t n_main = S.fit_root, new_copy = n_main + R.nodes;
    if (!gate.alloc((void**)&R.wnodes, (size_t)(8 * new_copy) * sizeof(W4Node)) ||
        !gate.alloc((void**)&R.levels, (size_t)R.nodes * sizeof(int32_t))) {
        R.drop();
        R.reason = RT_REBUILD_NO_MEMORY;
        return RT_OK;
    }
    for (int o = 0; o < 8 && n_main > 0; ++o)
        HIP_TRY(hipMemcpyAsync(R.wnodes + (size_t)o * new_copy, r.wnodes + (size_t)o * S.wide_copy, (size_t)n_main * sizeof(W4Node),
                               hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(R.wnodes + n_main, m.wn, (size_t)R.nodes * sizeof(W4Node), hipMemcpyDeviceToDevice, st));
    const std::vector<int32_t> list = levels_from_counts(n_main, R.level_count).nodes;
    HIP_TRY(hipMemcpyAsync(R.levels, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    octant_copies(r, R.wnodes, R.levels, R.nodes, new_copy);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    R.build_ms = ms_since(t1);
    return RT_OK;
}

// The cost of the fit tree replica r holds (rebuild.h k_fit_cost; rt_scene_fit_cost); 0 without one.
// The partial sums go through the replica's bounds scratch: the scene lock is held.
static int32_t fit_cost_on(const HostScene& S, DeviceReplica& r, AllocGate& gate, double* cost) {
    *cost = 0.0;
    if (S.fit_root < 0 || S.fit_nodes <= 0 || S.wide_copy <= 0 || !r.wnodes) return RT_OK;
    HIP_TRY(hipSetDevice(r.device));
    if (!r.bounds_part.grow(gate, dev::kFcBlocks + 1)) return fail(RT_ERR_OOM, "device allocation failed (tree cost scratch)");
    const W4Node* fit = r.wnodes + S.fit_root;
    hipLaunchKernelGGL(dev::k_fit_cost, dim3(dev::kFcBlocks), dim3(dev::kRbBlock), 0, r.stream, fit, S.fit_nodes, r.bounds_part.p);
    hipLaunchKernelGGL(dev::k_fit_cost_fold, dim3(1), dim3(64), 0, r.stream, (const double*)r.bounds_part.p, dev::kFcBlocks, fit,
                       r.bounds_part.p + dev::kFcBlocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r.stream));
    HIP_TRY(hipMemcpy(cost, r.bounds_part.p + dev::kFcBlocks, sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int32_t rt_scene_fit_cost(rt_scene* s, double* cost) {
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (!cost) return fail(RT_ERR_INVALID_ARG, "cost is NULL");
    *cost = 0.0;
    if (!s->host.dynamic) return fail(RT_ERR_UNSUPPORTED, "not a dynamic scene (rt_scene_create_ex, RT_SCENE_DYNAMIC)");
    std::lock_guard<std::mutex> lock(s->mu);
    COMMIT_TRY(scene_lost(s));
    if (scene_busy(s)) return fail(RT_ERR_BUSY, "renders of the scene are in flight: wait for them first");
    if (s->devs.empty() || s->host.winst.empty()) return RT_OK;
    return fit_cost_on(s->host, s->devs[0], s->gate, cost);
}

// The rebuild step of a commit (the scene lock is held, no render is in flight).  Returns RT_OK
// also when nothing was rebuilt (s->last_rebuild says why); an error only for a device failure.
// clustered: RT_COMMIT_REBUILD_FIT_CLUSTERED; s->last_detail says which builder made the tree.
static int32_t rebuild_fit(rt_scene* s, bool clustered) {
    const auto t0 = CommitClock::now();
    HostScene& S = s->host;
    rt_rebuild_stats st{};
    rt_rebuild_detail dt{};
    const bool has = has_fit_tree(S);
    const int64_t n_live = has ? pairs_flagged(S, &S.dyn.visible) : 0;     // the tree holds the visible pairs only
    st.pairs = has ? (int64_t)S.fpairs.size() : 0;
    st.nodes_before = st.nodes_after = has ? S.fit_nodes : 0;
    st.depth_before = st.depth_after = has ? S.fit_depth : 0;
    auto done = [&](int32_t reason) {
        st.reason = reason;
        st.rebuilt = reason == RT_REBUILD_NONE ? 1 : 0;
        st.total_ms = ms_since(t0);
        if (!st.rebuilt) { dt.builder = 0; dt.cost_after = dt.cost_before; }
        s->last_rebuild = st;
        s->last_detail = dt;
        return (int32_t)RT_OK;
    };
    bool tree = has && n_live >= 2 && S.fpairs.size() < (size_t(1) << 30);
    for (const DeviceReplica& r : s->devs) tree = tree && r.wnodes && r.fpairs && r.lbox && r.insts;
    if (!tree) return done(RT_REBUILD_NO_TREE);
    if (S.dyn.fit_blocked) return done(RT_REBUILD_BLOCKED);
    {   // the cost scratch is an allocation of the rebuild like the others: without it the old tree stays
        const int32_t rc = fit_cost_on(S, s->devs[0], s->gate, &dt.cost_before);
        if (rc == RT_ERR_OOM) return done(RT_REBUILD_NO_MEMORY);
        if (rc != RT_OK) return rc;
    }
    // the clustering gives up after 4 ceil(log2 n) + 32 iterations (the test hook can only lower that)
    int64_t log2n = 0;
    while ((int64_t(1) << log2n) < n_live) ++log2n;
    const int64_t iter_cap = std::min<int64_t>(4 * log2n + 32, s->opt[kOptRebuildClusterIterCap]);
    std::vector<RebuiltTree> res;
    auto drop_all = [&]() {
        for (size_t j = 0; j < res.size(); ++j) {
            (void)hipSetDevice(s->devs[j].device);
            res[j].drop();
        }
    };
    try {
        res.resize(s->devs.size());
        for (size_t k = 0; k < res.size(); ++k) {
            const int32_t rc = rebuild_fit_on(S, s->devs[k], s->gate, s->opt[kOptRebuildDepthCap], clustered, iter_cap, n_live, res[k]);
            dt.iterations = std::max(dt.iterations, res[k].iterations);
            dt.fell_back = std::max(dt.fell_back, res[k].fell_back);
            dt.cluster_ms = std::max(dt.cluster_ms, res[k].cluster_ms);
            if (rc == RT_OK && res[k].reason == RT_REBUILD_NONE && res[k].level_count == res[0].level_count) continue;
            const int32_t reason = res[k].reason;
            drop_all();
            if (rc != RT_OK) return rc;
            if (reason != RT_REBUILD_NONE) return done(reason);
            return fail(RT_ERR_DEVICE, "rebuild: the replicas built different trees");
        }
        // what the host keeps is made before anything is swapped: a host allocation that fails here
        // still leaves the old tree in use everywhere
        const RebuiltTree& R0 = res[0];
        RefitLevels new_levels = levels_from_counts(S.fit_root, R0.level_count);
        std::vector<uint8_t> new_in_tree = S.dyn.visible;
        for (size_t k = 0; k < res.size(); ++k) {
            DeviceReplica& r = s->devs[k];
            HIP_TRY(hipSetDevice(r.device));
            (void)hipFree(r.wnodes);                        // no kernel holds it: commits do not run beside renders
            (void)hipFree(r.fit_levels);
            r.wnodes = res[k].wnodes;
            r.fit_levels = res[k].levels;
            r.bytes += (8 * (res[k].nodes - S.fit_nodes)) * (int64_t)sizeof(W4Node) +
                       (res[k].nodes - (int64_t)std::max<size_t>(1, S.dyn.fit_levels.nodes.size())) * (int64_t)sizeof(int32_t);
            st.sort_ms = std::max(st.sort_ms, res[k].sort_ms);
            st.build_ms = std::max(st.build_ms, res[k].build_ms);
            res[k].wnodes = nullptr;                        // the replica's now
            res[k].levels = nullptr;
        }
        // what the host keeps: the counts renders and queries are made from, and the level lists
        // a later plain commit refits
        S.dyn.fit_levels = std::move(new_levels);
        S.wide_copy = S.fit_root + R0.nodes;
        S.fit_nodes = R0.nodes;
        S.fit_depth = (int64_t)R0.level_count.size();
        S.dyn.in_tree = std::move(new_in_tree);             // the pairs the new tree holds
        S.dyn.fit_incomplete = false;
        st.nodes_after = S.fit_nodes;
        st.depth_after = S.fit_depth;
        dt.builder = clustered && !dt.fell_back ? 2 : 1;
        COMMIT_TRY(fit_cost_on(S, s->devs[0], s->gate, &dt.cost_after));
        return done(RT_REBUILD_NONE);
    } catch (const std::bad_alloc&) {                       // thrown before the swap only
        drop_all();
        return done(RT_REBUILD_NO_MEMORY);
    }
}

// ---- the steps of a commit ------------------------------------------------------------------------
// What the steps share.  Built once the commit is known to have something staged; the staged
// transforms and deformations are swapped out of the scene, so a failed commit stages nothing.
struct CommitPlan {
    std::vector<std::pair<int32_t, std::array<double, 16>>> staged;   // (instance, new localToWorld)
    std::vector<rt_scene::StagedDeform> sdef;
    std::vector<int8_t> svis;                     // per instance: -1 nothing staged, else the new flag (or empty)
    std::vector<char> deformed;                   // per BLAS: new positions are staged for it
    // per staged deformation: its host arrays in a replica's def_stage, its first |e1||e2| partial in def_part
    std::vector<int64_t> pos_off, nrm_off, part_off;
    int64_t stage_total = 0, part_total = 2 * dev::kValidateParts, face_need = 0, vnorm_need = 0;
    std::vector<char> later;                      // per staged transform: its instance's mesh deforms, bounds come last
    std::vector<double> nb;                       // per staged transform: the instance's new world bounds
    std::vector<double> roots;                    // per staged deformation: root box[6], max |e1||e2|, 0 (k_blas_root)
    std::vector<int32_t> rebound;                 // the instances of the deformed meshes, by staged deformation ...
    std::vector<double> rebound_box;              // ... and their new world bounds
    rt_deform_stats dst{};
    rt_visibility_stats vst{};
    double bounds_ms = 0.0;
    CommitClock::time_point t0;

    CommitPlan(rt_scene* s, CommitClock::time_point start) : t0(start) {
        const HostScene& S = s->host;
        staged.swap(s->staged);
        sdef.swap(s->staged_deform);
        svis.swap(s->staged_vis);
        deformed.assign(S.dyn.blas.size(), 0);
        later.assign(staged.size(), 0);
        nb.assign(6 * staged.size(), 0.0);
        int64_t blocks = 0;
        for (const rt_scene::StagedDeform& sd : sdef) {
            deformed[(size_t)sd.blas] = 1;
            const DeformBlas& f = S.def.blas[(size_t)sd.blas];
            const int64_t nt = S.dyn.blas[(size_t)sd.blas].tri_end - S.dyn.blas[(size_t)sd.blas].tri_first;
            pos_off.push_back(stage_total); stage_total += (int64_t)sd.pos.size();
            nrm_off.push_back(stage_total); stage_total += (int64_t)sd.nrm.size();
            part_off.push_back(blocks);
            blocks += (nt + dev::kDeformBlock - 1) / dev::kDeformBlock;
            if (f.normals == kNormalsSmooth) {
                face_need = std::max(face_need, 3 * nt);
                vnorm_need = std::max(vnorm_need, 3 * f.verts);
            }
            dst.triangles += nt;
        }
        part_total = std::max(part_total, blocks);
        // host memory the steps past the first write need is taken here, while a failure changes nothing
        for (const rt_scene::StagedDeform& sd : sdef)
            for (size_t i = 0; i < S.dyn.inst_blas.size(); ++i)
                if (S.dyn.inst_blas[i] == sd.blas) rebound.push_back((int32_t)i);
        roots.assign(8 * sdef.size(), 0.0);
        rebound_box.reserve(6 * rebound.size());
    }
    // the matrix instance k has once this commit is through
    const double* matrix_of(const HostScene& S, int32_t k) const {
        for (const auto& e : staged)
            if (e.first == k) return e.second.data();
        return S.insts[(size_t)k].l2w;
    }
    // staged deformation m's positions / newly supplied normals (or null) as replica r sees them
    const double* pos_ptr(const DeviceReplica& r, size_t m) const { return sdef[m].dpos ? sdef[m].dpos : r.def_stage + pos_off[m]; }
    const double* nrm_ptr(const DeviceReplica& r, size_t m) const {
        return !sdef[m].has_nrm ? nullptr : sdef[m].dnrm ? sdef[m].dnrm : r.def_stage + nrm_off[m];
    }
};

static dev::RefitMove move_for(const HostScene& S, int32_t k, const double* m16) {
    const DynBlas& y = S.dyn.blas[(size_t)S.dyn.inst_blas[(size_t)k]];
    dev::RefitMove mv{};
    std::memcpy(mv.m, m16, sizeof(mv.m));
    for (int a = 0; a < 3; ++a) mv.motion[a] = y.motion[a];
    mv.tri_first = (int32_t)y.tri_first; mv.tri_end = (int32_t)y.tri_end;
    mv.blur = blurred(y) ? 1 : 0;
    return mv;
}
static dev::DeformRun run_of(const DeviceReplica& r, const DynBlas& y) {
    dev::DeformRun R{};
    R.tris = r.tris; R.pbox = r.pbox; R.tri_end = (int32_t)y.tri_end;
    R.blur = blurred(y) ? 1 : 0;
    for (int a = 0; a < 3; ++a) R.motion[a] = y.motion[a];
    return R;
}
static double matrix_reach(const double* m16) {
    double reach = 0.0;
    for (int a = 0; a < 16; ++a) reach = std::max(reach, std::fabs(m16[a]));
    return reach;
}

// Every device allocation steps 1 - 9 need, made before the first kernel that writes scene memory:
// a failure here is RT_ERR_OOM with nothing changed on any replica or on the host.  Every replica's
// deformation scratch, and replica 0's instance-bounds scratch for the larger of its two
// reductions (the moved instances, commit_moved_bounds; those of the deformed meshes,
// commit_rebound_deformed).  The arrays are kept, so a commit like the last one allocates nothing.
static int32_t commit_reserve(rt_scene* s, CommitPlan& P) {
    const HostScene& S = s->host;
    AllocGate& g = s->gate;
    if (!P.sdef.empty())
        for (DeviceReplica& r : s->devs) {
            HIP_TRY(hipSetDevice(r.device));
            if (!r.def_stage.grow(g, P.stage_total) || !r.def_part.grow(g, P.part_total) ||
                !r.def_out.grow(g, 8 * (int64_t)P.sdef.size()) || !r.def_face.grow(g, P.face_need) ||
                !r.def_vnorm.grow(g, P.vnorm_need))
                return fail(RT_ERR_OOM, "device allocation failed (deformation scratch)");
        }
    auto tris_of = [&](int32_t k) {
        const DynBlas& y = S.dyn.blas[(size_t)S.dyn.inst_blas[(size_t)k]];
        return y.tri_end - y.tri_first;
    };
    int64_t moved = 0, moved_most = 1, rebound_most = 1;
    for (const auto& e : P.staged) {
        const int32_t blas = S.dyn.inst_blas[(size_t)e.first];
        if (S.dyn.blas[(size_t)blas].kind != kPrimTriangles || P.deformed[(size_t)blas]) continue;
        ++moved;
        moved_most = std::max<int64_t>(moved_most, tris_of(e.first));
    }
    const int64_t rebound = (int64_t)P.rebound.size();
    for (const int32_t k : P.rebound) rebound_most = std::max<int64_t>(rebound_most, tris_of(k));
    return reserve_instance_bounds(s, std::max(moved, rebound),
                                   std::max(6 * moved * bounds_parts(moved_most), 6 * rebound * bounds_parts(rebound_most)));
}

// The staged host arrays in a replica's staging buffer (commit_reserve made it)
static int32_t stage_replica(DeviceReplica& r, const CommitPlan& P) {
    HIP_TRY(hipSetDevice(r.device));
    for (size_t m = 0; m < P.sdef.size(); ++m) {
        const rt_scene::StagedDeform& sd = P.sdef[m];
        if (!sd.pos.empty())
            HIP_TRY(hipMemcpy(r.def_stage + P.pos_off[m], sd.pos.data(), sd.pos.size() * sizeof(double), hipMemcpyHostToDevice));
        if (!sd.nrm.empty())
            HIP_TRY(hipMemcpy(r.def_stage + P.nrm_off[m], sd.nrm.data(), sd.nrm.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return RT_OK;
}

// Staged positions: on replica 0, then checked there before anything changes (deform.h k_deform_validate):
// all finite, and no instance of the mesh out of range under the matrix it will have
static int32_t commit_validate_positions(rt_scene* s, CommitPlan& P) {
    const size_t nd = P.sdef.size();
    if (nd == 0) return RT_OK;
    const HostScene& S = s->host;
    DeviceReplica& r = s->devs[0];
    COMMIT_TRY(stage_replica(r, P));
    for (size_t m = 0; m < nd; ++m) {
        const int64_t n3 = 3 * S.def.blas[(size_t)P.sdef[m].blas].verts;
        const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(dev::kValidateParts, (n3 + dev::kDeformBlock - 1) / dev::kDeformBlock));
        hipLaunchKernelGGL(dev::k_deform_validate, dim3((unsigned)parts), dim3(dev::kDeformBlock), 0, r.stream, P.pos_ptr(r, m), n3,
                           r.def_part.p);
        hipLaunchKernelGGL(dev::k_deform_validate_final, dim3(1), dim3(64), 0, r.stream, r.def_part.p, parts, r.def_out + 2 * m);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(r.stream));
    std::vector<double> v(2 * nd, 0.0);
    HIP_TRY(hipMemcpy(v.data(), r.def_out, v.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < nd; ++m) {
        if (!(v[2 * m] == 1.0)) return fail(RT_ERR_INVALID_ARG, "staged positions are not all finite");
        const DynBlas& y = S.dyn.blas[(size_t)P.sdef[m].blas];
        const double c = v[2 * m + 1] + std::fmax(std::fabs(y.motion[0]), std::fmax(std::fabs(y.motion[1]), std::fabs(y.motion[2])));
        for (size_t i = 0; i < S.dyn.inst_blas.size(); ++i) {
            if (S.dyn.inst_blas[i] != P.sdef[m].blas) continue;
            if (!(matrix_reach(P.matrix_of(S, (int32_t)i)) * (3.0 * c + 1.0) < 1e30))
                return fail(RT_ERR_INVALID_ARG, "staged positions put an instance of the mesh out of range");
        }
    }
    P.dst.validate_ms = ms_since(P.t0);
    return RT_OK;
}

// Instance.worldBounds of the moved instances: triangle meshes on the device, spheres and planes (one
// primitive) here; instances of a deformed mesh wait for its new triangle boxes (commit_rebound_deformed)
static int32_t commit_moved_bounds(rt_scene* s, CommitPlan& P) {
    const HostScene& S = s->host;
    const auto t = CommitClock::now();
    std::vector<dev::RefitMove> moves;
    std::vector<size_t> move_of;
    for (size_t q = 0; q < P.staged.size(); ++q) {
        const int32_t k = P.staged[q].first;
        const int32_t blas = S.dyn.inst_blas[(size_t)k];
        if (S.dyn.blas[(size_t)blas].kind != kPrimTriangles) {
            special_instance_bounds(S, k, P.staged[q].second.data(), &P.nb[6 * q], &P.nb[6 * q + 3]);
            continue;
        }
        if (P.deformed[(size_t)blas]) { P.later[q] = 1; continue; }
        moves.push_back(move_for(S, k, P.staged[q].second.data()));
        move_of.push_back(q);
    }
    std::vector<double> devb;
    COMMIT_TRY(device_instance_bounds(s, moves, devb));
    for (size_t j = 0; j < move_of.size(); ++j) std::memcpy(&P.nb[6 * move_of[j]], &devb[6 * j], 6 * sizeof(double));
    P.bounds_ms = ms_since(t);
    return RT_OK;
}

// Nothing is changed unless every moved instance stays in range (float boxes stay finite)
static int32_t commit_range_check(rt_scene* s, CommitPlan& P) {
    const HostScene& S = s->host;
    for (size_t q = 0; q < P.staged.size(); ++q) {
        if (P.later[q]) continue;
        bool ok = true;
        for (int a = 0; a < 6; ++a) ok = ok && std::isfinite(P.nb[6 * q + a]) && std::fabs(P.nb[6 * q + a]) < 1e30;
        if (!S.winst.empty())
            ok = ok && matrix_reach(P.staged[q].second.data()) * (3.0 * S.winst[(size_t)P.staged[q].first].bcoord + 1.0) < 1e30;
        if (!ok) return fail(RT_ERR_INVALID_ARG, "a staged transform puts its instance out of range");
    }
    return RT_OK;
}

// The deformations (deform.h), the same kernels on every replica's stream: triangles, triangle
// boxes, normals and leaf boxes.  From here on the device is changed.
static int32_t commit_deform_triangles(rt_scene* s, CommitPlan& P) {
    if (P.sdef.empty()) return RT_OK;
    const HostScene& S = s->host;
    const auto t = CommitClock::now();
    const dim3 block(dev::kDeformBlock);
    for (DeviceReplica& r : s->devs) {                      // before the first launch: what can still fail cleanly
        if (!r.pbox || !r.vid) return fail(RT_ERR_DEVICE, "deformable scene without triangle boxes");
        if (&r != &s->devs[0]) COMMIT_TRY(stage_replica(r, P));
    }
    for (DeviceReplica& r : s->devs) {
        HIP_TRY(hipSetDevice(r.device));
        for (size_t m = 0; m < P.sdef.size(); ++m) {
            const DeformBlas& f = S.def.blas[(size_t)P.sdef[m].blas];
            const DynBlas& y = S.dyn.blas[(size_t)P.sdef[m].blas];
            const dim3 tris = blocks_for(y.tri_end - y.tri_first);
            dev::DeformMesh M{};
            M.pos = P.pos_ptr(r, m); M.vid = r.vid;
            const double* new_nrm = P.nrm_ptr(r, m);     // newly supplied per-vertex normals, or null
            M.tri_first = (int32_t)y.tri_first; M.tri_end = (int32_t)y.tri_end;
            M.prim_base = f.prim_base; M.normals = f.normals;
            hipLaunchKernelGGL(dev::k_deform_tris, tris, block, 0, r.stream, M, r.tris, r.pbox, r.normals, r.def_face.p,
                               r.def_part + P.part_off[m]);
            if (f.normals == kNormalsSmooth) {
                hipLaunchKernelGGL(dev::k_vertex_normals, blocks_for(f.verts), block, 0, r.stream, r.csr_off + f.csr_off_first,
                                   r.csr_tri + f.csr_first, f.verts, r.def_face.p, r.def_vnorm.p);
                hipLaunchKernelGGL(dev::k_gather_normals, tris, block, 0, r.stream, r.vid, M.tri_first, M.tri_end,
                                   (const double*)r.def_vnorm, r.normals);
            } else if (f.normals == kNormalsSupplied && new_nrm) {
                hipLaunchKernelGGL(dev::k_gather_normals, tris, block, 0, r.stream, r.vid, M.tri_first, M.tri_end, new_nrm, r.normals);
            }
            if (!S.winst.empty())
                hipLaunchKernelGGL(dev::k_leaf_boxes, tris, block, 0, r.stream, run_of(r, y), M.tri_first, r.lbox);
        }
        HIP_TRY(hipGetLastError());
    }
    COMMIT_TRY(sync_replicas(s));
    P.dst.deform_ms = ms_since(t);
    return RT_OK;
}

// The deformed meshes' BLAS records and four-wide nodes, level by level, on every replica's stream;
// replica 0's root boxes and |e1||e2| come back to the host (P.roots)
static int32_t commit_refit_blas(rt_scene* s, CommitPlan& P) {
    const size_t nd = P.sdef.size();
    if (nd == 0) return RT_OK;
    const HostScene& S = s->host;
    const auto t = CommitClock::now();
    const dim3 block(dev::kDeformBlock);
    for (DeviceReplica& r : s->devs) {
        HIP_TRY(hipSetDevice(r.device));
        for (size_t m = 0; m < nd; ++m) {
            const DeformBlas& f = S.def.blas[(size_t)P.sdef[m].blas];
            const DynBlas& y = S.dyn.blas[(size_t)P.sdef[m].blas];
            const dev::DeformRun R = run_of(r, y);
            launch_levels(f.rec_off, r.rec_list, 2, [&](dim3 grid, const int32_t* recs, int32_t count) {
                hipLaunchKernelGGL(dev::k_refit_recs, grid, block, 0, r.stream, r.recs, recs, count, R);
            });
            hipLaunchKernelGGL(dev::k_blas_root, dim3(1), dim3(64), 0, r.stream, (const WRec*)r.recs, f.root_ref, R,
                               (const double*)(r.def_part + P.part_off[m]),
                               (int)((y.tri_end - y.tri_first + dev::kDeformBlock - 1) / dev::kDeformBlock), r.def_out + 8 * m);
            if (S.winst.empty() || !r.wnodes || f.wroot < 0 || f.wide_off.size() <= 1) continue;
            launch_levels(f.wide_off, r.wide_list, 4, [&](dim3 grid, const int32_t* nodes, int32_t count) {
                hipLaunchKernelGGL(dev::k_refit_level<dev::LeafRunBox>, grid, block, 0, r.stream, r.wnodes, nodes, count,
                                   dev::LeafRunBox{r.lbox});
            });
            octant_copies(r, r.wnodes, r.wide_list + f.wide_off.front(), f.wide_off.back() - f.wide_off.front(), S.wide_copy);
        }
        HIP_TRY(hipGetLastError());
    }
    COMMIT_TRY(sync_replicas(s));
    HIP_TRY(hipSetDevice(s->devs[0].device));
    HIP_TRY(hipMemcpy(P.roots.data(), s->devs[0].def_out, P.roots.size() * sizeof(double), hipMemcpyDeviceToHost));
    P.dst.blas_refit_ms = ms_since(t);
    return RT_OK;
}

// The host's copies of what a deformation changes - the pruning margin's constant, the BLAS root box
// of every instance of the mesh and the widening bound of its local rays (scene.cpp build_wide_tw:
// bcoord) - and those instances' new world bounds from the new triangle boxes
static int32_t commit_rebound_deformed(rt_scene* s, CommitPlan& P) {
    if (P.sdef.empty()) return RT_OK;
    HostScene& S = s->host;
    const auto t = CommitClock::now();
    // the device first: the host's copies are written once nothing can fail any more
    std::vector<dev::RefitMove> moves;
    for (const int32_t i : P.rebound) moves.push_back(move_for(S, i, P.matrix_of(S, i)));
    COMMIT_TRY(device_instance_bounds(s, moves, P.rebound_box));
    for (size_t m = 0; m < P.sdef.size(); ++m) {
        const double* o = &P.roots[8 * m];
        S.dyn.blas[(size_t)P.sdef[m].blas].P = o[6];
        double bc = 0.0;
        for (int a = 0; a < 6; ++a) bc = std::fmax(bc, std::fabs(o[a]));
        for (size_t i = 0; i < S.dyn.inst_blas.size(); ++i) {
            if (S.dyn.inst_blas[i] != P.sdef[m].blas) continue;
            DInstance& di = S.insts[i];
            for (int a = 0; a < 3; ++a) { di.root_lo[a] = o[a]; di.root_hi[a] = o[3 + a]; }
            if (!S.winst.empty()) S.winst[i].bcoord = bc;
        }
    }
    P.bounds_ms += ms_since(t);
    P.dst.meshes_deformed = (int64_t)P.sdef.size();
    P.dst.instances_rebounded = (int64_t)P.rebound.size();
    return RT_OK;
}

// Host: DInstance, instance bounds, then TLAS bounds bottom-up, TLAS records, tbox and the margins'
// constants (scene.cpp refit_host_scene)
// The staged visibility flags become the scene's: from here on refit_host_scene leaves the hidden
// instances out, and the upload gives their device DInstance a root box of NaNs.  Nothing here can
// un-hide: a hidden instance's host DInstance keeps (and commit_rebound_deformed rewrites) its real box.
static int32_t commit_apply_visibility(rt_scene* s, CommitPlan& P) {
    DynScene& Y = s->host.dyn;
    for (size_t i = 0; i < P.svis.size() && i < Y.visible.size(); ++i) {
        if (P.svis[i] < 0 || (P.svis[i] != 0) == (Y.visible[i] != 0)) continue;
        Y.visible[i] = P.svis[i] ? 1 : 0;
        ++(P.svis[i] ? P.vst.shown : P.vst.hidden);
    }
    Y.n_visible = 0;
    for (const uint8_t v : Y.visible) Y.n_visible += v ? 1 : 0;
    return RT_OK;
}

static int32_t commit_host_refit(rt_scene* s, CommitPlan& P) {
    HostScene& S = s->host;
    for (size_t q = 0; q < P.staged.size(); ++q) {
        set_instance_matrix(S, P.staged[q].first, P.staged[q].second.data());
        if (!P.later[q]) std::memcpy(&S.inst_bounds[6 * (size_t)P.staged[q].first], &P.nb[6 * q], 6 * sizeof(double));
    }
    for (size_t j = 0; j < P.rebound.size(); ++j)
        std::memcpy(&S.inst_bounds[6 * (size_t)P.rebound[j]], &P.rebound_box[6 * j], 6 * sizeof(double));
    std::string err;
    const int32_t rc = refit_host_scene(S, err);
    return rc == RT_OK ? rc : fail(rc, err);
}

// Every replica: instances, TLAS records, tbox; then the four-wide trees on its stream
static int32_t commit_upload_and_refit(rt_scene* s, CommitPlan&) {
    const HostScene& S = s->host;
    const DynScene& Y = S.dyn;
    // The device copy of a hidden instance has a BLAS root box of NaNs.  Every walk accepts a
    // primitive of instance k only after the FP64 slab test of k's root box with the local ray
    // (device.h, wide.h); every plane distance of a NaN box is a NaN, so tmax is one and the test
    // fails in both of slab_hit's forms: no kernel changes.  The host keeps the real box.
    std::vector<DInstance> masked;
    const std::vector<DInstance>* dinsts = &S.insts;
    if (Y.n_visible < (int64_t)S.insts.size()) {
        masked = S.insts;
        for (size_t i = 0; i < masked.size(); ++i)
            if (!Y.is_visible(i))
                for (int a = 0; a < 3; ++a) masked[i].root_lo[a] = masked[i].root_hi[a] = std::numeric_limits<double>::quiet_NaN();
        dinsts = &masked;
    }
    for (DeviceReplica& r : s->devs) {
        HIP_TRY(hipSetDevice(r.device));
        HIP_TRY(hipMemcpy(r.insts, dinsts->data(), dinsts->size() * sizeof(DInstance), hipMemcpyHostToDevice));
        if (!Y.tlas_recs.empty())
            HIP_TRY(hipMemcpy(r.recs + S.blas_records, Y.tlas_recs.data(), Y.tlas_recs.size() * sizeof(WRec),
                              hipMemcpyHostToDevice));
        if (!S.winst.empty() && r.wnodes) {
            HIP_TRY(hipMemcpy(r.winst, S.winst.data(), S.winst.size() * sizeof(DWideInst), hipMemcpyHostToDevice));
            refit_tree(S, r, Y.tlas_levels, r.tlas_levels, (int32_t)(S.tlas_leaf_base + (int64_t)S.tlas_leaf.size()));
            if (S.fit_root >= 0) refit_tree(S, r, Y.fit_levels, r.fit_levels, -1);
            HIP_TRY(hipGetLastError());
        }
    }
    return sync_replicas(s);
}

// ---- the driver ------------------------------------------------------------------------------------
// A commit ends in one of four ways (rtcore.h "how a commit ends"):
//   1  done.
//   2  refused (RT_ERR_INVALID_ARG) or out of memory (RT_ERR_OOM) before anything changed: every
//      replica, the host and the last_* stats are what they were; what was staged is dropped.
//   3  the pose committed, the tree not rebuilt for want of memory: RT_OK, RT_REBUILD_NO_MEMORY.
//   4  the scene lost: any failure once the first writing step has begun, and any HIP runtime
//      error (also before that: the device is in no known state).  RT_ERR_DEVICE now and from
//      every later call on the scene (scene_lost); no rollback, the host keeps no old positions.
// The steps are numbered for the test hook debug_fail_commit_step: 1 - 9 below, 10 the rebuild.
static int32_t commit_steps(rt_scene* s, bool rebuild, bool clustered, rt_commit_stats* stats, bool& wrote);
static int32_t commit_impl(rt_scene* s, uint32_t flags, rt_commit_stats* stats) {
    if (stats) *stats = rt_commit_stats{};
    if (!s) return fail(RT_ERR_NO_SCENE, "No scene loaded.");
    if (flags & ~(RT_COMMIT_REBUILD_FIT | RT_COMMIT_REBUILD_FIT_CLUSTERED)) return fail(RT_ERR_INVALID_ARG, "unknown commit flags");
    const bool clustered = (flags & RT_COMMIT_REBUILD_FIT_CLUSTERED) != 0;     // alone or with RT_COMMIT_REBUILD_FIT
    const bool rebuild = clustered || (flags & RT_COMMIT_REBUILD_FIT) != 0;
    if (!s->host.dynamic) return fail(RT_ERR_UNSUPPORTED, "not a dynamic scene (rt_scene_create_ex, RT_SCENE_DYNAMIC)");
    std::lock_guard<std::mutex> lock(s->mu);
    COMMIT_TRY(scene_lost(s));
    if (scene_busy(s)) return fail(RT_ERR_BUSY, "renders of the scene are in flight: wait for them first");
    // the test hooks hold for this commit alone
    s->gate.fail_at = s->opt[kOptDebugFailCommitAlloc];
    s->gate.count = 0;
    bool wrote = false;
    int32_t rc = commit_steps(s, rebuild, clustered, stats, wrote);
    s->gate.fail_at = 0;
    s->opt[kOptDebugFailCommitAlloc] = s->opt[kOptDebugFailCommitStep] = 0;
    if (rc != RT_OK && (wrote || rc == RT_ERR_DEVICE)) {
        s->lost.store(true);
        rc = fail(RT_ERR_DEVICE, "rt_scene_commit failed on the device and the scene is lost (" + g_err +
                                     "): every later call on it fails; rt_scene_destroy it and create it again");
    }
    return rc;
}
static int32_t commit_steps(rt_scene* s, bool rebuild, bool clustered, rt_commit_stats* stats, bool& wrote) {
    const auto t0 = CommitClock::now();
    const int64_t fail_step = s->opt[kOptDebugFailCommitStep];
    auto injected = [&](int k) {
        return fail_step != k ? (int32_t)RT_OK
                              : fail(RT_ERR_DEVICE, "injected failure before step " + std::to_string(k) +
                                                        " (option debug_fail_commit_step)");
    };
    if (s->staged.empty() && s->staged_deform.empty() && s->staged_vis.empty()) {
        if (rebuild) {                                       // nothing staged: the pose as it stands
            COMMIT_TRY(injected(10));
            COMMIT_TRY(rebuild_fit(s, clustered));
            drop_tile_orders(s);
        } else {
            s->last_rebuild = rt_rebuild_stats{};
            s->last_detail = rt_rebuild_detail{};
        }
        s->last_deform = rt_deform_stats{};
        s->last_vis = rt_visibility_stats{};
        if (stats) stats->total_ms = ms_since(t0);
        return RT_OK;
    }
    try {
        CommitPlan P(s, t0);
        COMMIT_TRY(commit_reserve(s, P));
        // 1 - 3 check before anything changes; from 4 on the scene is written: the deformations on the
        // device (4 - 6), then the transforms and visibility on the host and on every replica (7 - 9)
        int k = 0;
        CommitClock::time_point t1;
        for (auto step : {commit_validate_positions, commit_moved_bounds, commit_range_check, commit_deform_triangles,
                          commit_refit_blas, commit_rebound_deformed, commit_apply_visibility, commit_host_refit,
                          commit_upload_and_refit}) {
            COMMIT_TRY(injected(++k));
            if (k == 4) wrote = true;
            if (k == 7) t1 = CommitClock::now();
            COMMIT_TRY(step(s, P));
        }
        drop_tile_orders(s);
        s->last_deform = P.dst;
        s->last_vis = P.vst;
        const double refit_ms = ms_since(t1);
        // a walk must never use a tree that lacks a visible pair: the commit that shows an instance
        // the tree does not hold rebuilds it on its own; until a rebuild succeeds the walks take tw_walk
        DynScene& Y = s->host.dyn;
        bool complete = true;
        for (size_t i = 0; i < Y.visible.size() && has_fit_tree(s->host); ++i) complete = complete && (!Y.visible[i] || Y.in_tree[i]);
        Y.fit_incomplete = !complete;
        // on request the flattened instance tree again, from the pose just committed
        if (rebuild || !complete) {
            COMMIT_TRY(injected(10));
            COMMIT_TRY(rebuild_fit(s, clustered));
            s->last_vis.forced_rebuild = (!rebuild && s->last_rebuild.rebuilt) ? 1 : 0;
        } else {
            s->last_rebuild = rt_rebuild_stats{};
            s->last_detail = rt_rebuild_detail{};
        }
        if (stats) {
            stats->instances_moved = (int64_t)P.staged.size();
            stats->bounds_ms = P.bounds_ms;
            stats->refit_ms = refit_ms;
            stats->total_ms = ms_since(t0);
        }
        return RT_OK;
    } catch (const std::bad_alloc&) {
        return fail(RT_ERR_OOM, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(RT_ERR_INVALID_ARG, e.what());
    }
}

int32_t rt_scene_commit(rt_scene* s, rt_commit_stats* stats) { return commit_impl(s, 0u, stats); }
int32_t rt_scene_commit_ex(rt_scene* s, uint32_t flags, rt_commit_stats* stats) { return commit_impl(s, flags, stats); }
