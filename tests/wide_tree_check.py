"""Structural verifier of the four-wide trees (wide.h), in numpy, for tests/test_wide_build.py and
tests/test_gpu_refit_edges.py.  A helper module, not a conftest.

Input: the read-back of rt_debug_wide_build / rt_debug_wide_read (myraytracer_amd.engine.wide_build,
RayTracerEngine.wide_read) and the Python Scene the tree was built or committed for.  Every check is
exact - float comparisons with ==, no tolerance anywhere - against an FP64 restatement written from
the documented rules (wide.h, layout.h W4Node, scene.cpp build_fit / aabb_transformed, refit.h); none
of the product's code is used.  numpy does not fuse multiply-adds and the product is built with
-ffp-contract=off, so an expression written here term by term in the product's operation order gives
the product's bits.  (+0 and -0 compare equal, as they do in every box test of the walks.)

What is checked, per tree (the identity tree; the TLAS part and every BLAS part of a transformed
scene; the flattened instance tree), on octant copy 0:
  reach     every node of the tree's range is reached from the root exactly once; an empty slot has
            +inf in all six rows; 3 * depth + slack fits kStackCap as the builders state
  terminal  a leaf-run slot is down/up of lbox[run], and lbox[run] the min/max over the run's
            triangles' vertices (the scene's own arrays through tri_prim); a marker slot is down/up
            of its instance's tbox, tbox the min/max over the world bounds of the instances of its
            TLAS leaf, the world bounds the union of AABB.transformed over the mesh's triangles; a
            pair slot is down/up of the eight corners of lbox[pair.t0] through l2w[pair.inst]
  pairs     every (instance, leaf run) is exactly one pair and every pair exactly one slot
  inner     an inner slot equals the float union of its child node's non-empty slots ("equal"), or
            contains it ("contain")
  octant    per node and copy 1..7: the multiset of (ref, box) is copy 0's with the rows swapped by
            the octant's bits; empties last; pad zero
  order     the sort keys of wide_octant_copies, recomputed in FP64 from the floats, do not decrease
            across a node's slots (the order among equal keys is free)
  scalar    wide_coord, fit_coord and fit_blocked bound what wide.h says they bound

verify() returns a Report; Report.problems is a list of (kind, message)."""
import numpy as np

import myraytracer_amd as M

K_STACK_CAP = 128          # layout.h kStackCap
K_FIT_KAPPA = 4096.0       # scene.cpp kFitKappa
INF32 = np.float32(np.inf)


class Report:
    def __init__(self):
        self.problems = []
        self.trees = {}          # name -> dict(levels=[sizes, root first], depth, nodes, terminals)

    def bad(self, kind, msg):
        if len(self.problems) < 200:
            self.problems.append((kind, msg))

    def kinds(self):
        return sorted({k for k, _ in self.problems})

    def ok(self):
        return not self.problems


# ------------------------------------------------------------------ restated arithmetic
def f32_down(x):
    """The nearest float not above x (scene.cpp WideBuilder::down)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    bad = f.astype(np.float64) > x
    f[bad] = np.nextafter(f[bad], np.float32(-np.inf))
    return f


def f32_up(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    bad = f.astype(np.float64) < x
    f[bad] = np.nextafter(f[bad], np.float32(np.inf))
    return f


def aabb_transformed(lo, hi, m):
    """AABB.transformed(by:) (AABB.swift:71-92) in scene.cpp aabb_transformed's operation order.
    lo, hi: (n, 3); m: 16 values, column-major.  Returns (n, 3) lo and hi."""
    c = 0.5 * (lo + hi)
    e = 0.5 * (hi - lo)
    olo, ohi = np.empty_like(lo), np.empty_like(hi)
    for r in range(3):
        acc = m[0 + r] * c[:, 0]
        acc = m[4 + r] * c[:, 1] + acc
        acc = m[8 + r] * c[:, 2] + acc
        cn = acc + m[12 + r]
        en = abs(m[0 + r]) * e[:, 0] + abs(m[4 + r]) * e[:, 1] + abs(m[8 + r]) * e[:, 2]
        olo[:, r] = cn - en
        ohi[:, r] = cn + en
    return olo, ohi


def pair_boxes(lbox, m):
    """scene.cpp build_fit: the eight corners of each local box through l2w, min / max.
    lbox: (n, 6); m: (n, 16).  Returns (n, 3) lo, hi and the largest |local corner coordinate| (n)."""
    n = lbox.shape[0]
    lo = np.full((n, 3), np.inf)
    hi = np.full((n, 3), -np.inf)
    for q in range(8):
        p = [lbox[:, 3 + a] if (q >> a) & 1 else lbox[:, a] for a in range(3)]
        for a in range(3):
            v = m[:, a] * p[0] + m[:, 4 + a] * p[1] + m[:, 8 + a] * p[2] + m[:, 12 + a]
            lo[:, a] = np.minimum(lo[:, a], v)
            hi[:, a] = np.maximum(hi[:, a], v)
    lc = np.abs(lbox).max(axis=1) if n else np.zeros(0)
    return lo, hi, lc


def inf_norm3(m):
    """scene.cpp m3_inf_norm: the largest row sum of the 3x3 part (m: (..., 16) column-major)."""
    m = np.asarray(m, np.float64)
    rows = [np.abs(m[..., r]) + np.abs(m[..., 4 + r]) + np.abs(m[..., 8 + r]) for r in range(3)]
    return np.maximum(np.maximum(rows[0], rows[1]), rows[2])


# ------------------------------------------------------------------ the scene's own triangles
def scene_triangles(scene):
    """(T, 3, 3) vertices in the order of the reference's `triangles[]` (RTContext.swift:120-378:
    every sphere, plane, triangle and mesh object appends in object order), and per mesh id the
    (first, count) of its run."""
    out, runs = [], {}
    n = 0
    for oi, o in enumerate(scene.objects):
        if isinstance(o, (M.Sphere, M.Plane)):
            v = np.full((1, 3, 3), np.nan)
        elif isinstance(o, M.Triangle):
            v = np.asarray(o.vertices, np.float64).reshape(1, 3, 3)
            runs[("triangle", oi)] = (n, 1)                     # a triangle object is a mesh of one
        elif isinstance(o, M.Mesh):
            assert o.ply_path is None, "the verifier reads inline meshes"
            pos = np.asarray(o.positions, np.float64).reshape(-1, 3)
            idx = np.asarray(o.indices, np.int64).reshape(-1)
            idx = idx[: 3 * (idx.size // 3)].reshape(-1, 3) - (1 if o.indices_one_based else 0)
            v = pos[idx]
            runs[o.id] = (n, len(v))
        else:
            continue
        out.append(v)
        n += len(v)
    return (np.concatenate(out) if out else np.zeros((0, 3, 3))), runs


def scene_instances(scene, runs):
    """The multiset of (first triangle of the mesh, transform) the scene's mesh objects and mesh
    instances produce (RTContext.swift:384-410)."""
    by_id = {}
    for o in scene.objects:
        if isinstance(o, M.Mesh):
            if runs[o.id][1] > 0:
                by_id[o.id] = runs[o.id]
            else:
                by_id.pop(o.id, None)
    out = []
    for o in scene.objects:
        if isinstance(o, M.MeshInstance) and o.base_mesh_id in by_id:
            out.append((by_id[o.base_mesh_id][0], tuple(float(x) for x in o.transform)))
            by_id[o.id] = by_id[o.base_mesh_id]
    taken = {o.id for o in scene.objects if isinstance(o, M.MeshInstance)}
    for o in scene.objects:
        if isinstance(o, M.Mesh) and o.id in by_id and o.id not in taken:
            out.append((runs[o.id][0], tuple(float(x) for x in o.transform)))
    for oi, o in enumerate(scene.objects):
        if isinstance(o, M.Triangle):
            out.append((runs[("triangle", oi)][0], tuple(float(x) for x in o.transform)))
    return out


# ------------------------------------------------------------------ the read-back
def split_nodes(nodes):
    """(N, 32) uint32 raw records -> near (N, 3, 4) f32, ref (N, 4) i32, far (N, 3, 4) f32, pad (N, 4)."""
    nodes = np.ascontiguousarray(nodes, np.uint32)
    n = nodes.shape[0]
    near = nodes[:, 0:12].copy().view(np.float32).reshape(n, 3, 4)
    ref = nodes[:, 12:16].copy().view(np.int32)
    far = nodes[:, 16:28].copy().view(np.float32).reshape(n, 3, 4)
    pad = nodes[:, 28:32].copy()
    return near, ref, far, pad


def leaf_runs(tri_last):
    """First TriRec of every leaf run -> its length."""
    last = np.flatnonzero(np.asarray(tri_last) != 0)
    first = np.concatenate([[0], last[:-1] + 1]) if len(last) else np.zeros(0, np.int64)
    return {int(a): int(b - a + 1) for a, b in zip(first, last)}


class _Tree:
    """One tree of octant copy 0 walked from its root."""

    def __init__(self, rep, name, near, far, ref, root, lo, hi):
        self.name = name
        n_all = near.shape[0]
        seen = np.zeros(n_all, bool)
        self.levels = []
        self.ok = True
        cur = np.array([root], np.int64)
        if not (lo <= root < hi):
            rep.bad("reach", f"{name}: root {root} outside [{lo}, {hi})")
            self.ok = False
            cur = cur[:0]
        while len(cur):
            seen[cur] = True
            self.levels.append(cur)
            full = near[cur, 0, :] < INF32
            r = ref[cur]
            ch = r[full & (r >= 0)].astype(np.int64)
            out = (ch < lo) | (ch >= hi)
            if out.any():
                rep.bad("reach", f"{name}: child node {int(ch[out][0])} outside [{lo}, {hi})")
                self.ok = False
                ch = ch[~out]
            dup = seen[ch]
            u, cnt = np.unique(ch, return_counts=True)
            if dup.any() or (cnt > 1).any():
                rep.bad("reach", f"{name}: a node is reached more than once")
                self.ok = False
                ch = u[~seen[u]]
            if len(self.levels) > 64:
                rep.bad("reach", f"{name}: deeper than 64 levels")
                self.ok = False
                break
            cur = ch
        self.nodes = np.concatenate(self.levels) if self.levels else np.zeros(0, np.int64)
        self.depth = len(self.levels)
        missing = np.setdiff1d(np.arange(lo, hi), self.nodes)
        if len(missing) and lo < hi:
            rep.bad("reach", f"{name}: {len(missing)} nodes of [{lo}, {hi}) are not reached (first {int(missing[0])})")
        rep.trees[name] = dict(levels=[len(l) for l in self.levels], depth=self.depth, nodes=self.nodes)


def tlas_leaves(scene):
    """Per instance the TLAS leaf that holds it, from the oracle's TLAS of `scene` (tests/test_bvh.py
    shows it equal to the product's).  A refit keeps the topology of the BUILD: after commits pass
    the leaves of the scene as it was built."""
    import oracle
    osc = oracle.OracleScene(scene)
    out = osc.tlas_leaves()
    osc.close()
    return out


def verify(dump, scene, inner=None, after_refit=False, leaf_of=None):
    """dump: the dict of engine.wide_build / RayTracerEngine.wide_read.  leaf_of: tlas_leaves() of
    the scene as built (default: of `scene`, right for a build).  inner: per tree kind
    ("identity", "tlas", "blas", "fit") "equal" or "contain" (default: "equal", "contain" for the
    identity tree, whose TLAS-leaf slots carry the TLAS leaf's own box).  after_refit: every inner
    slot of the TLAS part and of the fit tree must equal the union (refit.h), whatever `inner`."""
    rep = Report()
    mode = {"identity": "contain", "tlas": "equal", "blas": "equal", "fit": "equal"}
    mode.update(inner or {})
    if after_refit:
        mode["tlas"] = mode["fit"] = "equal"
    d = dump
    if d["wide_root"] < 0:
        rep.bad("reach", "no four-wide tree")
        return rep
    N = int(d["wide_copy"])
    near8, ref8, far8, pad8 = split_nodes(d["nodes"])
    if near8.shape[0] != 8 * N:
        rep.bad("reach", "the node array does not hold eight copies")
        return rep
    near, ref, far = near8[:N], ref8[:N], far8[:N]
    full = near[:, 0, :] < INF32                                   # (N, 4)
    tris, mesh_runs = scene_triangles(scene)
    tri_prim = np.asarray(d["tri_prim"], np.int64)
    lbox = np.asarray(d["lbox"], np.float64)
    runs = leaf_runs(d["tri_last"])
    ni = int(d["instances"])
    l2w = np.asarray(d["l2w"], np.float64).reshape(ni, 16)
    base, mbase = int(d["tlas_leaf_base"]), int(d["marker_base"])
    fit_root, fit_nodes = int(d["fit_root"]), int(d["fit_nodes"])
    n_main = N - (fit_nodes if fit_root >= 0 else 0)

    # ---- empty slots / finite boxes
    rows = np.concatenate([near, far], axis=1)                     # (N, 6, 4)
    emp = ~full
    if not np.all(np.where(emp[:, None, :], rows == INF32, True)):
        rep.bad("reach", "an empty slot has a row that is not +inf")
    fin = np.where(full[:, None, :], np.isfinite(rows), True)
    if not fin.all() or np.any(full & np.any(near > far, axis=1)):
        rep.bad("terminal", "a slot box is not finite or has near > far in copy 0")

    # ---- lbox of every run: min / max over the run's triangles' vertices
    r_first = np.array(sorted(runs), np.int64)
    if len(r_first):
        if tri_prim.min() < 0 or tri_prim.max() >= len(tris):
            rep.bad("terminal", "tri_prim outside the scene's triangles")
            return rep
        v = tris[tri_prim]                                         # (n, 3, 3) local vertices per TriRec
        tlo, thi = v.min(axis=1), v.max(axis=1)
        rid = np.cumsum(np.concatenate([[0], np.asarray(d["tri_last"][:-1]) != 0])).astype(np.int64)
        rlo = np.full((len(r_first), 3), np.inf)
        rhi = np.full((len(r_first), 3), -np.inf)
        np.minimum.at(rlo, rid, tlo)
        np.maximum.at(rhi, rid, thi)
        want = np.concatenate([rlo, rhi], axis=1)
        got = lbox[r_first]
        if not np.array_equal(got, want):
            b = np.flatnonzero((got != want).any(axis=1))
            rep.bad("terminal", f"lbox of {len(b)} leaf runs is not the min/max of their triangles (first run {int(r_first[b[0]])})")

    # ---- trees
    reached_runs = []

    def check_tree(kind, name, root, lo, hi, slack):
        t = _Tree(rep, name, near, far, ref, root, lo, hi)
        if 3 * t.depth + slack > K_STACK_CAP:
            rep.bad("reach", f"{name}: depth {t.depth} exceeds the stack bound")
        nd = t.nodes
        if not len(nd):
            return t, np.zeros(0, np.int64)
        f = full[nd]
        r = ref[nd]
        term = f & (r < 0)
        e = (~r[term]).astype(np.int64)                            # terminal ids
        tn, ts = np.nonzero(term)
        got_lo = near[nd[tn], :, ts]                               # (k, 3)
        got_hi = far[nd[tn], :, ts]
        if kind in ("identity", "blas"):
            okr = np.isin(e, r_first) & (e < base)
            if not okr.all():
                rep.bad("terminal", f"{name}: a terminal slot is not the start of a leaf run")
            e2 = e[okr]
            w_lo, w_hi = f32_down(lbox[e2, :3]), f32_up(lbox[e2, 3:])
            neq = (got_lo[okr] != w_lo).any(axis=1) | (got_hi[okr] != w_hi).any(axis=1)
            if neq.any():
                rep.bad("terminal", f"{name}: {int(neq.sum())} leaf-run slots are not down/up of lbox (first run {int(e2[neq][0])})")
            reached_runs.append(e2)
        elif kind == "tlas":
            k = e - mbase
            okm = (k >= 0) & (k < ni)
            if not okm.all():
                rep.bad("terminal", f"{name}: a terminal slot of the TLAS part is no instance marker")
            k = k[okm]
            u, c = np.unique(k, return_counts=True)
            if len(u) != ni or (c != 1).any():
                rep.bad("pairs", f"{name}: {ni} instances but markers of {len(u)}, largest multiplicity {int(c.max()) if len(c) else 0}")
            tb = np.asarray(d["tbox"], np.float64)[k]
            neq = (got_lo[okm] != f32_down(tb[:, :3])).any(axis=1) | (got_hi[okm] != f32_up(tb[:, 3:])).any(axis=1)
            if neq.any():
                rep.bad("terminal", f"{name}: {int(neq.sum())} marker slots are not down/up of tbox (first instance {int(k[neq][0])})")
        else:                                                      # fit: pairs
            np_ = int(d["pairs"])
            okp = e < np_
            if not okp.all():
                rep.bad("pairs", f"{name}: a slot names pair {int(e[~okp][0])} of {np_}")
            u, c = np.unique(e[okp], return_counts=True)
            if len(u) != np_ or (c != 1).any():
                rep.bad("pairs", f"{name}: {np_} pairs, {len(u)} of them in slots")
            fp = np.asarray(d["fpairs"], np.int64).reshape(-1, 2)[e[okp]]
            plo, phi, _ = pair_boxes(lbox[fp[:, 0]], l2w[fp[:, 1]])
            neq = (got_lo[okp] != f32_down(plo)).any(axis=1) | (got_hi[okp] != f32_up(phi)).any(axis=1)
            if neq.any():
                rep.bad("terminal", f"{name}: {int(neq.sum())} pair slots are not down/up of the pair's box (first pair {int(e[okp][neq][0])})")
        # inner slots against the union of their child node's slots
        inn = f & (r >= 0)
        pn, ps = np.nonzero(inn)
        ch = r[inn].astype(np.int64)
        chf = full[ch]                                             # (k, 4)
        u_lo = np.where(chf[:, None, :], near[ch], INF32).min(axis=2)
        u_hi = np.where(chf[:, None, :], far[ch], -INF32).max(axis=2)
        b_lo, b_hi = near[nd[pn], :, ps], far[nd[pn], :, ps]
        if mode[kind] == "equal":
            badi = (b_lo != u_lo).any(axis=1) | (b_hi != u_hi).any(axis=1)
        else:
            badi = (b_lo > u_lo).any(axis=1) | (b_hi < u_hi).any(axis=1)
        if badi.any():
            rep.bad("inner", f"{name}: {int(badi.sum())} inner slots do not {mode[kind]} the union of their child's slots "
                             f"(first node {int(nd[pn][badi][0])} slot {int(ps[badi][0])})")
        rep.trees[name]["terminals"] = e
        return t, e

    world_boxes = []          # FP64 boxes wide_coord must cover
    if d["identity"]:
        check_tree("identity", "identity", int(d["wide_root"]), 0, n_main, 2)
        world_boxes.append(lbox[r_first])
    else:
        nt = int(d["tw_tlas_nodes"])
        tl, _ = check_tree("tlas", "tlas", int(d["wide_root"]), 0, nt, 0)
        wroot = np.asarray(d["wroot"], np.int64)
        roots = sorted({int(x) for x in wroot if x >= 0})
        # every BLAS part: its nodes are a contiguous preorder range starting at its root
        bounds = roots + [n_main]
        bdepth = 0
        inst_runs = {}
        for i, rt in enumerate(roots):
            if not (nt <= rt < n_main):
                rep.bad("reach", f"BLAS root {rt} outside the BLAS part")
                continue
            t, e = check_tree("blas", f"blas@{rt}", rt, rt, bounds[i + 1], 0)
            bdepth = max(bdepth, t.depth)
            inst_runs[rt] = e
        if roots and roots[0] != nt:
            rep.bad("reach", "nodes between the TLAS part and the first BLAS part")
        for x in {int(x) for x in wroot if x < 0}:
            if ~x not in runs:
                rep.bad("terminal", f"wroot {x} is not a leaf run")
            inst_runs[x] = np.array([~x], np.int64)
            reached_runs.append(inst_runs[x])
            bdepth = max(bdepth, 0)
        if 3 * (tl.depth + bdepth) + 4 > K_STACK_CAP:
            rep.bad("reach", "TLAS + BLAS depth exceeds the stack bound")
        # ---- instances: transforms, world bounds, tbox, bcoord
        blas_prims = {w: np.unique(np.concatenate([tri_prim[a:a + runs[int(a)]] for a in rr if int(a) in runs] or
                                                  [np.zeros(0, np.int64)])) for w, rr in inst_runs.items()}
        starts = np.array([int(blas_prims[int(w)].min()) if len(blas_prims.get(int(w), ())) else -1 for w in wroot])
        mesh_of = {s: c for s, c in mesh_runs.values()}
        got = sorted((int(starts[k]), tuple(l2w[k])) for k in range(ni))
        want = sorted(scene_instances(scene, mesh_runs))
        if got != want:
            rep.bad("terminal", "the instances' (mesh, l2w) differ from the scene's objects")
        ib = np.asarray(d["inst_bounds"], np.float64).reshape(ni, 6)
        for k in range(ni):
            s = int(starts[k])
            if s not in mesh_of:
                rep.bad("terminal", f"instance {k}: its triangles start at {s}, which begins no mesh")
                continue
            if not np.array_equal(blas_prims[int(wroot[k])], np.arange(s, s + mesh_of[s])):
                rep.bad("terminal", f"instance {k}: its leaf runs do not hold exactly its mesh's triangles")
            v = tris[s:s + mesh_of[s]]
            olo, ohi = aabb_transformed(v.min(axis=1), v.max(axis=1), l2w[k])
            wb = np.concatenate([olo.min(axis=0), ohi.max(axis=0)])
            if not np.array_equal(ib[k], wb):
                rep.bad("terminal", f"instance {k}: world bounds differ from the union of its triangles' transformed boxes")
            rr = inst_runs[int(wroot[k])]
            bc = np.abs(lbox[rr]).max() if len(rr) else 0.0
            if not d["bcoord"][k] >= bc:
                rep.bad("scalar", f"instance {k}: bcoord {d['bcoord'][k]} below its largest local coordinate {bc}")
        # tbox: the min / max of the world bounds over the instances of the instance's TLAS leaf
        # (membership: the oracle's TLAS of the scene as built)
        tb = np.asarray(d["tbox"], np.float64).reshape(ni, 6)
        lf = np.asarray(tlas_leaves(scene) if leaf_of is None else leaf_of)
        if len(lf) != ni or (lf < 0).any():
            rep.bad("terminal", f"the oracle's TLAS holds {len(lf)} instances, the read-back {ni}")
        else:
            for leaf in np.unique(lf):
                ks = np.flatnonzero(lf == leaf)
                u = np.concatenate([ib[ks, :3].min(axis=0), ib[ks, 3:].max(axis=0)])
                badk = ks[(tb[ks] != u).any(axis=1)]
                if len(badk):
                    rep.bad("terminal", f"tbox of instances {badk[:4].tolist()} is not the union of the world bounds "
                                        f"of their TLAS leaf {ks[:6].tolist()}")
        world_boxes.append(tb)
        # ---- the flattened instance tree
        if fit_root >= 0:
            check_tree("fit", "fit", fit_root, fit_root, fit_root + fit_nodes, 2)
            if fit_root != n_main:
                rep.bad("reach", "the fit tree does not follow the BLAS parts")
            fp = np.asarray(d["fpairs"], np.int64).reshape(-1, 2)
            have = sorted((int(b), int(a)) for a, b in fp)
            want = sorted((k, int(a)) for k in range(ni) for a in inst_runs.get(int(wroot[k]), []))
            if have != want:
                miss = len(set(want) - set(have))
                rep.bad("pairs", f"the pairs are not the (instance, leaf run) set: {miss} missing, {len(have)} held, {len(want)} expected")
            plo, phi, lc = pair_boxes(lbox[fp[:, 0]], l2w[fp[:, 1]])
            nl = inf_norm3(l2w)
            need = max(float(np.abs(l2w[:, 12:15]).max()), float((nl[fp[:, 1]] * lc).max()),
                       float(np.abs(plo).max()), float(np.abs(phi).max()))
            if not d["fit_coord"] >= need:
                rep.bad("scalar", f"fit_coord {d['fit_coord']} below {need}")
        # kappa = |l2w|_inf |w2l|_inf (the inverse of the 3x3 part; the cases tested lie far from 2^12)
        lin = l2w.reshape(ni, 4, 4)[:, :3, :3].transpose(0, 2, 1)
        kap = inf_norm3(l2w) * np.abs(np.linalg.inv(lin)).sum(axis=2).max(axis=1)
        over = bool((kap > K_FIT_KAPPA).any())
        if fit_root >= 0 and bool(d["fit_blocked"]) != over and after_refit:
            rep.bad("scalar", f"fit_blocked is {d['fit_blocked']} with the largest kappa {kap.max()}")
        if fit_root >= 0 and not d["fit_blocked"] and over:
            rep.bad("scalar", f"a fit tree in use with kappa {kap.max()} above 2^12")
    # every leaf run is one terminal slot of exactly one tree
    rr = np.concatenate(reached_runs) if reached_runs else np.zeros(0, np.int64)
    if sorted(rr.tolist()) != sorted(runs):
        rep.bad("pairs", f"{len(runs)} leaf runs, {len(rr)} terminal slots ({len(set(rr.tolist()))} distinct)")
    wb = np.concatenate(world_boxes) if world_boxes else np.zeros((0, 6))
    if len(wb) and not d["wide_coord"] >= np.abs(wb).max():
        rep.bad("scalar", f"wide_coord {d['wide_coord']} below a world box coordinate {np.abs(wb).max()}")
    # ... and every slot box of the world-space trees (the identity tree; the TLAS part): a row is an FP64
    # coordinate of magnitude <= wide_coord rounded outward, or a min / max of such rows
    wn = slice(0, n_main if d["identity"] else int(d["tw_tlas_nodes"]))
    wrows = rows[wn][np.broadcast_to(full[wn][:, None, :], rows[wn].shape)]
    wc = np.array([d["wide_coord"]])
    if len(wrows) and (wrows.min() < f32_down(-wc)[0] or wrows.max() > f32_up(wc)[0]):
        rep.bad("scalar", f"wide_coord {d['wide_coord']} below a world-space slot row ({wrows.min()}, {wrows.max()})")

    # ---- octant copies
    if np.any(pad8 != 0):
        rep.bad("octant", "a pad word is not zero")
    canon0 = None
    for o in range(8):
        nr, fr, rf = near8[o * N:(o + 1) * N], far8[o * N:(o + 1) * N], ref8[o * N:(o + 1) * N]
        neg = [(o >> a) & 1 for a in range(3)]
        lo = np.stack([fr[:, a, :] if neg[a] else nr[:, a, :] for a in range(3)], axis=1).astype(np.float64)
        hi = np.stack([nr[:, a, :] if neg[a] else fr[:, a, :] for a in range(3)], axis=1).astype(np.float64)
        fl = nr[:, 0, :] < INF32
        lo, hi = np.where(fl[:, None, :], lo, 0.0), np.where(fl[:, None, :], hi, 0.0)
        if np.any(fl[:, 1:] & ~fl[:, :-1]):
            rep.bad("octant", f"copy {o}: an empty slot precedes a full one")
        key = np.zeros(fl.shape)
        for a in range(3):
            key = key + (-0.5 if neg[a] else 0.5) * (lo[:, a, :] + hi[:, a, :])
        key = np.where(fl, key, np.inf)
        dec = key[:, 1:] < key[:, :-1]
        if dec.any():
            rep.bad("order", f"copy {o}: the sort keys decrease in {int(dec.any(axis=1).sum())} nodes (first node {int(np.flatnonzero(dec.any(axis=1))[0])})")
        rec = np.concatenate([rf[:, None, :].astype(np.float64), lo, hi], axis=1)        # (N, 7, 4)
        rec = np.where(fl[:, None, :], rec, np.inf).transpose(0, 2, 1).reshape(-1, 7)   # (N * 4, 7)
        node = np.repeat(np.arange(N), 4)
        order = np.lexsort(tuple(rec[:, c] for c in range(6, -1, -1)) + (node,))
        canon = rec[order]
        if o == 0:
            canon0 = canon
        elif not np.array_equal(canon, canon0):
            b = np.flatnonzero((canon != canon0).any(axis=1)) // 4
            rep.bad("octant", f"copy {o}: {len(np.unique(b))} nodes differ from copy 0 as multisets of (ref, box) (first node {int(b[0])})")
    return rep


def assert_ok(dump, scene, **kw):
    rep = verify(dump, scene, **kw)
    assert rep.ok(), rep.problems[:8]
    return rep


def node_multisets(dump, lo, hi):
    """Per node of [lo, hi) of copy 0: its non-empty slots as a sorted (ref, box) array - what a
    build and a refit at one pose must agree on (the slot order among equal keys is free)."""
    N = int(dump["wide_copy"])
    near, ref, far, _ = split_nodes(dump["nodes"][:N])
    fl = near[:, 0, :] < INF32
    rec = np.concatenate([ref[:, None, :].astype(np.float64), near.astype(np.float64), far.astype(np.float64)], axis=1)
    rec = np.where(fl[:, None, :], rec, np.inf).transpose(0, 2, 1)[lo:hi].reshape(-1, 7)
    node = np.repeat(np.arange(hi - lo), 4)
    return rec[np.lexsort(tuple(rec[:, c] for c in range(6, -1, -1)) + (node,))]


def same_dump(a, b):
    """Byte equality of two read-backs (scalars and arrays)."""
    for k in a:
        if isinstance(a[k], np.ndarray):
            if a[k].dtype.kind == "f":
                if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)):
                    return k
            elif not np.array_equal(a[k], b[k]):
                return k
        elif a[k] != b[k]:
            return k
    return None
