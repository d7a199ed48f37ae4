"""The face table of ray queries (rt_debug_query_tables, a host-only build): per triangle record,
in leaf order, the triangle's index in its own object's face list, and per instance the object it
came from.  In every scene, per object, the faces its records name are exactly range(ntri), once
each, and a record's v0, e1, e2 are that face's vertices as the scene gave them, bit for bit
(e1 = v1 - v0 in FP64).  Identity scenes matter most: there TriRec::prim holds the owning instance
and the face index survives only in this table.  No GPU."""
import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes

import deform_scenes as DS


def _object_faces(obj):
    """(F, 3, 3) vertices of an object's faces in the order the scene gives them; None: no faces."""
    if isinstance(obj, M.Mesh):
        if obj.ply_path is not None:
            m = M.ply_load(obj.ply_path)
            pos, idx = m["positions"], np.asarray(m["indices"], np.int64).reshape(-1, 3)
        else:
            pos = np.asarray(obj.positions, np.float64)
            idx = np.asarray(obj.indices, np.int64).reshape(-1, 3) - (1 if obj.indices_one_based else 0)
        return pos[idx]
    if isinstance(obj, M.Triangle):
        return np.asarray(obj.vertices, np.float64).reshape(1, 3, 3)
    return None


def _check(sc, flags=0):
    tab = M.engine.query_tables(sc, flags)
    face, owner, verts = tab["face"], tab["tri_object"], tab["verts"].reshape(-1, 3, 3)
    assert len(face) == len(owner) == len(verts) > 0
    seen = 0
    for oi, obj in enumerate(sc.objects):
        mine = np.flatnonzero(owner == oi)
        tris = _object_faces(obj)
        if tris is None:                                   # a sphere or a plane: one record, no face;
            if not isinstance(obj, M.MeshInstance):        # a MeshInstance: no geometry of its own
                assert len(mine) == 1 and face[mine[0]] == -1, oi
                seen += 1
            else:
                assert len(mine) == 0
            continue
        assert np.array_equal(np.sort(face[mine]), np.arange(len(tris))), f"object {oi}: faces named != range(ntri)"
        f = tris[face[mine]]
        want = np.stack([f[:, 0], f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]], axis=1)
        assert np.array_equal(verts[mine].view(np.uint64), want.view(np.uint64)), f"object {oi}: v0, e1, e2 differ"
        seen += len(mine)
    assert seen == len(face)
    return tab


def _instance_objects(sc, tab):
    """Every instance names the object it came from; a mesh's own instance and its MeshInstances."""
    io = tab["inst_object"]
    kinds = [type(sc.objects[o]).__name__ for o in io if o >= 0]
    return io, kinds


def test_c2_identity_scene():
    sc = scenes.scaled(scenes.scene_c2(inline=True), 8, 8)
    tab = _check(sc)
    assert list(tab["inst_object"]) == [0]
    # leaf order is not face order: the table is not the identity permutation
    assert not np.array_equal(tab["face"], np.arange(len(tab["face"])))


def _three_meshes():
    hp, hf = scenes.heightfield(9, 4.0, 0.5, 3)
    objs = []
    for k, n in enumerate((7, 64, 131)):
        objs.append(M.Mesh(id=10 + k, material="1", positions=hp + np.array([6.0 * k, 0.0, 0.0]),
                           indices=hf[k:k + n].astype(np.int32) + (1 if k == 1 else 0), indices_one_based=(k == 1),
                           shading_mode="flat"))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = objs
    return sc


def test_three_meshes_identity_and_with_a_mesh_instance():
    sc = _three_meshes()
    tab = _check(sc)
    assert sorted(tab["inst_object"]) == [0, 1, 2]
    sc.objects.insert(1, M.MeshInstance(id=77, base_mesh_id=11, material="1", transform=M.translation(0.0, 3.0, 0.0)))
    tab = _check(sc)
    io, kinds = _instance_objects(sc, tab)
    assert sorted(io) == [0, 1, 2, 3] and kinds.count("MeshInstance") == 1
    # a MeshInstance that takes over its base mesh's id: the base has no instance of its own
    sc.objects[1] = M.MeshInstance(id=11, base_mesh_id=11, material="1", transform=M.translation(0.0, 3.0, 0.0))
    tab = _check(sc)
    assert sorted(tab["inst_object"]) == [-1, 0, 1, 3]


def test_ply_with_quads(tmp_path):
    """Faces in the order rt_ply_load returns them (quads fan-triangulated by the loader)."""
    n = 5
    g = np.arange(n + 1, dtype=np.float64)
    X, Z = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([X, 0.25 * np.sin(X + 2 * Z), Z], -1).reshape(-1, 3).astype(np.float32)
    lines = ["ply", "format ascii 1.0", f"element vertex {len(pos)}", "property float x", "property float y",
             "property float z", f"element face {n * n + 1}", "property list uchar int vertex_indices", "end_header"]
    lines += [" ".join(repr(float(x)) for x in p) for p in pos]
    for i in range(n):
        for j in range(n):
            a = i * (n + 1) + j
            lines.append(f"4 {a} {a + 1} {a + n + 2} {a + n + 1}")
    lines.append("3 0 1 7")
    path = str(tmp_path / "quads.ply")
    open(path, "w").write("\n".join(lines) + "\n")
    assert len(M.ply_load(path)["indices"]) == 2 * n * n + 1
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [M.Mesh(id=1, material="1", ply_path=path, shading_mode="smooth")]
    _check(sc)


def test_triangle_objects_and_special_primitives():
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [M.Triangle(vertices=((-3, -1, -3), (3, -1, -3), (0, 2, -3.5)), material="1"),
                  M.Triangle(vertices=((0.1, 0.2, 0.3), (1.5, 0.25, 0.125), (0.7, 1.9, -0.3)), material="1")]
    tab = _check(sc)
    assert list(tab["face"]) == [0, 0] and sorted(tab["inst_object"]) == [0, 1]
    sc.objects = [M.Sphere(center=(-2.5, 0.3, 0.5), radius=0.7, material="1"),
                  M.Plane(center=(0.0, -1.5, 0.0), normal=(0.0, 1.0, 0.0), material="1")]
    tab = _check(sc)
    assert list(tab["face"]) == [-1, -1] and sorted(tab["inst_object"]) == [0, 1]


def test_mixed_transformed_scene():
    _check(DS.base_scene("special", sizes=(1, 3, 65, 257)))


@pytest.mark.parametrize("flags", [A.RT_SCENE_DYNAMIC, A.RT_SCENE_DEFORMABLE])
def test_dynamic_and_deformable_builds(flags):
    sc = DS.base_scene("smooth", sizes=(2, 64, 255))
    a, b = _check(sc, flags), _check(sc, 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    import ctypes as C
    io, pk = A.rt_query_tables(), sc.to_desc()
    assert M.load_library().rt_debug_query_tables(pk.ptr, 4, C.byref(io)) == A.RT_ERR_INVALID_ARG
