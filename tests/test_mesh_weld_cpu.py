"""CPU tests of vertex welding (include/ts_weld.h, diff_recon_hip/mesh_weld.py): the numpy reference tests/ref_mesh_weld.py against hand-written
answers, the argument checks of the C ABI (decided before any HIP call, so they run without a device), and RawTriangle.saveGLB: process=True
refuses to run without a device, process=False writes the bytes it always wrote."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import ref_mesh_weld as ref

OK, INVALID = 0, 1  # TS2D_OK, TS2D_ERR_INVALID (include/ts2d.h)


# ---- the reference against known answers ----------------------------------------------------------------------------------------------------
def test_reference_chain_is_one_cluster_and_breaks_at_a_wide_gap():
    eps = 0.5
    x = np.array([0.0, 0.375, 0.75, 1.125, 1.5, 2.25, 2.625], np.float32)  # steps of 0.75 eps, one step of 1.5 eps between 4 and 5
    v = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    assert ref.labels(v, eps).tolist() == [0, 0, 0, 0, 0, 5, 5]
    perm = np.array([3, 6, 0, 5, 2, 4, 1])  # vertex k of the permuted array is vertex perm[k]: clusters {3, 0, 2, 4, 1} and {6, 5}
    assert ref.labels(v[perm], eps).tolist() == [0, 1, 0, 1, 0, 0, 0]
    w = ref.weld(v, [[0, 1, 5], [0, 5, 6], [2, 5, 9], [-1, 0, 5]], eps, "mean")
    assert w["remap"].tolist() == [0, 0, 0, 0, 0, 1, 1] and w["num_vertices"] == 2 and w["largest_cluster"] == 5
    assert w["faces"].tolist() == [[0, 0, 1], [0, 1, 1], [-1, -1, -1], [-1, -1, -1]] and w["keep"].tolist() == [False] * 4
    assert w["vertices"].tolist() == [[0.75, 0.0, 0.0], [2.4375, 0.0, 0.0]]
    assert ref.compact(w["label"], v, "first")[1].tolist() == [[0.0, 0.0, 0.0], [2.25, 0.0, 0.0]]


def test_reference_threshold_zero_and_non_finite():
    a = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [np.nextafter(np.float32(0.5), np.float32(1)), 0.0, 0.0]], np.float32)
    assert ref.labels(a, 0.25).tolist() == [0, 0, 2]  # d2 == eps^2 merges; 0.25 + one ulp does not
    z = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [0.0, 1.0, 2.0000002], [np.nan, 1.0, 2.0], [np.nan, 1.0, 2.0], [np.inf, 0, 0], [np.inf, 0, 0]], np.float32)
    assert ref.labels(z, 0.0).tolist() == [0, 0, 2, 3, 4, 5, 6]
    assert ref.labels(z, 3e38).tolist() == [0, 0, 0, 3, 4, 5, 6]  # eps * eps = inf in fp32: every finite pair passes, no other


def test_reference_triangle_fan():
    n = 6  # a closed fan: centre 0, rim 1 .. 6
    faces = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    t = ref.topology(7, faces)
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["euler"]) == (12, 6, 6, 0, 1, 1)
    t = ref.topology(7, faces, keep=[True] * 5 + [False])  # an open fan
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["euler"]) == (11, 7, 4, 0, 1, 1)
    t = ref.topology(8, faces + [[0, 1, 7], [3, 3, 9], [-1, 0, 1]])  # a third face on the edge (0, 1); two faces that name no vertex
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["faces"]) == (14, 8, 5, 1, 1, 7)


def test_reference_two_disjoint_quads():
    faces = [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]]
    t = ref.topology(9, faces)  # vertex 8 is named by no face
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["vertices_referenced"], t["euler"]) == (10, 8, 2, 0, 2, 8, 2)
    assert t["label"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8]
    assert ref.same_partition([0, 0, 2, 2], [5, 5, 1, 1]) and not ref.same_partition([0, 0, 2, 2], [0, 1, 2, 2])


def test_reference_jittered_grid_counts():
    eps = 1e-3
    v, f, grid_id = ref.grid_soup(20, eps, seed=1)
    assert v.shape == (2166, 3) and f.shape == (722, 3)
    w = ref.weld(v, f, eps)
    assert w["num_vertices"] == 400 and w["keep"].all() and ref.same_partition(w["label"], grid_id)
    t = ref.topology(400, w["faces"])
    assert (t["edges"], t["boundary"], t["manifold"], t["nonmanifold"], t["pieces"], t["euler"]) == (1121, 76, 1045, 0, 1, 1)


# ---- the C ABI's argument checks, without a device --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(hip_lib_built):
    from diff_triangle_rasterization_2D import _abi  # the one table of signatures, on a CDLL of this module's own
    return _abi.bind(ctypes.CDLL(hip_lib_built))


X = 0x1000  # stands for a non-null device pointer: every call below is refused (or is a no-op) before anything is dereferenced or enqueued
BIG = 1 << 40


def _refused(lib, rc, *words):
    text = lib.ts2d_last_error()
    return rc == INVALID and text and all(w in text for w in words)


def test_negative_counts_and_bad_eps_are_invalid(lib):
    assert _refused(lib, lib.ts2d_weld_labels(-1, X, 0.1, X, X, BIG, None), b"V")
    assert _refused(lib, lib.ts2d_weld_compact(-1, X, X, 0, X, X, X, X, BIG, None), b"V")
    assert _refused(lib, lib.ts2d_weld_face_components(-1, 1, X, None, X, None, 0, None), b"V")
    assert _refused(lib, lib.ts2d_weld_face_components(1, -1, X, None, X, None, 0, None), b"F")
    assert _refused(lib, lib.ts2d_weld_remap_faces(-1, 1, X, X, X, X, None), b"V")
    assert _refused(lib, lib.ts2d_weld_remap_faces(1, -1, X, X, X, X, None), b"F")
    assert _refused(lib, lib.ts2d_weld_edge_census(-1, 1, X, None, X, X, BIG, None), b"V")
    assert _refused(lib, lib.ts2d_weld_edge_census(1, -5, X, None, X, X, BIG, None), b"F")
    assert _refused(lib, lib.ts2d_weld_edge_census(1, 715827883, X, None, X, X, BIG, None), b"F")  # 3 F edge slots must fit 31 bits
    for eps in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert _refused(lib, lib.ts2d_weld_labels(4, X, eps, X, X, BIG, None), b"eps"), eps
        assert _refused(lib, lib.ts2d_weld_labels(0, X, eps, X, X, BIG, None), b"eps"), eps  # also where nothing would run
    assert _refused(lib, lib.ts2d_weld_compact(4, X, X, 2, X, X, X, X, BIG, None), b"mode")


def test_null_pointers_are_invalid(lib):
    for args in ((4, None, 0.1, X, X, BIG, None), (4, X, 0.1, None, X, BIG, None), (4, X, 0.1, X, None, BIG, None)):
        assert _refused(lib, lib.ts2d_weld_labels(*args), b"null"), args
    assert _refused(lib, lib.ts2d_weld_labels_counted(4, None, 0.1, X, None, X, BIG, None), b"null")
    assert _refused(lib, lib.ts2d_weld_face_components(4, 2, None, None, X, None, 0, None), b"null")
    assert _refused(lib, lib.ts2d_weld_face_components(4, 2, X, None, None, None, 0, None), b"null")
    for hole in range(7):  # label, vertices, remap, out_vertices, count, workspace
        if hole == 2:
            continue  # the mode
        args = [X, X, 0, X, X, X, X]
        args[hole] = None
        assert _refused(lib, lib.ts2d_weld_compact(4, *args, BIG, None), b"null"), hole
    for hole in range(4):
        args = [X, X, X, X]
        args[hole] = None
        assert _refused(lib, lib.ts2d_weld_remap_faces(4, 2, *args, None), b"null"), hole
    assert _refused(lib, lib.ts2d_weld_edge_census(4, 2, None, None, X, X, BIG, None), b"null")
    assert _refused(lib, lib.ts2d_weld_edge_census(4, 2, X, None, None, X, BIG, None), b"null")
    assert _refused(lib, lib.ts2d_weld_edge_census(4, 2, X, None, X, None, BIG, None), b"null")


def test_a_small_workspace_is_invalid(lib):
    need = lib.ts2d_weld_workspace_bytes(5000, 0)
    assert _refused(lib, lib.ts2d_weld_labels(5000, X, 0.1, X, X, need - 1, None), b"workspace")
    assert _refused(lib, lib.ts2d_weld_compact(5000, X, X, 1, X, X, X, X, need - 1, None), b"workspace")
    need = lib.ts2d_weld_workspace_bytes(5000, 3000)
    assert _refused(lib, lib.ts2d_weld_edge_census(5000, 3000, X, None, X, X, need - 1, None), b"workspace")


def test_empty_input_is_a_no_op(lib):
    assert lib.ts2d_weld_labels(0, None, 0.0, None, None, 0, None) == OK
    assert lib.ts2d_weld_labels_counted(0, None, 1.0, None, None, None, 0, None) == OK
    assert lib.ts2d_weld_face_components(0, 0, None, None, None, None, 0, None) == OK
    assert lib.ts2d_weld_face_components(0, 5, None, None, None, None, 0, None) == OK
    assert lib.ts2d_weld_compact(0, None, None, 0, None, None, None, None, 0, None) == OK
    assert lib.ts2d_weld_remap_faces(7, 0, None, None, None, None, None) == OK
    assert lib.ts2d_weld_remap_faces(0, 0, None, None, None, None, None) == OK
    assert lib.ts2d_weld_edge_census(7, 0, None, None, None, None, 0, None) == OK


def test_workspace_bytes_are_monotonic(lib):
    sizes = (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 2500, 65_537, 1_000_000, 3_000_000, 3_000_001, 50_000_000)
    for fixed in (0, 1, 1000, 1_000_000):
        by_v = [lib.ts2d_weld_workspace_bytes(n, fixed) for n in sizes]
        by_f = [lib.ts2d_weld_workspace_bytes(fixed, n) for n in sizes]
        assert by_v == sorted(by_v) and by_f == sorted(by_f), fixed
    assert lib.ts2d_weld_workspace_bytes(0, 0) < 1 << 16
    assert lib.ts2d_weld_workspace_bytes(3_000_000, 0) >= 3_000_000 * 32  # codes, ids and the gathered float4 points
    assert lib.ts2d_weld_workspace_bytes(0, 1_000_000) >= 3_000_000 * 16  # two ping-pong pairs of edge words


# ---- Python surface ------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes(hip_lib_built):
    import diff_recon_hip as D
    from diff_recon_hip import mesh_weld
    assert D.weld_mesh is mesh_weld.weld_mesh and D.mesh_topology is mesh_weld.mesh_topology and D.WeldedMesh is mesh_weld.WeldedMesh
    v, f = torch.zeros(6, 3), torch.arange(6, dtype=torch.int32).reshape(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.weld_mesh(v, f, eps=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.mesh_topology(6, f)
    with pytest.raises(RuntimeError, match=r"vertices must have dimensions \(num_vertices, 3\)"):
        D.weld_mesh(torch.zeros(6, 2), f)
    with pytest.raises(RuntimeError, match=r"faces must be an int32 or int64 tensor with dimensions \(num_faces, 3\)"):
        D.weld_mesh(v, f.to(torch.float32))
    with pytest.raises(ValueError, match="position"):
        D.weld_mesh(v, f, position="median")
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps must be finite"):
            D.weld_mesh(v, f, eps=eps)


def _model():
    from diff_recon_hip.raw_triangle import RawTriangle
    P, K = 37, 4  # no random numbers: the file below is pinned by its hash
    vertex = ((np.arange(P * 9, dtype=np.float32) * 37 % 101) / 8 - 6).reshape(P, 3, 3)
    opacity = ((np.arange(P, dtype=np.float32) * 13 % 29) / 4 - 3).reshape(P, 1)
    shs = ((np.arange(P * 3 * K, dtype=np.float32) * 7 % 23) / 8 - 1.25).reshape(P, 3 * K)
    return RawTriangle(vertex, opacity, shs)


# sha256 of what saveGLB(process=False) wrote for _model() before process=True existed
PINNED = {True: "4064a55d5fb77446df653c88a8544571ebd47a96464fae0e917741b2ec3ae17e", False: "03722fb2484eb0769fb91bf13529145dfd877bdbe1be645882405880b67c45f4"}


def test_save_glb_without_process_writes_the_bytes_it_always_wrote(tmp_path, hip_lib_built):
    import sys
    m = _model()
    before = {}
    for back in (True, False):
        m.saveGLB(str(tmp_path / f"a{back}.glb"), save_back=back)
        before[back] = open(tmp_path / f"a{back}.glb", "rb").read()
    from diff_recon_hip import mesh_weld  # noqa: F401  (bound by now at the latest)
    assert "diff_recon_hip.mesh_weld" in sys.modules
    for back in (True, False):
        m.saveGLB(str(tmp_path / f"b{back}.glb"), save_back=back, process=False, weld_eps=0.5)  # weld_eps is ignored without process
        after = open(tmp_path / f"b{back}.glb", "rb").read()
        assert after == before[back] and hashlib.sha256(after).hexdigest() == PINNED[back], back


def test_save_glb_with_process_needs_a_device(tmp_path, monkeypatch, hip_lib_built):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = _model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.saveGLB(str(tmp_path / "w.glb"), process=True, weld_eps=0.1)
    assert not (tmp_path / "w.glb").exists()
    from diff_recon_hip.raw_triangle import RawTriangle
    z = np.zeros
    RawTriangle(z((0, 3, 3), np.float32), z((0, 1), np.float32), z((0, 3), np.float32)).saveGLB(str(tmp_path / "e.glb"), process=True)  # empty: returns first
    assert not (tmp_path / "e.glb").exists()


def test_the_render_pose_of_the_gpu_test_is_mostly_unambiguous():
    """The GPU test renders the welded posed grid and compares it on the pixels the float64 checker does not call ambiguous: at most 5 % may be."""
    import ref_mesh_f64
    import synthetic
    v, f, grid_id = ref.posed_grid()
    w = ref.weld(v, f, ref.GRID_EPS)
    assert w["num_vertices"] == 400 and w["keep"].all() and ref.same_partition(w["label"], grid_id)
    cam = synthetic.camera(ref.RENDER_W, ref.RENDER_H)
    want = ref_mesh_f64.render(w["vertices"], w["faces"], ref.face_colors(722), ref.RENDER_W, ref.RENDER_H, cam["tanfovx"], cam["tanfovy"], cam["viewmatrix"])
    share = want["ambiguous"].mean()
    print(f"ambiguous share {share:.4f}, covered {want['mask'].mean():.3f}, faces seen {len(np.unique(want['face_idx'])) - 1}")
    assert share <= ref_mesh_f64.MAX_AMBIGUOUS_SHARE and want["mask"].mean() > 0.5 and len(np.unique(want["face_idx"])) > 300
