"""CPU tests of the mesh-distance feature (no GPU): the numpy reference holds its own promises, libts_geom.so is a library of its own with
exactly the C ABI of include/ts_geom.h, every argument check answers before any HIP call, and RawTriangle's host-side set operations."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_distance as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_geom.h")
INVALID = 1  # TS2D_ERR_INVALID


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built (the package itself needs libts2d.so)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ts2d_abi_geom", os.path.join(ROOT, "triangle-splatting_amd", "diff_triangle_rasterization_2D", "_abi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEOM_SIGNATURES = _abi_module().GEOM_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def geom_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_geom.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_geom.so"
    return path


@pytest.fixture(scope="module")
def lib(geom_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_geom(ctypes.CDLL(geom_path))


def _header_prototypes():
    """name -> number of parameters of every tsg_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the reference by itself -----------------------------------------------------------------------------------------------------------------
def test_reference_search_agrees_with_a_kd_tree_and_keeps_its_rules():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    q, r = rng.random((700, 3), dtype=np.float32), rng.random((900, 3), dtype=np.float32)
    idx, d2 = ref.nearest(q, r)
    dist, _ = cKDTree(r.astype(np.float64)).query(q.astype(np.float64))
    assert np.allclose(np.sqrt(d2.astype(np.float64)), dist, rtol=1e-5, atol=1e-7)
    exact = ((q.astype(np.float64) - r[idx].astype(np.float64)) ** 2).sum(axis=1)
    assert np.allclose(d2, exact, rtol=1e-5)
    r2 = np.concatenate([r[:5], r[:5]])  # duplicates: the smallest index wins
    idx, d2 = ref.nearest(r[:5], r2)
    assert idx.tolist() == [0, 1, 2, 3, 4] and (d2 == 0).all()
    r3 = r[:4].copy()
    r3[0, 1] = np.nan
    r3[2, 0] = np.inf
    idx, _ = ref.nearest(q[:50], r3)
    assert set(idx.tolist()) <= {1, 3}
    idx, d2 = ref.nearest(np.array([[0, np.nan, 0], [0, 0, 0]], np.float32), r3)
    assert idx[0] == -1 and np.isnan(d2[0]) and idx[1] in (1, 3)
    idx, d2 = ref.nearest(q[:3], np.full((2, 3), np.nan, np.float32))
    assert (idx == -1).all() and np.isinf(d2).all()
    idx, d2 = ref.nearest(q[:3], np.zeros((0, 3), np.float32))
    assert (idx == -1).all() and np.isinf(d2).all()
    big = np.array([[3e38, 3e38, 3e38], [-3e38, 3e38, 0]], np.float32)  # every distance overflows: the smallest index still wins
    idx, d2 = ref.nearest(np.array([[-3e38, -3e38, -3e38]], np.float32), big)
    assert idx[0] == 0 and np.isinf(d2[0])


def test_reference_sampler_is_stratified_and_monotone():
    v, f = ref.heavy_tailed_soup(5000, seed=3)
    area = ref.face_areas(v, f)
    N = 20000
    points, face = ref.sample(v, f, area, N, seed=11)
    assert (np.diff(face) >= 0).all() and face.min() >= 0 and face.max() < 5000
    w, C = ref.weights(area)
    expected = N * w.astype(np.float64) / float(C[-1])
    count = np.bincount(face, minlength=5000)
    assert np.abs(count - expected).max() < 2
    assert (count[w == 0] == 0).all()
    assert ref.barycentric_excess(v, f, points, face) < 1e-5  # every point lies in its face
    again, face2 = ref.sample(v, f, area, N, seed=11)
    assert np.array_equal(again.view(np.uint32), points.view(np.uint32)) and np.array_equal(face, face2)
    other, _ = ref.sample(v, f, area, N, seed=12)
    assert not np.array_equal(other, points)


def test_reference_known_answer_two_parallel_squares():
    h = 0.5
    a, b = ref.two_squares(h)
    res = ref.mesh_distance(a, b, 2000, seed=0, thresholds=[h / 2, 2 * h])
    print(res["accuracy"] / h - 1, res["completeness"] / h - 1)
    assert h <= res["accuracy"] <= h * (1 + 1e-3) and h <= res["completeness"] <= h * (1 + 1e-3)
    assert res["precision"] == [0.0, 1.0] and res["recall"] == [0.0, 1.0] and res["fscore"] == [0.0, 1.0]
    assert res["area_a"] == 1.0 and res["area_b"] == 1.0 and res["a_dropped"] == res["b_dropped"] == 0
    assert res["chamfer"] == (res["accuracy"] + res["completeness"]) / 2


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(geom_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsg_last_error.restype = ctypes.c_char_p; l.tsg_sample_workspace_bytes.restype = ctypes.c_size_t; "
            "print(l.tsg_sample_workspace_bytes(1000) >= 8000, repr(l.tsg_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, geom_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(geom_path):
    out = subprocess.run(["nm", "-D", "--defined-only", geom_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    declared = _header_prototypes()
    assert len(declared) == 6
    assert ours == sorted(declared)
    everything = subprocess.run(["nm", "-D", geom_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    soname = subprocess.run(["readelf", "-d", geom_path], capture_output=True, text=True).stdout
    assert "libts_geom.so" in soname and "libts2d.so" not in soname


def test_library_registers_the_radix_sort_and_none_of_the_rasterizer_binning_kernels(geom_path):
    names = open(geom_path, "rb").read()  # the kernel names the library registers with the runtime are strings of the file
    assert b"rs_scatter_kernel" in names
    for kernel in (b"scan_emit_kernel", b"tile_ranges_kernel", b"gather_blocksum_kernel", b"depth_order_small_kernel", b"depth_bucket_sort_kernel",
                   b"depth_split_"):
        assert kernel not in names, kernel


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(GEOM_SIGNATURES)
    for name, arity in declared.items():
        assert len(GEOM_SIGNATURES[name][1]) == arity, name
    assert not set(GEOM_SIGNATURES) & set(_abi_module().SIGNATURES)


def test_build_tables_name_the_units_and_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ts2d_build_geom", os.path.join(ROOT, "triangle-splatting_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert list(build.GEOM_SOURCES) == ["mesh_distance.hip", "api_geom.hip"]
    assert "-ffp-contract=off" in build.GEOM_SOURCES["mesh_distance.hip"]
    cmd = build.geom_command("mesh_distance", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.geom_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_distance", "api_geom", "radix_sort")]
    assert not {os.path.join(build.OBJ_DIR, n + ".o") for n in ("depth_order", "emit")} & set(build.geom_objects())  # the rasterizer's own binning units
    assert "mesh_distance" not in build.units() and "api_geom" not in build.units()  # libts2d.so links neither
    stamp = open(os.path.join(build.OBJ_DIR, "mesh_distance.o.cmd")).read()  # what the object on disk was compiled with
    assert "-ffp-contract=off" in stamp


def test_workspace_queries_are_monotone(lib):
    sizes = [0, 1, 2, 1023, 1024, 1025, 65_537, 1_000_000, 2_499_999, 2_500_000, 2_500_001, 2_510_000, 2_560_000, 2_600_000, 5_000_000,
             100_000_000, 2 ** 31 - 1025]
    prev = -1
    for n in sizes:
        b = lib.tsg_sample_workspace_bytes(n)
        assert b >= 8 * n and b >= prev
        prev = b
    for fixed in (0, 1000, 3_000_000):
        prev_q = prev_r = -1
        for n in sizes:
            bq, br = lib.tsg_cross_workspace_bytes(n, fixed), lib.tsg_cross_workspace_bytes(fixed, n)
            assert bq >= 32 * n and bq >= prev_q and br >= 32 * n and br >= prev_r, (n, fixed)
            prev_q, prev_r = bq, br


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word):
        assert rc == INVALID, rc
        text = lib.tsg_last_error()
        assert text and word.encode() in text, text

    refused(lib.tsg_nearest_cross(-1, P, 1, P, P, P, None, P, big, None), "Q")
    refused(lib.tsg_nearest_cross(1, P, -1, P, P, P, None, P, big, None), "R")
    refused(lib.tsg_nearest_cross(2 ** 31 - 1, P, 1, P, P, P, None, P, big, None), "at most")
    refused(lib.tsg_nearest_cross(1, None, 1, P, P, P, None, P, big, None), "null")
    refused(lib.tsg_nearest_cross(1, P, 1, None, P, P, None, P, big, None), "null")
    refused(lib.tsg_nearest_cross(1, P, 1, P, None, P, None, P, big, None), "null")
    refused(lib.tsg_nearest_cross(1, P, 1, P, P, None, None, P, big, None), "null")
    refused(lib.tsg_nearest_cross(1, P, 1, P, P, P, None, None, big, None), "null")
    refused(lib.tsg_nearest_cross(1000, P, 1000, P, P, P, None, P, lib.tsg_cross_workspace_bytes(1000, 1000) - 1, None), "too small")
    assert lib.tsg_nearest_cross(0, None, 5, None, None, None, None, None, 0, None) == 0  # Q == 0: a no-op

    refused(lib.tsg_face_areas(-1, 1, P, P, None, P, None), "V")
    refused(lib.tsg_face_areas(1, -1, P, P, None, P, None), "F")
    refused(lib.tsg_face_areas(3, 1, None, P, None, P, None), "null")
    refused(lib.tsg_face_areas(3, 1, P, None, None, P, None), "null")
    refused(lib.tsg_face_areas(3, 1, P, P, None, None, None), "null")
    assert lib.tsg_face_areas(3, 0, None, None, None, None, None) == 0

    refused(lib.tsg_sample_surface(-1, 1, P, P, P, 1, 0, P, P, P, big, None), "V")
    refused(lib.tsg_sample_surface(3, -1, P, P, P, 1, 0, P, P, P, big, None), "F")
    refused(lib.tsg_sample_surface(3, 1, P, P, P, -1, 0, P, P, P, big, None), "N")
    refused(lib.tsg_sample_surface(3, 1, None, P, P, 1, 0, P, P, P, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1, P, None, P, 1, 0, P, P, P, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1, P, P, None, 1, 0, P, P, P, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1, P, P, P, 1, 0, None, P, P, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1, P, P, P, 1, 0, P, None, P, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1, P, P, P, 1, 0, P, P, None, big, None), "null")
    refused(lib.tsg_sample_surface(3, 1000, P, P, P, 1, 0, P, P, P, lib.tsg_sample_workspace_bytes(1000) - 1, None), "too small")
    assert lib.tsg_sample_surface(3, 1, None, None, None, 0, 0, None, None, None, 0, None) == 0  # N == 0: a no-op


def test_missing_library_fails_loudly(tmp_path, hip_lib_built):
    """diff_recon_hip.mesh_distance does not degrade when libts_geom.so is absent: the import raises and names the build command."""
    import shutil
    src = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip")
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    shutil.copy(os.path.join(src, "mesh_distance.py"), pkg / "mesh_distance.py")
    (pkg / "__init__.py").write_text("")
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    r = subprocess.run([sys.executable, "-c", "import diff_recon_hip.mesh_distance"], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "libts_geom.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


# ---- RawTriangle, the operations that need no device ----------------------------------------------------------------------------------------
def _raw(n, offset=0.0):
    from diff_recon_hip import RawTriangle
    vertex = (np.arange(n * 9, dtype=np.float32).reshape(n, 3, 3) + np.float32(offset))
    return RawTriangle(vertex, np.arange(n, dtype=np.float32).reshape(n, 1) + np.float32(offset), np.full((n, 3), offset, np.float32) + np.arange(n, dtype=np.float32)[:, None])


def test_raw_triangle_host_side_set_operations(hip_lib_built, capsys):
    from diff_recon_hip import RawTriangle
    a, b = _raw(4), _raw(2, offset=100.0)
    assert a.contained_idx.dtype == np.bool_ and a.contained_idx.tolist() == [True] * 4
    assert np.array_equal(a.center, a.vertex.mean(axis=1)) and a.center.shape == (4, 3)
    assert len(RawTriangle()) == 0 and RawTriangle().contained_idx.shape == (0,)

    same = a
    a += RawTriangle()  # an empty other: untouched
    assert a is same and len(a) == 4
    b.contained_idx[1] = False
    a += b
    assert a is same and len(a) == 6 and a.contained_idx.tolist() == [True] * 5 + [False]
    assert np.array_equal(a.vertex[4:], b.vertex) and np.array_equal(a.opacity[4:], b.opacity) and np.array_equal(a.shs[4:], b.shs)
    empty = RawTriangle()
    empty += b  # None arrays take the other's
    assert len(empty) == 2 and np.array_equal(empty.vertex, b.vertex)

    a.contained_idx[1] = False
    removed = a.reduce()
    assert len(removed) == 2 and removed.opacity.reshape(-1).tolist() == [1.0, 101.0]
    assert len(a) == 4 and a.opacity.reshape(-1).tolist() == [0.0, 2.0, 3.0, 100.0] and a.contained_idx.tolist() == [True] * 4
    nothing = a.reduce()  # nothing marked: an empty RawTriangle, self untouched
    assert isinstance(nothing, RawTriangle) and len(nothing) == 0 and len(a) == 4

    a.contained_idx[:] = False
    a.resetContainedIdx()
    assert a.contained_idx.tolist() == [True] * 4

    a.replace([0, 3], _raw(2, offset=500.0))
    assert a.opacity.reshape(-1).tolist() == [500.0, 2.0, 3.0, 501.0] and a.vertex[3, 0, 0] == 509.0 and a.shs[0, 0] == 500.0
    with pytest.raises(ValueError, match="length of removed_triangle is 3, length of other is 2"):
        a.replace([0, 1, 2], _raw(2))

    same = a
    a -= RawTriangle()  # an empty other: no search, no device
    assert a is same and len(a) == 4
    assert (a - RawTriangle()) is not a

    a.printStats()
    out = capsys.readouterr().out
    assert "RawTriangle Stats" in out and "Number of points: 4" in out and "z median" in out
