"""CPU tests of mesh simplification (no GPU): the numpy reference keeps the promises of include/ts_simplify.h on the fixtures of DESIGN.md
16i, libts_simplify.so is a library of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_simplify as ref
import ref_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_simplify.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsq_cluster_labels", "tsq_last_error", "tsq_place", "tsq_unique_faces", "tsq_workspace_bytes"]
SPHERE_ORIGIN = (-0.3, -0.3, -0.3)
SPHERE_CELLS = {1.7: (493, 993), 2.0: (375, 746), 3.0: (184, 366), 4.5: (72, 140)}  # cell -> (vertices, faces) out: the cell assignment alone
CUBE_ORIGIN = (-0.11, -0.07, -0.05)


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_simplify", ("diff_triangle_rasterization_2D", "_abi.py"))


SIMPLIFY_SIGNATURES = _abi_module().SIMPLIFY_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def simplify_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_simplify.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_simplify.so"
    return path


@pytest.fixture(scope="module")
def lib(simplify_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_simplify(ctypes.CDLL(simplify_path))


@pytest.fixture(scope="module")
def sphere():
    v, f = ref.sphere_mesh()
    assert v.shape == (4834, 3) and f.shape == (9664, 3) and v.dtype == np.float32
    topo = ref_volume.topology(f)
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0
    return v, f


def _header_prototypes():
    """name -> number of parameters of every tsq_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the reference holds the contract's promises -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", sorted(SPHERE_CELLS))
def test_sphere_stays_closed_and_quadric_keeps_more_volume_than_mean(sphere, cell):
    v, f = sphere
    analytic = 4.0 / 3.0 * np.pi * 9.3 ** 3
    err = {}
    for mode in ("quadric", "mean"):
        s = ref.simplify(v, f, cell, SPHERE_ORIGIN, mode)
        assert (s["num_vertices"], len(s["faces"])) == SPHERE_CELLS[cell]
        topo = ref_volume.topology(s["faces"])
        assert topo["boundary"] == 0  # no boundary edge at any cell size
        assert s["duplicates"] == (5 if cell == 1.7 else 0)
        if cell == 1.7:
            assert topo["nonmanifold"] > 0  # pinched cells: what stays open
        assert len(s["faces"]) == int(s["keep_remap"].sum()) - s["duplicates"]
        err[mode] = abs(1.0 - ref.signed_volume(s["vertices"], s["faces"]) / analytic)
        print(f"cell {cell} {mode}: |1 - volume / analytic| = {err[mode]:.5f}, flaps {s['flaps']}, nonmanifold {topo['nonmanifold']}")
    assert err["quadric"] < err["mean"]


@pytest.mark.parametrize("cell", [1.3, 2.1])
def test_cube_keeps_its_volume_with_quadric_placement(cell):
    v, f = ref.cube_mesh()
    assert ref_volume.topology(f)["boundary"] == 0 and len(f) == 12 * 12 * 12
    side = np.float64(np.float32(7.61)) - np.float64(np.float32(0.37))
    err = {}
    for mode in ("quadric", "mean"):
        s = ref.simplify(v, f, cell, CUBE_ORIGIN, mode)
        topo = ref_volume.topology(s["faces"])
        assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["euler"] == 2  # closed
        err[mode] = abs(1.0 - ref.signed_volume(s["vertices"], s["faces"]) / side ** 3)
        if mode == "quadric":  # the corners and edges of the cube are where the planes meet: the solve finds them
            p = s["vertices"].astype(np.float64)
            plane = np.minimum(np.abs(p - np.float64(np.float32(0.37))), np.abs(p - np.float64(np.float32(7.61)))).min(1)
            print(f"cell {cell}: largest distance of an output vertex to its nearest face plane {plane.max():.2e}")
            assert plane.max() < 2e-3
    print(f"cell {cell}: volume error quadric {err['quadric']:.2e}, mean {err['mean']:.2e}")
    assert err["quadric"] * 10.0 <= err["mean"]


def test_tilted_plane_stays_a_plane():
    v, f, p0, n = ref.plane_grid()
    dev_in = np.abs((v.astype(np.float64) - p0) @ n).max()
    s = ref.simplify(v, f, 1.1, (-20.0, -20.0, -20.0), "quadric")
    assert 0 < s["num_vertices"] < len(v) // 4
    dev_out = np.abs((s["vertices"].astype(np.float64) - p0) @ n).max()
    bound = dev_in + ref.ulp32(np.abs(v).max())
    print(f"plane deviation in {dev_in:.3e}, out {dev_out:.3e}, bound {bound:.3e}")
    assert dev_out <= bound


def test_every_valid_cluster_stays_in_its_cell(sphere):
    v, f = sphere
    rng = np.random.default_rng(3)
    for cell, origin in ((1.7, SPHERE_ORIGIN), (0.37, (-1.0, 2.0, 0.5)), (4.5, SPHERE_ORIGIN)):
        for mode in ("quadric", "mean"):
            for lam in (1e-3, 0.0):  # lambda 0: the solve is as ill-conditioned as the data makes it, and the clamp still holds
                s = ref.simplify(v, f, cell, origin, mode, lam)
                c, valid = ref.cell_indices(v, origin, cell)
                head = np.full(s["num_vertices"], len(v))
                np.minimum.at(head, s["remap"], np.arange(len(v)))
                assert valid.all()
                cc = np.array([np.float64(np.float32(o)) for o in origin]) + np.float64(np.float32(cell)) * (c[head] + 0.5)
                out = s["vertices"].astype(np.float64)
                assert (np.abs(out - cc) <= 0.5 * np.float64(np.float32(cell)) + ref.ulp32(s["vertices"])).all()
    # an invalid vertex keeps its position bit for bit and is its own cluster
    w = v[:200].copy()
    w[7] = (np.nan, 1.0, 2.0)
    w[11] = (np.inf, 1.0, 2.0)
    w[13] = (-5.0, 1.0, 2.0)  # cell -1
    s = ref.simplify(w, f[(f < 200).all(1)], 1.7, SPHERE_ORIGIN)
    for i in (7, 11, 13):
        assert s["label"][i] == i and s["member_count"][s["remap"][i]] == 1
        assert s["vertices"][s["remap"][i]].tobytes() == w[i].tobytes()
    del rng


def test_labels_numbering_attributes_and_the_duplicate_sweep():
    v = np.array([[0.1, 0.1, 0.1], [2.5, 0.1, 0.1], [0.9, 0.9, 0.9], [2.1, 0.9, 0.2], [0.5, 0.5, 0.5], [0.1, 2.5, 0.1]], np.float32)
    label = ref.cluster_labels(v, (0, 0, 0), 1.0)
    assert label.tolist() == [0, 1, 0, 1, 0, 5]
    a = np.array([[1.0], [2.0], [3.0], [np.nan], [5.0], [7.0]], np.float32)
    mask = np.array([1, 1, 0, 0, 1, 0], np.uint8)
    out = ref.place(v, np.zeros((0, 3), np.int64), [0, 1, 0, 1, 0, 2], (0, 0, 0), 1.0, mode=ref.MEAN, attributes=a, attr_valid=mask)
    assert out["attributes"][:, 0].tolist() == [3.0, 2.0, 0.0] and out["valid"].tolist() == [1, 1, 0] and out["member_count"].tolist() == [3, 2, 1]
    assert np.array_equal(out["vertices"][0], np.array([0.5, 0.5, 0.5], np.float32))
    assert np.isnan(ref.place(v, np.zeros((0, 3), np.int64), [0, 1, 0, 1, 0, 2], (0, 0, 0), 1.0, attributes=a)["attributes"][1, 0])  # NaNs propagate
    faces = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 1, 2], [3, 4, 5], [0, 2, 1], [0, 0, 1], [0, 1, 9]])
    keep, dup, flaps = ref.unique_faces(6, faces, np.ones(8, bool))
    assert keep.tolist() == [True, False, True, False, True, False, False, False] and dup == 3 and flaps == 2
    keep, dup, flaps = ref.unique_faces(6, faces, np.array([0, 1, 0, 1, 1, 0, 1, 1], bool))
    assert keep.tolist() == [False, True, False, False, True, False, False, False] and dup == 1 and flaps == 0


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(simplify_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsq_last_error.restype = ctypes.c_char_p; "
            "l.tsq_workspace_bytes.restype = ctypes.c_size_t; print(l.tsq_workspace_bytes(100000, 200000) >= 12 * 4 * 200000, "
            "repr(l.tsq_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, simplify_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(simplify_path):
    out = subprocess.run(["nm", "-D", "--defined-only", simplify_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", simplify_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", simplify_path], capture_output=True, text=True).stdout
    assert "libts_simplify.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so", "libts_color.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc)_[a-z0-9_]+)\s*\(", text)
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("-ffp-contract=off", "cz << 42 | cy << 21 | cx", "ONE thread's work", "linear in", "never leaves its cell", "TSQ_PLACE_QUADRIC",
                 "no square root", "duplicates, flaps"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(SIMPLIFY_SIGNATURES)
    for name, arity in declared.items():
        assert len(SIMPLIFY_SIGNATURES[name][1]) == arity, name
    assert declared["tsq_place"] == 21 and declared["tsq_cluster_labels"] == 10 and declared["tsq_unique_faces"] == 9
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES,
              abi.COLOR_SIGNATURES, abi.SIMPLIFY_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert SIMPLIFY_SIGNATURES["tsq_place"][1][5:10] == [ctypes.c_float] * 5 and SIMPLIFY_SIGNATURES["tsq_place"][1][19] == ctypes.c_size_t
    assert SIMPLIFY_SIGNATURES["tsq_workspace_bytes"][0] == ctypes.c_size_t


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_simplify", ("build.py",))
    assert list(build.SIMPLIFY_SOURCES) == ["mesh_simplify.hip", "api_simplify.hip"]
    assert "-ffp-contract=off" in build.SIMPLIFY_SOURCES["mesh_simplify.hip"]
    assert build.simplify_units() == ["mesh_simplify", "api_simplify"] and build.SIMPLIFY_SHARED == ["radix_sort"]
    cmd = build.simplify_command("mesh_simplify", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.simplify_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_simplify", "api_simplify", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units(), build.color_units()):
        assert not {"mesh_simplify", "api_simplify"} & set(others)  # its own library only
    assert build.SIMPLIFY_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_simplify.so")
    for header in ("ts_simplify_launch.h", os.path.join("..", "..", "include", "ts_simplify.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.simplify_command("volume")


def test_built_objects_carry_the_flags(simplify_path):
    build = _load("ts2d_build_simplify2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_simplify.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_simplify.so" in open(build.SIMPLIFY_LIB + ".cmd").read()


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 1024, 1025, 4097, 100000, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsq_workspace_bytes(n, fixed), lib.tsq_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_v >= 6 * 4 * n and by_f >= 12 * 4 * n  # the labels' six columns; the placement's four columns over 3 F slots
            prev_v, prev_f = by_v, by_f
    assert lib.tsq_workspace_bytes(-5, -5) == lib.tsq_workspace_bytes(0, 0)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    Q = 0x2000
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsq_last_error()
        assert text and word.encode() in text, text

    def labels(V=10, vertices=P, o=(0.0, 0.0, 0.0), cell=1.0, label=P, ws=P, ws_bytes=big):
        return lib.tsq_cluster_labels(V, vertices, *o, cell, label, ws, ws_bytes, None)

    def place(V=10, F=20, vertices=P, faces=P, remap=P, o=(0.0, 0.0, 0.0), cell=1.0, lam=1e-3, mode=1, attrs=None, mask=None, C=0, out=P,
              out_attrs=None, out_valid=None, members=P, ws=P, ws_bytes=big):
        return lib.tsq_place(V, F, vertices, faces, remap, *o, cell, lam, mode, attrs, mask, C, out, out_attrs, out_valid, members, ws, ws_bytes, None)

    def unique(V=10, F=20, faces=P, keep_in=P, keep_out=Q, counts=P, ws=P, ws_bytes=big):
        return lib.tsq_unique_faces(V, F, faces, keep_in, keep_out, counts, ws, ws_bytes, None)

    for call in (labels, place, unique):
        refused(call(V=-1), ">= 0")
        refused(call(V=-(2 ** 31)), ">= 0")
    for call in (place, unique):
        refused(call(F=-1), ">= 0")
        refused(call(F=715827883), "exceeds", CAPACITY)
    for call in (labels, place):
        for bad in (0.0, -1.0, nan, inf, -inf):
            refused(call(cell=bad), "cell must be finite and > 0")
        for bad in (nan, inf, -inf):
            refused(call(o=(0.0, bad, 0.0)), "origin must be finite")
    for bad in (-1e-9, -1.0, nan, inf):
        refused(place(lam=bad), "lambda")
    for bad in (-1, 2, 7):
        refused(place(mode=bad), "mode")
    for bad in (0, -1, 9, 100):
        refused(place(attrs=P, C=bad, out_attrs=P, out_valid=P), "C must be 1 .. 8")
    refused(place(attrs=P, C=3, out_attrs=None, out_valid=P), "null")
    refused(place(attrs=P, C=3, out_attrs=P, out_valid=None), "null")
    for name in ("vertices", "remap", "out", "members"):
        refused(place(**{name: None}), "null")
    refused(place(faces=None), "faces is null")
    for name in ("vertices", "label"):
        refused(labels(**{name: None}), "null")
    for name in ("faces", "keep_in", "keep_out"):
        refused(unique(**{name: None}), "null")
    refused(unique(counts=None), "counts is null")
    refused(unique(keep_out=P), "alias")
    for call in (labels, place, unique):
        refused(call(ws=None), "workspace is null")
    need = lib.tsq_workspace_bytes(1000, 2000)
    refused(place(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsq_last_error()
    refused(unique(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    refused(labels(V=1000, ws_bytes=lib.tsq_workspace_bytes(1000, 0) - 1), "workspace too small")
    # the no-ops answer without touching anything either
    assert labels(V=0, vertices=None, label=None, ws=None, ws_bytes=0) == 0
    assert place(V=0, F=0, vertices=None, faces=None, remap=None, out=None, members=None, ws=None, ws_bytes=0) == 0


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, simplify_path):
    """Without libts_simplify.so, diff_recon_hip.mesh_simplify raises and names the build command; everything else still imports."""
    src = os.path.dirname(simplify_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or (name.endswith(".so") and name != "libts_simplify.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.fuse_mesh), callable(diff_recon_hip.fuse_colored_mesh))\n"
            "try:\n    diff_recon_hip.simplify_mesh\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_simplify\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_simplify.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_simplify.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature(simplify_path):
    import inspect

    import diff_recon_hip
    from diff_recon_hip import mesh_simplify, volume
    for name in ("SimplifiedMesh", "simplify_mesh", "drop_small_pieces", "cluster_labels", "place_clusters", "unique_faces"):
        assert getattr(diff_recon_hip, name) is getattr(mesh_simplify, name)
    assert diff_recon_hip.mesh_simplify is mesh_simplify
    assert list(inspect.signature(mesh_simplify.simplify_mesh).parameters) == [
        "vertices", "faces", "cell", "origin", "placement", "regularization", "vertex_attributes", "attribute_valid", "faces_color"]
    assert mesh_simplify.SimplifiedMesh._fields == ("vertices", "faces", "vertex_attributes", "attribute_valid", "faces_color", "vertex_map",
                                                    "face_keep", "stats")
    assert list(inspect.signature(mesh_simplify.drop_small_pieces).parameters) == ["vertices", "faces", "min_faces"]
    for fn in (volume.fuse_mesh, mesh_simplify.simplify_fused):  # optional keywords whose default changes nothing
        p = inspect.signature(fn).parameters
        assert p["simplify_cell"].default is None and p["min_piece_faces"].default == 0
    assert diff_recon_hip.simplify_fused is mesh_simplify.simplify_fused
    assert mesh_simplify.simplify_fused("the mesh", None) == "the mesh"  # without either keyword nothing is touched
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_simplify.cluster_labels(torch.zeros((4, 3)), (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="cell"):
        mesh_simplify.cluster_labels(torch.zeros((4, 3)), (0, 0, 0), 0.0)
    with pytest.raises(ValueError, match="placement"):
        mesh_simplify.place_clusters(torch.zeros((4, 3)), torch.zeros((0, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32), (0, 0, 0), 1.0,
                                     placement="median")


def test_example_refuses_simplify_mesh_without_extract_mesh():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--simplify-mesh", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--simplify-mesh simplifies the mesh of --extract-mesh" in r.stderr
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--min-piece", "10"], capture_output=True, text=True)
    assert r.returncode == 2 and "--min-piece filters the mesh of --extract-mesh" in r.stderr
