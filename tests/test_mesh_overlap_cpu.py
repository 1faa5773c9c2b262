"""CPU tests of the triangle-overlap query (no GPU): the numpy reference on constructions with small integer coordinates, where every
determinant is exact and the geometric answer is known; libts_overlap.so is a library of its own with exactly the C ABI of the header;
every argument check answers before any HIP call; the Python wrappers check their arguments and the package re-exports the feature."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_overlap as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_overlap.h")
INVALID = 1  # TS2D_ERR_INVALID
NAMES = ["tsx_last_error", "tsx_overlap", "tsx_sort_pairs", "tsx_sort_workspace_bytes"]


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_overlap", ("diff_triangle_rasterization_2D", "_abi.py"))


OVERLAP_SIGNATURES = _abi_module().OVERLAP_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def overlap_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_overlap.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_overlap.so"
    return path


@pytest.fixture(scope="module")
def lib(overlap_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_overlap(ctypes.CDLL(overlap_path))


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the reference on exact constructions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.constructions()))
def test_reference_gives_the_known_answer_on_exact_constructions(name):
    v, f, want_kind, want_stats = ref.constructions()[name]
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 8  # small integers: every product and sum below is exact in float64
    got = ref.overlap(v, f)
    assert ref.kind_of(v, f, 0, 1) == want_kind, (name, got)
    for key, value in want_stats.items():
        assert got["stats"][key] == value, (name, key, got["stats"])
    want_count = [1, 1] if want_kind == ref.KIND_CROSSING else [0, 0]
    assert got["count_a"].tolist() == want_count and got["count_b"] is None
    assert len(got["pairs"]) == (1 if want_kind else 0) == got["stats"]["stored"]
    # the answer does not depend on which face comes first, nor on a rotation of either face's corners
    swapped = ref.overlap(v, f[::-1])
    assert ref.kind_of(v, f[::-1], 0, 1) == want_kind and swapped["count_a"].tolist() == want_count
    for ra in range(3):
        for rb in range(3):
            g = np.stack([np.roll(f[0], ra), np.roll(f[1], rb)])
            assert ref.kind_of(v, g, 0, 1) == want_kind, (name, ra, rb)


def test_reference_constructions_in_cross_mode():
    """Cross mode compares no indices: the pairs that were decided by coordinates keep their kind, the index-decided ones change."""
    cons = ref.constructions()
    for name in ("piercing", "parallel", "vertex_rests_inside", "edges_cross_in_a_point", "overlapping_in_one_plane"):
        v, f, want_kind, _ = cons[name]
        got = ref.overlap(v, f[:1], None, v, f[1:])
        assert got["kind"].tolist() == ([want_kind] if want_kind else []), name
        assert got["count_a"].tolist() == got["count_b"].tolist() == [int(want_kind == 1)]
        back = ref.overlap(v, f[1:], None, v, f[:1])
        assert back["kind"].tolist() == got["kind"].tolist(), name
    v, f, _, _ = cons["same_indices_other_order"]
    assert ref.overlap(v, f[:1], None, v, f[1:])["kind"].tolist() == [ref.KIND_COPLANAR]   # a face against itself: one plane
    v, f, _, _ = cons["edge_adjacent"]
    assert ref.overlap(v, f[:1], None, v, f[1:])["kind"].tolist() == [ref.KIND_CROSSING]   # the shared edge is a touch
    v, f, _, _ = cons["degenerate_face"]
    got = ref.overlap(v, f[:1], None, v, f[1:])                                            # (v, v, w) is eligible in ts_bvh.h's sense
    assert got["stats"]["degenerate"] == 0


@pytest.mark.parametrize("solid", ["tetrahedron", "cube", "octahedron"])
def test_reference_finds_nothing_on_closed_convex_solids(solid):
    v, f = getattr(ref, solid)()
    got = ref.overlap(v, f)
    assert len(got["pairs"]) == 0 and not got["count_a"].any(), got
    st = got["stats"]
    assert st["crossing"] == st["coplanar"] == st["duplicate"] == st["degenerate"] == 0
    assert st["adjacent"] == 3 * len(f) // 2  # one pair per edge of a closed manifold
    assert st["candidates"] >= st["adjacent"]


def test_reference_masks_ineligible_faces_and_generators_hold_every_kind():
    v, f = ref.soup(40, 1)
    keep = np.arange(40) % 4 == 0
    got, sub = ref.overlap(v, f, keep), ref.overlap(v, f[keep])
    idx = np.nonzero(keep)[0]
    assert np.array_equal(got["pairs"], idx[sub["pairs"]].astype(np.int32)) and np.array_equal(got["count_a"][keep], sub["count_a"])
    assert got["stats"]["degenerate"] == 30 and not got["count_a"][~keep].any()
    bad = v.copy()
    bad[f[3, 1]] = np.nan
    assert ref.overlap(bad, f)["stats"]["degenerate"] == 1
    assert ref.overlap(v, np.zeros((0, 3), np.int32))["stats"] == dict.fromkeys(ref.STATS_KEYS, 0)
    kinds = set()
    for gen in (ref.soup, ref.sheets):
        v, f = gen(521, 7)
        assert f.shape == (521, 3)
        kinds |= set(ref.overlap(v, f)["kind"].tolist())
    assert kinds == {1, 2, 3}


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(overlap_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsx_last_error.restype = ctypes.c_char_p; "
            "l.tsx_sort_workspace_bytes.restype = ctypes.c_size_t; print(l.tsx_sort_workspace_bytes(1000) >= 25000, repr(l.tsx_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, overlap_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(overlap_path):
    out = subprocess.run(["nm", "-D", "--defined-only", overlap_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", overlap_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", overlap_path], capture_output=True, text=True).stdout
    assert "libts_overlap.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_inside.so", "libts_winding.so"):
        assert other not in dynamic


def test_header_text_stays_out_of_the_other_libraries_lists():
    """tests/test_cabi_cpu.py collects the names of libts2d.so's entry points from every header by prefix, tso_ (ts_optim.h) among them: this
    library's prefix is tsx_, and no word of the header reads as a call of another library."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsi|tsw|tsn)_[a-z0-9_]+)\s*\(", text)
    full = open(HEADER).read()
    for word in ("-ffp-contract=off", "ts_bvh.h", "orient(a, b, c, d) = (b - a) . ((c - a) x (d - a))", "takes part", "closed", "ADJACENT", "DUPLICATE",
                 "COPLANAR", "CROSSING", "min(total, capacity)", "Purity", "equal to brute force"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(OVERLAP_SIGNATURES)
    for name, arity in declared.items():
        assert len(OVERLAP_SIGNATURES[name][1]) == arity, name
    assert declared["tsx_overlap"] == 15 and declared["tsx_sort_pairs"] == 8
    abi = _abi_module()
    for table in (abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.ATLAS_SIGNATURES,
                  abi.INSIDE_SIGNATURES, abi.ORIENT_SIGNATURES, abi.WINDING_SIGNATURES):
        assert not set(OVERLAP_SIGNATURES) & set(table)
    assert OVERLAP_SIGNATURES["tsx_overlap"][1][10] is ctypes.c_int32 and OVERLAP_SIGNATURES["tsx_overlap"][1][2] is ctypes.c_size_t


def test_build_tables_name_the_units_and_flags(overlap_path):
    build = _load("ts2d_build_overlap", ("build.py",))
    assert list(build.OVERLAP_SOURCES) == ["mesh_overlap.hip", "api_overlap.hip"] and build.OVERLAP_SHARED == ["radix_sort"]
    assert "-ffp-contract=off" in build.OVERLAP_SOURCES["mesh_overlap.hip"]
    assert build.overlap_units() == ["mesh_overlap", "api_overlap"]
    cmd = build.overlap_command("mesh_overlap", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.overlap_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_overlap", "api_overlap", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.inside_units(), build.winding_units()):
        assert not {"mesh_overlap", "api_overlap"} & set(others)  # its own library only
    assert build.OVERLAP_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_overlap.so")
    for header in ("ts_overlap_launch.h", "ts_bvh_layout.h", "ts_bvh_walk.h", os.path.join("..", "..", "include", "ts_overlap.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.overlap_command("mesh_winding")
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "mesh_overlap.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_overlap.so" in open(build.OVERLAP_LIB + ".cmd").read()


def test_the_unit_walks_with_the_shared_header_and_reads_the_shared_layout():
    build = _load("ts2d_build_overlap3", ("build.py",))
    text = open(os.path.join(build.CSRC, "mesh_overlap.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert '#include "ts_bvh_layout.h"' in text and '#include "ts_bvh_walk.h"' in text and "struct Leaf" not in code
    for used in ("WalkShared", "walk_levels", "bvh_walk<false>", "for_each_face", "NoChildKey"):
        assert used in code, used
    for absent in ("walk_query", "__syncthreads", "knn_prepare", "<< 28", "printf", "assert("):  # queries of its own, no barrier, no front half
        assert absent not in code, absent
    assert len(re.findall(r"__global__[^;{]*overlap_kernel", code)) == 1  # one walking kernel, a template over the mode


def test_size_query_and_index_sizes(lib, overlap_path):
    prev = -1
    for n in [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 65_537, 2_499_999, 2_500_000, 2_500_001, 5_000_000, 2 ** 31 - 1025]:
        got = lib.tsx_sort_workspace_bytes(n)
        assert got >= 25 * n and got >= prev, (n, got, prev)  # four words, a copy of the pair and of the kind, per pair
        prev = got
    from diff_triangle_rasterization_2D import _abi
    bvh = _abi.bind_bvh(ctypes.CDLL(os.path.join(os.path.dirname(overlap_path), "libts_bvh.so")))
    P = 0x1000
    for F in (1, 8, 9, 64, 65, 513, 4097, 1_000_000):  # one byte short of the other library's size query is refused, on either side
        need = bvh.tsb_bvh_bytes(F)
        assert lib.tsx_overlap(F, P, need - 1, P, 0, None, 0, P, None, P, 0, None, None, None, None) == INVALID
        assert b"bvh_a too small" in lib.tsx_last_error() and str(need).encode() in lib.tsx_last_error()
        assert lib.tsx_overlap(1, P, 1 << 40, None, F, P, need - 1, P, None, P, 0, None, None, None, None) == INVALID
        assert b"bvh_b too small" in lib.tsx_last_error() and str(need).encode() in lib.tsx_last_error()


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word):
        assert rc == INVALID, rc
        text = lib.tsx_last_error()
        assert text and word.encode() in text, text

    def self_(FA=1, bvh=P, bvh_bytes=big, faces=P, FB=0, bvh_b=None, bvh_b_bytes=0, count_a=P, count_b=None, stats=P, capacity=0, pairs=None,
              kind=None):
        return lib.tsx_overlap(FA, bvh, bvh_bytes, faces, FB, bvh_b, bvh_b_bytes, count_a, count_b, stats, capacity, pairs, kind, None, None)

    def cross(**kw):
        return self_(**{**dict(faces=None, FB=1, bvh_b=P, bvh_b_bytes=big), **kw})

    refused(self_(FA=-1), "FA")
    refused(self_(FA=2 ** 31 - 1), "at most")
    refused(cross(FB=-1), "FB")
    refused(cross(FB=2 ** 31 - 1), "at most")
    refused(self_(capacity=-1), "capacity")
    refused(self_(capacity=4), "pairs/kind is null")
    refused(self_(capacity=4, pairs=P), "pairs/kind is null")
    refused(self_(capacity=4, kind=P), "pairs/kind is null")
    refused(self_(stats=None), "stats is null")
    refused(self_(count_a=None), "count_a is null")
    refused(self_(bvh=None), "bvh_a is null")
    refused(self_(FA=1000, bvh_bytes=1000), "bvh_a too small")
    refused(self_(FB=1), "self mode")
    refused(self_(bvh_b=P), "self mode")
    refused(self_(count_b=P), "self mode")
    refused(cross(bvh_b=None), "bvh_b is null")
    refused(cross(FB=1000, bvh_b_bytes=1000), "bvh_b too small")
    refused(cross(stats=None), "stats is null")

    def sort(P_=1, bits_first=1, bits_second=1, pairs=P, kind=P, ws=P, ws_bytes=big):
        return lib.tsx_sort_pairs(P_, bits_first, bits_second, pairs, kind, ws, ws_bytes, None)

    refused(sort(P_=-1), "P")
    refused(sort(P_=2 ** 31 - 1), "at most")
    for bits in (0, 32, -1):
        refused(sort(bits_first=bits), "bits_first")
        refused(sort(bits_second=bits), "bits_second")
    refused(sort(P_=0, bits_first=0), "bits_first")  # the values are checked whatever the count
    refused(sort(pairs=None), "null")
    refused(sort(kind=None), "null")
    refused(sort(ws=None), "workspace is null")
    refused(sort(P_=1000, ws_bytes=lib.tsx_sort_workspace_bytes(1000) - 1), "workspace too small")
    assert sort(P_=0, pairs=None, kind=None, ws=None, ws_bytes=0) == 0  # the no-op


# ---- the package ------------------------------------------------------------------------------------------------------------------------------
def test_package_re_exports_the_feature(overlap_path):
    import diff_recon_hip
    from diff_recon_hip import mesh_overlap
    for name in mesh_overlap.__all__:
        assert getattr(diff_recon_hip, name) is getattr(mesh_overlap, name)
    assert sorted(mesh_overlap.__all__) == sorted(diff_recon_hip._OVERLAP_NAMES)
    assert callable(diff_recon_hip.MeshBVH.overlap)
    sig = inspect.signature(diff_recon_hip.MeshBVH.overlap).parameters
    assert list(sig)[:3] == ["self", "other", "capacity"] and sig["other"].default is None and sig["capacity"].default is None
    assert list(inspect.signature(diff_recon_hip.mesh_intersections).parameters)[:2] == ["mesh_a", "mesh_b"]
    assert (mesh_overlap.KIND_CROSSING, mesh_overlap.KIND_COPLANAR, mesh_overlap.KIND_DUPLICATE) == (ref.KIND_CROSSING, ref.KIND_COPLANAR, ref.KIND_DUPLICATE)
    assert mesh_overlap.STATS_KEYS == ref.STATS_KEYS
    assert mesh_overlap.MeshOverlap._fields == ("pairs", "kind", "count", "count_b", "stats")
    assert [mesh_overlap.default_capacity(n) for n in (0, 8191, 8192, 80_000)] == [1024, 1024, 1024, 10_000]
    assert [mesh_overlap._bits(n) for n in (0, 1, 2, 3, 256, 257, 2 ** 31 - 1)] == [1, 1, 1, 2, 8, 9, 31]


def test_wrappers_check_their_arguments_before_the_device(overlap_path):
    import torch
    from diff_recon_hip import mesh_overlap
    with pytest.raises(TypeError, match="MeshBVH"):
        mesh_overlap.overlap((torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # the index itself refuses host tensors
        mesh_overlap.self_intersections((torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="faces must be"):
        mesh_overlap.self_intersection_report((torch.zeros(3, 3), torch.zeros(1, 3)))


def test_example_takes_the_flag():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--check-intersections" in r.stdout
    r = subprocess.run([sys.executable, example, "--check-intersections"], capture_output=True, text=True)
    assert r.returncode == 2 and "--check-intersections" in r.stderr and "--extract-mesh" in r.stderr
