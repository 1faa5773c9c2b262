"""CPU tests of the non-manifold split (no GPU): the numpy reference finds the same fans by a union-find and by a plain walk around every
vertex, keeps the promises of include/ts_manifold.h on every fixture and reproduces the figures of DESIGN.md 16l; libts_manifold.so is a
library of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_holes
import ref_mesh_manifold as ref
import ref_mesh_simplify as fixtures
import ref_mesh_weld
import ref_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_manifold.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsf_fans", "tsf_last_error", "tsf_split", "tsf_workspace_bytes"]
MAX_FACES = 715827882


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_manifold", ("diff_triangle_rasterization_2D", "_abi.py"))


MANIFOLD_SIGNATURES = _abi_module().MANIFOLD_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def manifold_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_manifold.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_manifold.so"
    return path


@pytest.fixture(scope="module")
def lib(manifold_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_manifold(ctypes.CDLL(manifold_path))


def _header_prototypes():
    """name -> number of parameters of every tsf_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the fixtures: computed once, never changed ---------------------------------------------------------------------------------------------------
def _pinched_sphere():
    """test_mesh_holes_cpu._pinched_sphere: the sphere with two fan faces of vertex 100 removed that share only that vertex."""
    v, f = fixtures.sphere_mesh()
    fan = np.nonzero((f == 100).any(1))[0]
    pair = next((a, b) for a in fan for b in fan if a < b and len(set(f[a]) & set(f[b])) == 1)
    return v, np.delete(f, pair, axis=0)


@functools.lru_cache(maxsize=None)
def _simplified(cell):
    v, f = fixtures.sphere_mesh()
    s = fixtures.simplify(v, f, cell, v.min(0) - 0.01)
    return s["vertices"], s["faces"], s["flaps"]


def _positions(V):
    return np.random.default_rng(V).uniform(-1, 1, (V, 3)).astype(np.float32)


def _indexed(builder):
    V, f = builder()[:2]
    return _positions(V), f


FIXTURES = {
    "sphere": fixtures.sphere_mesh,
    "pinched": _pinched_sphere,
    "kissing": lambda: ref.kissing(*fixtures.sphere_mesh()),
    "tetrahedra": lambda: _indexed(ref.two_tetrahedra),
    "book3": lambda: _indexed(lambda: ref.book(3)),
    "book4": lambda: _indexed(lambda: ref.book(4)),
    "hub5": lambda: _indexed(lambda: ref.hub(5)),
    "cones": lambda: _indexed(lambda: ref.cones((3, 7), seed=1)),
    "cell2": lambda: _simplified(2.0)[:2],
    "cell4": lambda: _simplified(4.0)[:2],
    "cell6": lambda: _simplified(6.0)[:2],
    "cell8": lambda: _simplified(8.0)[:2],
    "soup63": lambda: (_positions(63), ref.soups()[63]),
    "soup257": lambda: (_positions(257), ref.soups()[257]),
    "soup1025": lambda: (_positions(1025), ref.soups()[1025]),
}
# (vertices split, new vertices, edges used three times or more before)
FIGURES = {"sphere": (0, 0, 0), "pinched": (1, 1, 0), "kissing": (1, 1, 0), "tetrahedra": (2, 2, 1), "book3": (2, 4, 1), "cell2": (30, 63, 30),
           "cell4": (17, 35, 16), "cell6": (15, 63, 18), "cell8": (3, 5, 2), "soup63": (62, 240, 1), "soup257": (247, 1180, 0),
           "soup1025": (1007, 5044, 0)}


@functools.lru_cache(maxsize=None)
def _case(name):
    v, f = FIXTURES[name]()
    before, sp, after = ref.check_promises(len(v), f)  # the promises, on every fixture
    w = np.concatenate([v, v[sp["new_vertex_source"]]])
    return v, f, before, sp, after, w, sp["out_faces"]


# ---- the two forms of the reference agree, the promises hold, the figures are the table's -------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_union_find_and_walking_find_the_same_fans_and_the_promises_hold(name):
    v, f, before, sp, after, w, g = _case(name)
    walked = ref.fans(len(v), f, walk=True)
    for key in ("corner_fan", "vertex_fans"):
        assert np.array_equal(before[key], walked[key]) and before[key].dtype == np.int32, key
    assert before["counts"] == walked["counts"]
    F, V = len(f), len(v)
    assert before["corner_fan"].shape == (3 * F,) and before["vertex_fans"].shape == (V,) and g.shape == (F, 3) and g.dtype == np.int32
    fan, flat = before["corner_fan"], np.asarray(f).reshape(-1)
    part = fan >= 0
    assert (fan[part] <= np.nonzero(part)[0]).all() and (fan[fan[part]] == fan[part]).all()  # labelled by the smallest corner, itself a root
    assert (flat[fan[part]] == flat[part]).all()                                            # all corners of a fan sit on one vertex
    assert before["vertex_fans"].sum() == before["counts"][1] and len(w) == V + before["new_vertices"]
    assert np.array_equal(w[:V].view(np.uint32), v.view(np.uint32))                          # the old vertices first, bit for bit
    assert (sp["new_vertex_source"] >= 0).all() and (before["vertex_fans"][sp["new_vertex_source"]] >= 2).all()
    if name in FIGURES:
        split, new, nonmanifold = FIGURES[name]
        print(f"{name}: {V} V, {F} F: {before['counts'][3]} / {before['new_vertices']} split / new vertices, {before['counts'][4]} -> "
              f"{after['counts'][4]} edges used >= 3 times, {before['counts'][5]} same-direction edges")
        assert (before["counts"][3], before["new_vertices"], before["counts"][4], after["counts"][4]) == (split, new, nonmanifold, 0)
    else:
        assert before["counts"][3] > 0 or name == "book4"


def test_sphere_comes_back_bit_for_bit_and_the_small_fixtures_have_the_table_s_edges():
    v, f, before, sp, _, w, g = _case("sphere")
    assert (len(v), len(f)) == (4834, 9664) and np.array_equal(g, f.astype(np.int32)) and sp["totals"] == [0, 0]
    assert before["counts"] == [3 * 9664, 4834, 4834, 0, 0, 0]
    _, f, _, _, _, w, g = _case("tetrahedra")
    a, b = ref_volume.topology(f), ref_volume.topology(g)
    assert (len(f), a["edges"] - a["nonmanifold"] - a["boundary"], a["nonmanifold"]) == (8, 10, 1) and len(w) == 8
    assert (b["edges"] - b["nonmanifold"] - b["boundary"], b["nonmanifold"], b["boundary"]) == (12, 0, 0)
    v, f, _, _, _, w, g = _case("book3")
    assert (len(v), len(f)) == (5, 3) and ref_volume.topology(f)["boundary"] == 6 and ref_volume.topology(g)["boundary"] == 9
    _, f, before, _, _, w, g = _case("kissing")
    assert ref_mesh_weld.topology(len(w), g)["pieces"] == 2 and ref_mesh_weld.topology(len(w) - 1, f)["pieces"] == 1
    assert ref_volume.topology(g)["boundary"] == 0 and before["vertex_fans"][7] == 2


def test_hub_and_book_and_cones_have_the_fans_their_builders_promise():
    V, f = ref.hub(5)
    fn = ref.fans(V, f)
    assert fn["vertex_fans"][0] == 5 and fn["new_vertices"] == 4 and fn["counts"][3] == 1
    sp = ref.split(V, f, fn["corner_fan"], capacity=7)
    assert sp["new_vertex_source"].tolist() == [0, 0, 0, 0, -1, -1, -1] and sp["new_vertex_fan"].tolist() == [3, 6, 9, 12, -1, -1, -1]
    assert sp["out_faces"][:, 0].tolist() == [0, V, V + 1, V + 2, V + 3] and sp["totals"] == [4, 4]
    assert ref.split(V, f, fn["corner_fan"], capacity=2)["new_vertex_fan"].tolist() == [3, 6]  # a short capacity lists the first ones
    V, f = ref.book(4)
    fn = ref.fans(V, f)
    assert fn["vertex_fans"][:2].tolist() == [4, 4] and fn["counts"][4] == 1 and fn["new_vertices"] == 6
    V, f, apexes = ref.cones((3, 7), seed=1)
    fn = ref.fans(V, f)
    for apex, n in apexes:
        assert fn["vertex_fans"][apex] == n
    assert fn["counts"][3] == 1 and fn["new_vertices"] == 1 and fn["counts"][4] == 0


def test_same_direction_edges_are_counted_and_still_linked():
    f = np.array([[0, 1, 2], [0, 1, 3]])  # both run 0 -> 1
    fn = ref.fans(4, f)
    assert fn["counts"] == [6, 4, 4, 0, 0, 1] and fn["corner_fan"].tolist() == [0, 1, 2, 0, 1, 5]
    f = np.array([[0, 1, 2], [1, 0, 3]])
    assert ref.fans(4, f)["counts"] == [6, 4, 4, 0, 0, 0]


def test_faces_that_do_not_take_part_come_back_bit_for_bit_and_a_foreign_table_stays_in_bounds():
    V, f = ref.hub(6)
    f = np.concatenate([f, [[-1, 0, 1], [0, V, 2], [3, 3, 0], [0, 1, 2]]])
    keep = np.ones(len(f), np.uint8)
    keep[1] = 0
    fn, sp, _ = ref.check_promises(V, f, keep)
    assert (fn["corner_fan"][3:6] == -1).all() and (fn["corner_fan"][18:27] == -1).all() and fn["counts"][0] == 18
    assert fn["counts"][5] == 3 and fn["corner_fan"][27:].tolist() == [0, 1, 2]  # the repeated face runs the same way and is linked to its twin
    assert np.array_equal(sp["out_faces"][[1, 6, 7, 8]], f[[1, 6, 7, 8]].astype(np.int32)) and sp["totals"] == [4, 4]
    foreign = fn["corner_fan"].copy()
    foreign[0], foreign[6], foreign[9], foreign[27] = 3 * len(f), 1, 3, -7  # out of range, another vertex, an excluded face, negative
    got = ref.split(V, f, foreign, keep)
    clean = foreign.copy()
    clean[[0, 6, 9, 27]] = -1
    want = ref.split(V, f, clean, keep)
    assert np.array_equal(got["out_faces"], want["out_faces"]) and got["totals"] == want["totals"] == [1, 1]
    assert got["new_vertex_fan"].tolist() == [15] and got["new_vertex_source"].tolist() == [0]  # corner 12 keeps vertex 0, corner 15 moves
    assert got["out_faces"][[0, 2, 3, 9], 0].tolist() == [0, 0, 0, 0] and got["out_faces"][5, 0] == V


# ---- through the hole filling and the edge census ---------------------------------------------------------------------------------------------
def test_pinched_sphere_closes_after_the_split():
    v, f, before, sp, _, w, g = _case("pinched")
    lp = ref_mesh_holes.loops(len(v), f)
    assert lp["counts"] == [6, 0, 0, 1] and lp["num_loops"] == 0           # no loop: the pinch opens both holes
    lp = ref_mesh_holes.loops(len(w), g)
    assert lp["counts"] == [6, 6, 1, 0] and ref_mesh_holes.loop_lengths(lp).tolist() == [6]  # ONE loop over both copies
    fl = ref_mesh_holes.fill(w, g, lp)
    x, h = ref_mesh_holes.filled_mesh(w, g, lp, fl)
    t = ref_volume.topology(h)
    assert (t["boundary"], t["euler"], len(x), len(h)) == (0, 2, 4836, 9668)


@pytest.mark.parametrize("cell,flaps,boundary,loops", [(2.0, 22, 89, [3] * 24 + [4, 6, 7]), (4.0, 12, 52, None)])
def test_split_simplified_spheres_are_manifold_and_fill_to_lone_flaps(cell, flaps, boundary, loops):
    name = "cell%d" % cell
    v, f, before, sp, _, w, g = _case(name)
    assert _simplified(cell)[2] == flaps and (len(v), len(f)) == {2.0: (356, 719), 4.0: (89, 182)}[cell]
    assert ref_volume.topology(f)["boundary"] == 0 and ref_volume.topology(g)["boundary"] == boundary
    assert ref_mesh_weld.topology(len(v), f)["nonmanifold"] == before["counts"][4] > 0 and ref_mesh_weld.topology(len(w), g)["nonmanifold"] == 0
    lp = ref_mesh_holes.loops(len(w), g)
    lengths = sorted(ref_mesh_holes.loop_lengths(lp).tolist())
    assert lp["counts"][3] == 0 and lp["counts"][0] == lp["counts"][1] == boundary and len(lengths) == (27 if cell == 2.0 else 15)
    if loops:
        assert lengths == loops
    fl = ref_mesh_holes.fill(w, g, lp)
    x, h = ref_mesh_holes.filled_mesh(w, g, lp, fl)
    t = ref_volume.topology(h)
    lone = int((fl["loop_status"] == ref_mesh_holes.LONE_FACE).sum())
    assert t["nonmanifold"] == 0 and t["boundary"] == 3 * lone and (fl["loop_status"] != ref_mesh_holes.FILLED).sum() == lone
    if cell == 2.0:
        assert (t["boundary"], lone) == (54, 18)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(manifold_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsf_last_error.restype = ctypes.c_char_p; "
            "l.tsf_workspace_bytes.restype = ctypes.c_size_t; print(l.tsf_workspace_bytes(100000, 200000) >= 24 * 3 * 200000, "
            "repr(l.tsf_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, manifold_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(manifold_path):
    out = subprocess.run(["nm", "-D", "--defined-only", manifold_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 4
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", manifold_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", manifold_path], capture_output=True, text=True).stdout
    assert "libts_manifold.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so", "libts_color.so", "libts_simplify.so",
                  "libts_smooth.so", "libts_holes.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss|tsh)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("TAKES PART", "CORNER", "EXACTLY TWICE", "FAN", "KEEPS", "NEW VERTEX", "SAME direction", "smallest corner", "ascending fan label",
                 "a foreign table stays in bounds", "bit for bit", "no floating-point", "compare-exchange", "nobody waits for anybody", "715827882",
                 "6-loop", "merged, not paired", "Monotonic", "path or a cycle"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(MANIFOLD_SIGNATURES) and len(declared) == 4
    for name, arity in declared.items():
        assert len(MANIFOLD_SIGNATURES[name][1]) == arity, name
    assert declared["tsf_fans"] == 10 and declared["tsf_split"] == 13
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES,
              abi.COLOR_SIGNATURES, abi.SIMPLIFY_SIGNATURES, abi.SMOOTH_SIGNATURES, abi.HOLES_SIGNATURES, abi.MANIFOLD_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert MANIFOLD_SIGNATURES["tsf_fans"][1][8] == ctypes.c_size_t and MANIFOLD_SIGNATURES["tsf_split"][1][11] == ctypes.c_size_t
    assert MANIFOLD_SIGNATURES["tsf_workspace_bytes"][0] == ctypes.c_size_t


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_manifold", ("build.py",))
    assert build.MANIFOLD_SOURCES == {"mesh_manifold.hip": [], "api_manifold.hip": []} and build.MANIFOLD_SHARED == ["radix_sort"]
    assert build.manifold_units() == ["mesh_manifold", "api_manifold"]
    cmd = build.manifold_command("mesh_manifold", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" not in cmd and "-fvisibility=hidden" in cmd
    assert build.manifold_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_manifold", "api_manifold", "radix_sort")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units(), build.color_units(),
                   build.simplify_units(), build.smooth_units(), build.holes_units()):
        assert not {"mesh_manifold", "api_manifold"} & set(others)  # its own library only
    assert build.MANIFOLD_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_manifold.so")
    for header in ("ts_manifold_launch.h", "ts_union_find.h", os.path.join("..", "..", "include", "ts_manifold.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.manifold_command("mesh_holes")


def test_built_objects_carry_the_flags_and_the_union_find_is_single_sourced(manifold_path):
    build = _load("ts2d_build_manifold2", ("build.py",))
    for unit in ("mesh_manifold", "api_manifold"):
        stamp = open(os.path.join(build.OBJ_DIR, unit + ".o.cmd")).read()  # what the object on disk was compiled with
        assert stamp.endswith(" ".join(build.manifold_command(unit, cc=stamp.splitlines()[1].split()[0]))) and "-ffp-contract=off" not in stamp
    link = open(build.MANIFOLD_LIB + ".cmd").read()
    assert "-soname,libts_manifold.so" in link and "radix_sort.o" in link and "mesh_weld" not in link
    texts = {n: open(os.path.join(build.CSRC, n)).read() for n in ("mesh_weld.hip", "mesh_manifold.hip", "ts_union_find.h")}
    for name in ("mesh_weld.hip", "mesh_manifold.hip"):
        assert '#include "ts_union_find.h"' in texts[name] and "uf_union(" in texts[name]
        assert not re.search(r"\buf_(load|find|union)\s*\([^;{]*\)\s*\{", texts[name].replace("\n", " "))  # used there, defined in the header alone
    for fn in ("uf_load", "uf_find", "uf_union"):
        assert len(re.findall(r"__forceinline__ \w+ %s\(" % fn, texts["ts_union_find.h"])) == 1
    assert "Termination" in texts["ts_union_find.h"] and "No lane ever waits for another" in texts["ts_union_find.h"]


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsf_workspace_bytes(n, fixed), lib.tsf_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_v >= 4 * n and by_f >= 24 * 3 * n  # the keepers; two keys, two values, the other end and the parent per corner
            prev_v, prev_f = by_v, by_f
    assert lib.tsf_workspace_bytes(-5, -5) == lib.tsf_workspace_bytes(0, 0)
    assert lib.tsf_workspace_bytes(10, 2 ** 31 - 1) == lib.tsf_workspace_bytes(10, MAX_FACES)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsf_last_error()
        assert text and word.encode() in text, text

    def fans(V=10, F=20, faces=P, keep=None, corner_fan=P, vertex_fans=P, counts=P, ws=P, ws_bytes=big):
        return lib.tsf_fans(V, F, faces, keep, corner_fan, vertex_fans, counts, ws, ws_bytes, None)

    def split(V=10, F=20, faces=P, keep=None, corner_fan=P, capacity=4, out_faces=P, source=P, label=P, totals=P, ws=P, ws_bytes=big):
        return lib.tsf_split(V, F, faces, keep, corner_fan, capacity, out_faces, source, label, totals, ws, ws_bytes, None)

    for call in (fans, split):
        refused(call(V=-1), ">= 0")
        refused(call(V=-(2 ** 31)), ">= 0")
        refused(call(F=-1), ">= 0")
        refused(call(F=-(2 ** 31)), ">= 0")
        refused(call(F=MAX_FACES + 1), "exceeds", CAPACITY)
        refused(call(F=2 ** 31 - 1), "exceeds", CAPACITY)
        refused(call(ws=None), "workspace is null")
        refused(call(faces=None), "null")
        refused(call(corner_fan=None), "null")
    for name in ("counts", "vertex_fans"):
        refused(fans(**{name: None}), "null")
    for bad in (-1, -(2 ** 31)):
        refused(split(capacity=bad), "capacity")
    for name in ("totals", "out_faces", "source", "label"):
        refused(split(**{name: None}), "null")
    refused(split(V=2 ** 31 - 1, F=1), "exceeds", CAPACITY)  # V + 3 F: the index of a new vertex
    need = lib.tsf_workspace_bytes(1000, 2000)
    refused(fans(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsf_last_error()
    refused(split(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    # what the checks accept, for the record: keep may be null, the two lists may be null with capacity == 0, and nothing but counts /
    # totals is needed with V == 0 and F == 0 (those calls would reach the device, so they are made in tests/test_mesh_manifold_gpu.py)


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, manifold_path):
    """Without libts_manifold.so, diff_recon_hip.mesh_manifold raises and names the build command; everything else still imports."""
    src = os.path.dirname(manifold_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or (name.endswith(".so") and name != "libts_manifold.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.fill_holes), callable(diff_recon_hip.simplify_mesh))\n"
            "try:\n    diff_recon_hip.split_nonmanifold\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_manifold\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_manifold.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_manifold.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature_and_keeps_the_pinned_parameter_lists(manifold_path):
    import inspect

    import diff_recon_hip
    from diff_recon_hip import color_volume, mesh_holes, mesh_manifold, mesh_simplify, mesh_smooth, volume
    names = ("VertexFans", "ManifoldMesh", "vertex_fans", "split_nonmanifold", "manifold_fused")
    assert diff_recon_hip._MANIFOLD_NAMES == names
    for name in names:
        assert getattr(diff_recon_hip, name) is getattr(mesh_manifold, name)
    assert diff_recon_hip.mesh_manifold is mesh_manifold
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(mesh_manifold.vertex_fans) == ["num_vertices", "faces", "keep"]
    assert params(mesh_manifold.split_nonmanifold) == ["vertices", "faces", "vertex_attributes", "attribute_valid", "keep", "fans"]
    defaults = {k: p.default for k, p in inspect.signature(mesh_manifold.split_nonmanifold).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"vertex_attributes": None, "attribute_valid": None, "keep": None, "fans": None}
    assert params(mesh_manifold.manifold_fused) == ["mesh"]
    assert mesh_manifold.VertexFans._fields == ("corner_fan", "vertex_fans", "stats")
    assert mesh_manifold.ManifoldMesh._fields == ("vertices", "faces", "vertex_attributes", "attribute_valid", "source_vertex", "new_vertex", "fans", "stats")
    assert mesh_manifold.COUNT_NAMES == ref.COUNT_NAMES
    # the neighbours keep their parameter lists
    assert diff_recon_hip._HOLES_NAMES == ("BoundaryLoops", "FilledMesh", "boundary_loops", "loop_vertices", "fill_holes", "fill_fused")
    assert params(mesh_holes.boundary_loops) == ["num_vertices", "faces", "keep", "adjacency"]
    assert params(mesh_holes.fill_holes) == ["vertices", "faces", "max_loop_edges", "vertex_attributes", "attribute_valid", "keep", "loops"]
    assert params(mesh_holes.fill_fused) == ["mesh", "max_loop_edges"]
    assert params(mesh_simplify.simplify_fused) == ["mesh", "volume", "simplify_cell", "min_piece_faces"]
    assert params(mesh_smooth.smooth_fused) == ["mesh", "volume", "iterations", "max_move_voxels", "kw"]
    assert params(volume.fuse_mesh)[:4] == ["views", "vertices", "faces", "resolution"]
    assert params(color_volume.fuse_colored_mesh)[:5] == ["views", "vertices", "faces", "faces_color", "resolution"]
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_manifold.vertex_fans(4, torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_manifold.split_nonmanifold(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="num_vertices"):
        mesh_manifold.vertex_fans(-1, torch.zeros((2, 3), dtype=torch.int32))


def test_example_refuses_split_nonmanifold_without_extract_mesh():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--split-nonmanifold"], capture_output=True, text=True)
    assert r.returncode == 2 and "--split-nonmanifold splits the vertices of the mesh of --extract-mesh" in r.stderr
