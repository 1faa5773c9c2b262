"""CPU tests of the one walk of the triangle index (csrc/ts_bvh_walk.h; no GPU), after tests/test_mesh_common_cpu.py: every name the header
provides is defined once, in it; the three units that walk the index with it carry no copy of what it holds (mesh_ray.hip keeps a walk
of its own, for its speed, and shares the carve only); a header edit rebuilds the units; and the four workspace size queries answer what
they answered before the walk was single-sourced, byte for byte (tests/golden/bvh_walk_bytes.json)."""
import glob
import importlib.util
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = "ts_bvh_walk.h"
UNITS = ("mesh_bvh.hip", "mesh_ray.hip", "mesh_inside.hip", "mesh_winding.hip")
WALKERS = ("mesh_bvh.hip", "mesh_inside.hip", "mesh_winding.hip")  # on the shared walk; cast_kernel of mesh_ray.hip kept its own
FUNCTIONS = ("query_carve_bytes", "walk_levels", "walk_query", "for_each_face", "walk_push", "bvh_walk")
STRUCTS = ("WalkShared", "WalkQuery", "NoChildKey")
# what a unit with a walk of its own would carry: the stacks, the level table, a carve of its own, the child ordering
GONE = ("__shared__ uint32_t stack", "lvl_off[tid]", "ray_carve_bytes", "inside_carve_bytes", "winding_carve_bytes", "far_key")


def _module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build_module():
    return _module("ts2d_build_bvh_walk", os.path.join(ROOT, "triangle-splatting_amd", "build.py"))


def _code(path):
    """The file without its comments: a name in a sentence is neither a definition nor a use."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


def _definitions(name, code):
    if name in STRUCTS:
        return len(re.findall(r"\bstruct\s+%s\b[^;{]*\{" % name, code))
    # "type name(parameters) {": the parameters with at most one level of parentheses inside them; a call ends in ; or stands in an expression
    return len(re.findall(r"[\w>*&)]\s+[*&]?%s\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*\{" % name, code))


def test_every_name_of_the_header_is_defined_once_and_in_it():
    csrc = _build_module().CSRC
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) > 40
    codes = {os.path.basename(p): _code(p) for p in files}
    for name in FUNCTIONS + STRUCTS:
        found = {f: _definitions(name, c) for f, c in codes.items() if _definitions(name, c)}
        assert found == {HEADER: 1}, (name, found)


def test_definition_counter_tells_a_definition_from_a_call():
    code = ("template <class F>\n__device__ __forceinline__ void for_each_face(const Leaf &lf, F face)\n{\n    face(1);\n}\nstruct WalkShared\n{ int a; };\n"
            "void k() { __shared__ WalkShared ws; for_each_face(l, [&](int id) { n++; }); bvh_walk<false>(ws, 1, [&](int) { return true; }); }")
    assert _definitions("for_each_face", code) == 1 and _definitions("WalkShared", code) == 1 and _definitions("bvh_walk", code) == 0


def test_the_four_units_walk_with_the_header_and_carry_no_copy():
    csrc = _build_module().CSRC
    header = open(os.path.join(csrc, HEADER)).read()
    assert '#include "ts_bvh_layout.h"' in header and _code(os.path.join(csrc, HEADER)).count("__syncthreads()") == 1
    assert _code(os.path.join(csrc, HEADER)).count("sp < STACK") == 1 and "__global__" not in _code(os.path.join(csrc, HEADER))
    for unit in UNITS:
        text, code = open(os.path.join(csrc, unit)).read(), _code(os.path.join(csrc, unit))
        assert '#include "ts_bvh_walk.h"' in text and "query_carve_bytes" in code, unit
        for gone in ("ray_carve_bytes", "inside_carve_bytes", "winding_carve_bytes", "constexpr int WAVES"):
            assert gone not in code, (unit, gone)
    for unit in WALKERS:
        code = _code(os.path.join(csrc, unit))
        for gone in GONE:
            assert gone not in code, (unit, gone)
        assert "__syncthreads" not in code and "readfirstlane(st[" not in code and "<< 28" not in code, unit  # the barrier, the pop, the packing
        for used in ("WalkShared", "walk_levels", "walk_query", "for_each_face", "bvh_walk", "query_carve_bytes"):
            assert re.search(r"\b%s\b" % used, code), (unit, used)
    # the two push policies and who uses which
    policy = {u: re.findall(r"bvh_walk<(\w+)>", _code(os.path.join(csrc, u))) for u in UNITS}
    assert policy == {"mesh_bvh.hip": ["true"], "mesh_ray.hip": [], "mesh_inside.hip": ["false"], "mesh_winding.hip": ["false"]}
    # which rays are cast at all: the rule lives with the ray tests, once
    tests_h = _code(os.path.join(csrc, "ts_ray_tests.h"))
    assert _definitions("ray_valid", tests_h) == 1 and _definitions("ray_direction_valid", tests_h) == 1
    for unit in ("mesh_ray.hip", "mesh_inside.hip"):
        code = _code(os.path.join(csrc, unit))
        assert "ray_valid(" in code and "ray_direction_valid(" in code and "finite_f(" not in code, unit


def test_a_header_edit_rebuilds_the_units():
    build = _build_module()
    assert HEADER in build.HEADERS and os.path.exists(os.path.join(build.CSRC, HEADER))
    for names in (build.units(), build.bvh_units(), build.ray_units(), build.inside_units(), build.winding_units()):  # header-only: no object
        assert not [n for n in names if n.startswith("ts_bvh_")]


def test_no_faces_kernels_are_launched_by_their_own_block_size():
    csrc = _build_module().CSRC
    for unit in UNITS:
        code = _code(os.path.join(csrc, unit))
        launches = re.findall(r"hipLaunchKernelGGL\(no_faces_kernel,\s*dim3\(([^;]*?)\),\s*dim3\((\w+)\)", code)
        assert len(launches) == 1 and launches[0][1] == "256" and "255) / 256" in launches[0][0] and "TPB" not in launches[0][0], (unit, launches)


def test_size_queries_answer_what_they_answered_before(hip_lib_built):
    gen = _module("make_golden_bvh_walk", os.path.join(GOLDEN, "make_golden_bvh_walk.py"))
    want = json.load(open(os.path.join(GOLDEN, "bvh_walk_bytes.json")))
    small = gen.SMALL_BELOW
    assert "#define TS_RS_SMALL_BELOW %d " % small in open(os.path.join(_build_module().CSRC, "ts2d_common.h")).read()
    assert want["sizes"] == list(gen.SIZES) == [0, 1, 63, 64, 65, 1023, 1024, 1025, small - 1, small, small + 1, 5000000, 2 ** 31 - 1025]
    assert set(want["queries"]) == set(gen.QUERIES) == {"tsb_closest_workspace_bytes", "tsr_cast_workspace_bytes", "tsi_crossings_workspace_bytes",
                                                         "tsn_winding_workspace_bytes"}
    got = gen.measure_bytes()
    for name in gen.QUERIES:
        assert len(want["queries"][name]) == len(gen.SIZES) and got["queries"][name] == want["queries"][name], name
