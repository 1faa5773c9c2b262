"""CPU tests of what the indexed-mesh units share (csrc/ts_mesh_common.h, ts_mesh_scan.h, ts_mesh_runs.h, ts_mesh_edges.h; no GPU): every
shared name is defined once, in a header; the units include what they use; no unit whose calls are captured in graphs clears or copies
with a memset or memcpy node; a header edit rebuilds the units; and the six size queries answer what they answered before the shared
pieces were single-sourced, byte for byte (tests/golden/mesh_workspace_bytes.json)."""
import glob
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHARED_HEADERS = ("ts_mesh_common.h", "ts_mesh_scan.h", "ts_mesh_runs.h", "ts_mesh_edges.h")
# shared name -> the header that defines it.  scan_offsets_kernel: the one-workgroup offsets kernel; edge_run_head: the run classifier
DEFINED_IN = {
    "blocks256": "ts_mesh_common.h", "bit_length": "ts_mesh_common.h", "finite32": "ts_mesh_common.h", "finite64": "ts_mesh_common.h",
    "count_into": "ts_mesh_common.h", "count4_into": "ts_mesh_common.h", "next_corner": "ts_mesh_common.h",
    "face_in_range": "ts_mesh_common.h", "face_takes_part": "ts_mesh_common.h", "edge_run_head": "ts_mesh_common.h",
    "sort_scratch_bytes": "ts_mesh_common.h", "Carver": "ts_mesh_common.h",
    "mesh_fill_kernel": "ts_mesh_common.h", "mesh_copy_kernel": "ts_mesh_common.h", "fill_blocks": "ts_mesh_common.h",
    "mesh_fill": "ts_mesh_common.h", "mesh_copy": "ts_mesh_common.h",
    "block_scan256": "ts_mesh_scan.h", "scan_offsets_kernel": "ts_mesh_scan.h", "scan_count_kernel": "ts_mesh_scan.h",
    "scan_apply_kernel": "ts_mesh_scan.h", "scan_columns": "ts_mesh_scan.h",
    "run_bounds_kernel": "ts_mesh_runs.h",
    "half_edge_records": "ts_mesh_edges.h", "other_end_kernel": "ts_mesh_edges.h", "edge_sort_carve": "ts_mesh_edges.h",
    "sort_half_edges": "ts_mesh_edges.h",
}
# unit -> the shared headers it names itself (ts_mesh_common.h comes with each of the other three)
INCLUDES = {
    "mesh_weld.hip": {"ts_mesh_scan.h"}, "mesh_simplify.hip": {"ts_mesh_runs.h"}, "mesh_smooth.hip": {"ts_mesh_runs.h", "ts_mesh_scan.h"},
    "mesh_holes.hip": {"ts_mesh_scan.h"}, "mesh_manifold.hip": {"ts_mesh_edges.h", "ts_mesh_scan.h"}, "mesh_orient.hip": {"ts_mesh_edges.h"},
    "mesh_subdivide.hip": {"ts_mesh_edges.h", "ts_mesh_scan.h"}, "mesh_flip.hip": {"ts_mesh_edges.h", "ts_mesh_scan.h"},
    # the two that take mesh_fill / mesh_copy alone name the common header itself
    "mesh_overlap.hip": {"ts_mesh_common.h"}, "mesh_distance.hip": {"ts_mesh_common.h"},
}
# every unit that clears or copies: each launches mesh_fill, and the ones that copied launch mesh_copy
FILLS = ("mesh_holes.hip", "mesh_manifold.hip", "mesh_subdivide.hip", "mesh_smooth.hip", "mesh_orient.hip", "mesh_overlap.hip", "mesh_flip.hip",
         "mesh_weld.hip", "mesh_simplify.hip", "mesh_distance.hip")
COPIES = ("mesh_manifold.hip", "mesh_orient.hip", "mesh_overlap.hip")
PROVIDES = {h: {n for n, where in DEFINED_IN.items() if where == h} for h in SHARED_HEADERS}


def _build_module():
    spec = importlib.util.spec_from_file_location("ts2d_build_mesh_common", os.path.join(ROOT, "triangle-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _strip(text):
    """Program text without its comments: a name in a sentence is neither a definition nor a use."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _code(path):
    return _strip(open(path).read())


def _definitions(name, code):
    if name == "Carver":
        return len(re.findall(r"\bstruct\s+Carver\b[^;{]*\{", code))
    # "type name(parameters) {": behind a type, a qualifier or __launch_bounds__(n), the parameters with at most one level of parentheses
    # inside them (int32_t (&v)[3]); a call ends in ; or stands behind an operator or a parenthesis
    return len(re.findall(r"[\w>*&)]\s+[*&]?%s\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*\{" % name, code))


def test_every_shared_name_is_defined_once_and_in_its_header():
    csrc = _build_module().CSRC
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) > 40
    codes = {os.path.basename(p): _code(p) for p in files}
    for name, header in DEFINED_IN.items():
        found = {f: _definitions(name, c) for f, c in codes.items() if _definitions(name, c)}
        assert found == {header: 1}, (name, found)
    # the copies that went: nothing under csrc/ still carries a name of theirs
    for gone in ("root_offsets_kernel", "head_offsets_kernel", "scan2_offsets_kernel", "scan2_count_kernel", "scan2_apply_kernel", "heads_a_pair",
                 "face_ok", "face_indices", "takes_part"):
        assert not [f for f, c in codes.items() if re.search(r"\b%s\b" % gone, c)], gone


def test_definition_counter_tells_a_definition_from_a_call():
    code = "__device__ int f(int a)\n{\n    return g(a);\n}\nvoid h() { if (f(1)) { f(2); } }\nstruct Carver // c\n{ int p; };\nCarver w(ws);"
    code = re.sub(r"//[^\n]*", "", code)
    assert _definitions("f", code) == 1 and _definitions("g", code) == 0 and _definitions("h", code) == 1 and _definitions("Carver", code) == 1


def test_the_units_include_what_they_use():
    csrc = _build_module().CSRC
    for header in SHARED_HEADERS[1:]:
        assert '#include "ts_mesh_common.h"' in open(os.path.join(csrc, header)).read(), header
    for unit, headers in INCLUDES.items():
        text, code = open(os.path.join(csrc, unit)).read(), _code(os.path.join(csrc, unit))
        named = set(re.findall(r'#include "(ts_mesh_\w+\.h)"', text))
        assert named == headers, (unit, named)
        reachable = PROVIDES["ts_mesh_common.h"].union(*(PROVIDES[h] for h in headers))
        used = {n for n in DEFINED_IN if re.search(r"\b%s\b" % n, code)}
        assert used <= reachable, (unit, used - reachable)
        for h in headers:  # no header is included for nothing
            assert used & PROVIDES[h], (unit, h)
    # a kernel that is not a template is emitted into every unit that sees its definition: only its users include its header
    for header, launcher in (("ts_mesh_runs.h", "run_bounds_kernel"), ("ts_mesh_edges.h", "sort_half_edges")):  # sort_half_edges launches other_end_kernel
        for unit, headers in INCLUDES.items():
            assert (header in headers) == bool(re.search(r"\b%s\b" % launcher, _code(os.path.join(csrc, unit)))), (unit, launcher)
    common = _code(os.path.join(csrc, "ts_mesh_common.h"))  # its only kernels are the fill and the copy, and both are templates
    assert len(re.findall(r"template <int = 0>\s*__global__", common)) == common.count("__global__") == 2
    assert len(re.findall(r"__global__ void __launch_bounds__\(256\) mesh_(?:fill|copy)_kernel\b", common)) == 2
    scan = _code(os.path.join(csrc, "ts_mesh_scan.h"))
    assert len(re.findall(r"template <int COLS>\s*__global__", scan)) == scan.count("__global__") == 3  # templates: emitted where launched


# Every unit behind a header whose calls "can be captured in a graph" (tests/test_graph_replay_gpu.py), with the launch headers, the shared
# headers and the C-ABI files of those libraries: a memset or a copy node of a graph does not reliably run where stream order put it
# (DESIGN.md 13b), so these clear and copy with kernels (mesh_fill, mesh_copy, ts_launch_zero_words).
CAPTURABLE = ("mesh_*.hip", "api_*.hip", "volume.hip", "color_volume.hip", "knn.hip", "radix_sort.hip", "ts_*.h")


def test_no_memset_or_memcpy_is_left_in_the_capturable_units():
    csrc = _build_module().CSRC
    files = sorted({p for pattern in CAPTURABLE for p in glob.glob(os.path.join(csrc, pattern))})
    names = {os.path.basename(p) for p in files}
    assert len(files) > 50 and {"mesh_holes.hip", "mesh_manifold.hip", "mesh_subdivide.hip", "mesh_smooth.hip", "mesh_orient.hip", "mesh_overlap.hip",
                                "mesh_flip.hip", "mesh_weld.hip", "mesh_simplify.hip", "mesh_distance.hip", "ts_mesh_common.h"} <= names
    left = {os.path.basename(p): sorted(set(re.findall(r"\bhipMem(?:set|cpy)\w*", _code(p)))) for p in files}
    assert {f: calls for f, calls in left.items() if calls} == {}
    # the scanner sees what it looks for, with the scan's own comment stripping: in a call, not in a comment of either kind
    sample = "e = hipMemsetAsync(p, 0, n, s); // hipMemcpyAsync\n/* hipMemset(p)\n hipMemcpyDtoD */ hipMemcpy2DAsync(a);"
    assert re.findall(r"\bhipMem(?:set|cpy)\w*", _strip(sample)) == ["hipMemsetAsync", "hipMemcpy2DAsync"]
    # and what replaced them is what the units launch
    for unit in sorted(n for n in names if n.startswith("mesh_") and n.endswith(".hip")):
        code = _code(os.path.join(csrc, unit))
        assert bool(re.search(r"\bmesh_fill\(", code)) == (unit in FILLS), unit
        assert bool(re.search(r"\bmesh_copy\(", code)) == (unit in COPIES), unit


def test_a_header_edit_rebuilds_the_units():
    build = _build_module()
    for header in SHARED_HEADERS:
        assert header in build.HEADERS and os.path.exists(os.path.join(build.CSRC, header)), header
    # header-only: no object and no library of its own
    for names in (build.units(), build.simplify_units(), build.smooth_units(), build.holes_units(), build.manifold_units(), build.orient_units()):
        assert not [n for n in names if n.startswith("ts_mesh_")]


def test_weld_carves_on_integer_addresses():
    code = _code(os.path.join(_build_module().CSRC, "mesh_weld.hip"))
    assert "Carver w(" in code and "char *" not in code  # no pointer arithmetic from a null workspace in the size query


def test_size_queries_answer_what_they_answered_before(hip_lib_built):
    spec = importlib.util.spec_from_file_location("make_golden_mesh_workspace_bytes", os.path.join(GOLDEN, "make_golden_mesh_workspace_bytes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(os.path.join(GOLDEN, "mesh_workspace_bytes.json")))
    assert want["sizes"] == list(gen.SIZES) and want["fixed"] == list(gen.FIXED) and set(want["queries"]) == set(gen.QUERIES) and len(gen.QUERIES) == 6
    for n in (682, 683, 416666, 416667, 833333, 833334, 2499999, 2500000, 2500001):  # either side of the radix sort's chunk switch, per record width
        assert n in gen.SIZES
    got = gen.measure()
    for name in gen.QUERIES:
        for side in ("by_v", "by_f"):
            assert len(want["queries"][name][side]) == len(gen.FIXED) and all(len(r) == len(gen.SIZES) for r in want["queries"][name][side])
            assert got["queries"][name][side] == want["queries"][name][side], (name, side)
