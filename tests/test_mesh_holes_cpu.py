"""CPU tests of hole filling (no GPU): the numpy reference finds the same loops by pointer doubling and by a plain walk, keeps the promises
of include/ts_holes.h on the existing fixtures and reproduces the figures of DESIGN.md 16k; libts_holes.so is a library of its own with
exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_mesh_holes as ref
import ref_mesh_simplify as fixtures
import ref_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_holes.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsh_fill", "tsh_last_error", "tsh_loops", "tsh_workspace_bytes"]


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_holes", ("diff_triangle_rasterization_2D", "_abi.py"))


HOLES_SIGNATURES = _abi_module().HOLES_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def holes_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_holes.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_holes.so"
    return path


@pytest.fixture(scope="module")
def lib(holes_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_holes(ctypes.CDLL(holes_path))


def _header_prototypes():
    """name -> number of parameters of every tsh_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsh_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


# ---- the fixtures: computed once, never changed ---------------------------------------------------------------------------------------------------
def _pinched_sphere():
    """The sphere with two fan faces of vertex 100 removed that share only that vertex: two holes that meet in a pinch."""
    v, f = fixtures.sphere_mesh()
    fan = np.nonzero((f == 100).any(1))[0]
    pair = next((a, b) for a in fan for b in fan if a < b and len(set(f[a]) & set(f[b])) == 1)
    return v, np.delete(f, pair, axis=0)


FIXTURES = {
    "punched": ref.punched_sphere,
    "capped": ref.capped_sphere,
    "plane": lambda: fixtures.plane_grid()[:2],
    "fused": ref.fused_sphere,
    "nan_blocks": ref.nan_block_sphere,
    "lone": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]])),
    "pinched": _pinched_sphere,
    "closed": fixtures.sphere_mesh,
    "bands": lambda: ref.open_bands((3, 4, 5, 17), seed=2),
}


@functools.lru_cache(maxsize=None)
def _case(name, limit=ref.UNBOUNDED):
    v, f = FIXTURES[name]()
    lp = ref.loops(len(v), f)
    fl = ref.fill(v, f, lp, limit)
    w, g = ref.filled_mesh(v, f, lp, fl)
    return v, f, lp, fl, w, g


# ---- the two forms of the reference agree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_doubling_and_walking_find_the_same_loops(name):
    v, f, lp, _, _, _ = _case(name)
    walked = ref.loops(len(v), f, walk=True)
    for key in ("half_edge_loop", "loop_offsets", "loop_half_edges"):
        assert np.array_equal(lp[key], walked[key]) and lp[key].dtype == np.int32, key
    assert lp["counts"] == walked["counts"]
    # the shape of the outputs: every member on its loop, heads ascending and smallest, the members chained tail to head
    n, total = lp["num_loops"], lp["num_members"]
    F = len(f)
    assert lp["half_edge_loop"].shape == (3 * F,) and lp["loop_offsets"].shape == (F + 1,) and lp["loop_half_edges"].shape == (3 * F,)
    assert (lp["loop_offsets"][n:] == total).all() and (lp["loop_half_edges"][total:] == -1).all()
    assert (lp["half_edge_loop"] >= 0).sum() == total == lp["counts"][1] and n == lp["counts"][2]
    heads = lp["loop_half_edges"][lp["loop_offsets"][:n]]
    assert (np.diff(heads) > 0).all()
    flat, nxt = np.asarray(f).reshape(-1), np.asarray(f)[:, [1, 2, 0]].reshape(-1)
    for i in range(n):
        m = lp["loop_half_edges"][lp["loop_offsets"][i]:lp["loop_offsets"][i + 1]]
        assert len(m) >= 3 and m[0] == m.min() and (lp["half_edge_loop"][m] == i).all()
        assert np.array_equal(nxt[m], flat[np.roll(m, -1)])          # every member's head is the next member's tail
        assert len(set(flat[m].tolist())) == len(m)                 # a simple cycle


def test_a_random_soup_with_a_foreign_table_agrees_too():
    rng = np.random.default_rng(5)
    V = 300
    f = rng.integers(0, V, (600, 3))
    f[:5, 0], f[5:9, 1] = -1, V
    table = ref.table_of(V, f)
    short = (table[0], table[1], table[2], table[3] // 2)  # a foreign table: rows cut at half the entries
    for t in (table, short):
        a, b = ref.loops(V, f, table=t), ref.loops(V, f, table=t, walk=True)
        assert all(np.array_equal(a[k], b[k]) for k in ("half_edge_loop", "loop_offsets", "loop_half_edges")) and a["counts"] == b["counts"]
    assert ref.loops(V, f, table=short)["counts"][0] < ref.loops(V, f, table=table)["counts"][0]


# ---- the figures of DESIGN.md 16k -----------------------------------------------------------------------------------------------------------------
def test_punched_sphere_closes_to_the_figures_of_the_table():
    v, f, lp, fl, w, g = _case("punched")
    before, after = ref_volume.topology(f), ref_volume.topology(g)
    lengths = sorted(ref.loop_lengths(lp).tolist())
    volume = [fixtures.signed_volume(v, f), fixtures.signed_volume(w, g), fixtures.signed_volume(*fixtures.sphere_mesh())]
    print(f"punched sphere: {before['boundary']} boundary edges, Euler {before['euler']}, volume {volume[0]:.2f}; loops {lengths}; "
          f"filled: {after['boundary']} boundary, {after['nonmanifold']} non-manifold, {after['directed_repeats']} directed repeats, Euler "
          f"{after['euler']}, volume {volume[1]:.2f} (clean {volume[2]:.2f}); added {fl['totals'][1]} vertices, {fl['totals'][2]} faces")
    assert (before["boundary"], before["nonmanifold"], before["euler"]) == (108, 0, -15)
    assert (after["boundary"], after["nonmanifold"], after["directed_repeats"], after["euler"]) == (0, 0, 0, 2)
    assert lp["counts"] == [108, 108, 17, 0]  # all 108 half-edges on loops, no non-simple vertex
    assert len(lengths) == 17 and lengths[0] == 3 and lengths[-1] == 12 and lengths.count(3) == 5
    assert fl["totals"] == [17, 12, 98] and (fl["loop_status"] == ref.FILLED).all()
    assert abs(volume[0] - 3298.18) < 0.005 and abs(volume[1] - 3349.67) < 0.005 and abs(volume[2] - 3349.80) < 0.005
    # max_loop_edges = 8: 13 loops are filled, 48 boundary edges are left
    _, _, _, fl8, _, g8 = _case("punched", 8)
    assert fl8["totals"][0] == 13 and np.bincount(fl8["loop_status"], minlength=4).tolist() == [13, 4, 0, 0]
    assert ref_volume.topology(g8)["boundary"] == 48


@pytest.mark.parametrize("name,loops,euler_before", [("capped", [116], 1), ("plane", [96], 1), ("fused", [38] * 12, -10), ("nan_blocks", [46, 52], 0)])
def test_other_fixtures_close(name, loops, euler_before):
    v, f, lp, fl, w, g = _case(name)
    before, after = ref_volume.topology(f), ref_volume.topology(g)
    assert sorted(ref.loop_lengths(lp).tolist()) == loops and lp["counts"] == [sum(loops), sum(loops), len(loops), 0]
    assert before["boundary"] == sum(loops) and before["euler"] == euler_before
    assert (after["boundary"], after["nonmanifold"], after["directed_repeats"], after["euler"]) == (0, 0, 0, 2)
    assert fl["totals"] == [len(loops), len(loops), sum(loops)]
    if name == "plane":  # a closed pillow of signed volume 0 up to rounding: this is why max_loop_edges exists
        volume = fixtures.signed_volume(w, g)
        scale = np.abs(w.astype(np.float64)).max() ** 3
        print(f"plane pillow: signed volume {volume:.3e} against a coordinate scale of {scale:.1f}")
        assert abs(volume) < 1e-5 * scale  # fp32 vertices on a plane: 2^-24 relative per coordinate, 96 + 1152 faces
    if name == "fused":  # max_loop_edges = 32: nothing is filled
        _, _, _, fl32, _, g32 = _case("fused", 32)
        assert fl32["totals"] == [0, 0, 0] and (fl32["loop_status"] == ref.TOO_LONG).all() and len(g32) == len(f)
        assert (fl32["new_faces"] == -1).all() and (fl32["new_face_loop"] == -1).all() and not fl32["new_vertices"].any()


def test_lone_triangle_pinch_and_closed_mesh():
    v, f, lp, fl, w, g = _case("lone")
    assert lp["counts"] == [3, 3, 1, 0] and fl["loop_status"].tolist() == [ref.LONE_FACE] and fl["totals"] == [0, 0, 0] and len(g) == 1
    v, f, lp, fl, w, g = _case("pinched")
    assert lp["counts"] == [6, 0, 0, 1] and lp["num_loops"] == 0 and (lp["half_edge_loop"] == -1).all()  # 6 boundary, all open, 1 non-simple
    assert fl["totals"] == [0, 0, 0] and len(g) == len(f)
    v, f, lp, fl, w, g = _case("closed")
    assert lp["counts"] == [0, 0, 0, 0] and not lp["loop_offsets"].any()


def test_fans_run_against_the_boundary_and_centroids_are_the_sequential_mean():
    v, f, lp, fl, w, g = _case("bands")
    assert sorted(ref.loop_lengths(lp).tolist()) == [3, 3, 4, 4, 5, 5, 17, 17]
    assert np.bincount(fl["loop_status"], minlength=4).tolist() == [8, 0, 0, 0] and fl["totals"] == [8, 6, 2 + 2 * (4 + 5 + 17)]
    assert ref_volume.topology(g)["boundary"] == 0 and ref_volume.topology(g)["directed_repeats"] == 0
    flat = f.reshape(-1)
    at = 0
    for i, L in enumerate(ref.loop_lengths(lp)):
        tails = flat[lp["loop_half_edges"][lp["loop_offsets"][i]:lp["loop_offsets"][i + 1]]]
        if L == 3:
            assert fl["new_faces"][at].tolist() == [tails[0], tails[2], tails[1]]
            at += 1
            continue
        c = fl["new_faces"][at, 2]
        assert np.array_equal(fl["new_faces"][at:at + L], np.stack([np.roll(tails, -1), tails, np.full(L, c)], 1))
        assert (fl["new_face_loop"][at:at + L] == i).all()
        s = np.zeros(3)
        for t in tails:
            s = s + v[t].astype(np.float64)
        assert np.array_equal(w[c], (s / float(L)).astype(np.float32))
        at += L
    assert at == fl["totals"][2] and (fl["new_faces"][at:] == -1).all()


def test_dead_loops_and_the_attribute_rule():
    v, f, lp, _, _, _ = _case("bands")
    flat = f.reshape(-1)
    tails = [flat[lp["loop_half_edges"][lp["loop_offsets"][i]:lp["loop_offsets"][i + 1]]] for i in range(lp["num_loops"])]
    long_ones = [i for i, t in enumerate(tails) if len(t) > 3]
    w = v.copy()
    w[tails[long_ones[0]][1], 1] = np.nan
    w[tails[0][0], 2] = np.inf if len(tails[0]) == 3 else w[tails[0][0], 2]
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    valid = np.ones(len(v), np.uint8)
    valid[tails[long_ones[1]]] = 0          # a loop none of whose members has a valid attribute
    valid[tails[long_ones[2]][::2]] = 0     # a loop where some have
    fl = ref.fill(w, f, lp, attributes=a, attr_valid=valid)
    assert fl["loop_status"][long_ones[0]] == ref.DEAD and (fl["loop_status"] == ref.DEAD).sum() == (2 if len(tails[0]) == 3 else 1)
    order = [i for i in long_ones if fl["loop_status"][i] == ref.FILLED]  # the new vertices, in ascending loop
    assert fl["totals"][1] == len(order)
    j = order.index(long_ones[1])
    assert fl["new_attr_valid"][j] == 0 and not fl["new_attributes"][j].any()
    j = order.index(long_ones[2])
    who = tails[long_ones[2]][1::2]
    s = np.zeros(3)
    for t in who:
        s = s + a[t].astype(np.float64)
    assert fl["new_attr_valid"][j] == 1 and np.array_equal(fl["new_attributes"][j], (s / float(len(who))).astype(np.float32))
    assert not fl["new_attributes"][len(order):].any() and not fl["new_attr_valid"][len(order):].any()
    everyone = ref.fill(v, f, lp, attributes=a)  # no valid bytes: all members count
    assert everyone["new_attr_valid"][:everyone["totals"][1]].all()


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(holes_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsh_last_error.restype = ctypes.c_char_p; "
            "l.tsh_workspace_bytes.restype = ctypes.c_size_t; print(l.tsh_workspace_bytes(100000, 200000) >= 32 * 3 * 200000, "
            "repr(l.tsh_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, holes_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "True"


def test_library_exports_exactly_the_header(holes_path):
    out = subprocess.run(["nm", "-D", "--defined-only", holes_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES and len(NAMES) == 4
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", holes_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower()
    dynamic = subprocess.run(["readelf", "-d", holes_path], capture_output=True, text=True).stdout
    assert "libts_holes.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so", "libts_color.so", "libts_simplify.so",
                  "libts_smooth.so"):
        assert other not in dynamic


def test_header_defines_no_struct_and_states_the_contract():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv|tsc|tsq|tss)_[a-z0-9_]+)\s*\(", text)  # a prefix of its own
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("-ffp-contract=off", "ONE thread per loop", "serial", "pointer doubling", "Wyllie", "SIMPLE", "OPEN", "pinch",
                 "stated, not fixed", "nobody waits for anybody", "TSH_TOO_LONG", "TSH_LONE_FACE", "TSH_DEAD", "a foreign table stays in bounds",
                 "against the boundary", "357913941"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(HOLES_SIGNATURES) and len(declared) == 4
    for name, arity in declared.items():
        assert len(HOLES_SIGNATURES[name][1]) == arity, name
    assert declared["tsh_loops"] == 15 and declared["tsh_fill"] == 22
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES,
              abi.COLOR_SIGNATURES, abi.SIMPLIFY_SIGNATURES, abi.SMOOTH_SIGNATURES, abi.HOLES_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert HOLES_SIGNATURES["tsh_loops"][1][13] == ctypes.c_size_t and HOLES_SIGNATURES["tsh_fill"][1][20] == ctypes.c_size_t
    assert HOLES_SIGNATURES["tsh_workspace_bytes"][0] == ctypes.c_size_t


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_holes", ("build.py",))
    assert build.HOLES_SOURCES == {"mesh_holes.hip": ["-ffp-contract=off"], "api_holes.hip": []}
    assert build.holes_units() == ["mesh_holes", "api_holes"] and not hasattr(build, "HOLES_SHARED")
    cmd = build.holes_command("mesh_holes", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert "-ffp-contract=off" not in build.holes_command("api_holes", cc="hipcc")
    assert build.holes_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("mesh_holes", "api_holes")]
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units(), build.color_units(),
                   build.simplify_units(), build.smooth_units()):
        assert not {"mesh_holes", "api_holes"} & set(others)  # its own library only
    assert build.HOLES_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_holes.so")
    for header in ("ts_holes_launch.h", os.path.join("..", "..", "include", "ts_holes.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.holes_command("mesh_smooth")


def test_built_objects_carry_the_flags(holes_path):
    build = _load("ts2d_build_holes2", ("build.py",))
    stamp = open(os.path.join(build.OBJ_DIR, "mesh_holes.o.cmd")).read()  # what the object on disk was compiled with
    assert stamp.endswith(" ".join(build.holes_command("mesh_holes", cc=stamp.splitlines()[1].split()[0]))) and "-ffp-contract=off" in stamp
    stamp = open(os.path.join(build.OBJ_DIR, "api_holes.o.cmd")).read()
    assert stamp.endswith(" ".join(build.holes_command("api_holes", cc=stamp.splitlines()[1].split()[0]))) and "-ffp-contract=off" not in stamp
    link = open(build.HOLES_LIB + ".cmd").read()
    assert "-soname,libts_holes.so" in link and "radix_sort" not in link


def test_size_query_is_monotone_in_both_counts(lib):
    sizes = (0, 1, 2, 63, 682, 683, 1024, 1025, 4097, 100000, 416666, 416667, 2499999, 2500000, 2500001, 2600000, 5000000)
    for fixed in (0, 1000, 3000000):
        prev_v = prev_f = -1
        for n in sizes:
            by_v, by_f = lib.tsh_workspace_bytes(n, fixed), lib.tsh_workspace_bytes(fixed, n)
            assert by_v >= prev_v and by_f >= prev_f, (n, fixed)
            assert by_v >= 12 * n and by_f >= 32 * 3 * n  # the census; succ, lab, two 8-byte states and the two scanned columns per half-edge
            prev_v, prev_f = by_v, by_f
    assert lib.tsh_workspace_bytes(-5, -5) == lib.tsh_workspace_bytes(0, 0)
    assert lib.tsh_workspace_bytes(10, 2 ** 31 - 1) == lib.tsh_workspace_bytes(10, 357913941)


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    big = 1 << 40

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsh_last_error()
        assert text and word.encode() in text, text

    def loops(V=10, F=20, faces=P, keep=None, offsets=P, neighbors=P, edge_faces=P, entries=60, hel=P, off=P, lhe=P, counts=P, ws=P, ws_bytes=big):
        return lib.tsh_loops(V, F, faces, keep, offsets, neighbors, edge_faces, entries, hel, off, lhe, counts, ws, ws_bytes, None)

    def fill(V=10, F=20, vertices=P, faces=P, num_loops=2, off=P, lhe=P, members=8, limit=64, attrs=None, valid=None, channels=0, status=P,
             new_v=P, new_a=None, new_valid=None, new_f=P, new_fl=P, totals=P, ws=P, ws_bytes=big):
        return lib.tsh_fill(V, F, vertices, faces, num_loops, off, lhe, members, limit, attrs, valid, channels, status, new_v, new_a, new_valid,
                            new_f, new_fl, totals, ws, ws_bytes, None)

    for call in (loops, fill):
        refused(call(V=-1), ">= 0")
        refused(call(V=-(2 ** 31)), ">= 0")
        refused(call(F=-1), ">= 0")
        refused(call(F=357913942), "exceeds", CAPACITY)
        refused(call(ws=None), "workspace is null")
    refused(loops(entries=-1), "num_entries")
    for name in ("counts", "off", "hel", "lhe", "faces", "offsets", "neighbors", "edge_faces"):
        refused(loops(**{name: None}), "null")
    for bad in (-1, -(2 ** 31)):
        refused(fill(limit=bad), "max_loop_edges")
        refused(fill(num_loops=bad), ">= 0")
        refused(fill(members=bad), ">= 0")
        refused(fill(channels=bad), ">= 0")
    refused(fill(num_loops=21), "exceed")
    refused(fill(members=61), "exceed")
    for name in ("totals", "new_f", "new_fl", "off", "status", "new_v", "lhe", "faces", "vertices"):
        refused(fill(**{name: None}), "null")
    for kw in (dict(channels=3, attrs=None, new_a=P, new_valid=P), dict(channels=3, attrs=P, new_a=None, new_valid=P),
               dict(channels=3, attrs=P, new_a=P, new_valid=None)):
        refused(fill(**kw), "attributes")
    need = lib.tsh_workspace_bytes(1000, 2000)
    refused(loops(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    assert str(need).encode() in lib.tsh_last_error()
    refused(fill(V=1000, F=2000, ws_bytes=need - 1), "workspace too small")
    # what the checks accept, for the record: neighbors / edge_faces may be null with num_entries == 0, attr_valid may be null, 0 and
    # 2^31 - 1 are both max_loop_edges (those calls would reach the device, so they are made in tests/test_mesh_holes_gpu.py)


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, holes_path):
    """Without libts_holes.so, diff_recon_hip.mesh_holes raises and names the build command; everything else still imports."""
    src = os.path.dirname(holes_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or (name.endswith(".so") and name != "libts_holes.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.smooth_mesh), callable(diff_recon_hip.simplify_mesh))\n"
            "try:\n    diff_recon_hip.fill_holes\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.mesh_holes\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_holes.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_holes.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature_and_keeps_the_pinned_parameter_lists(holes_path):
    import inspect

    import diff_recon_hip
    from diff_recon_hip import color_volume, mesh_holes, mesh_simplify, mesh_smooth, volume
    names = ("BoundaryLoops", "FilledMesh", "boundary_loops", "loop_vertices", "fill_holes", "fill_fused")
    assert diff_recon_hip._HOLES_NAMES == names
    for name in names:
        assert getattr(diff_recon_hip, name) is getattr(mesh_holes, name)
    assert diff_recon_hip.mesh_holes is mesh_holes
    params = lambda fn: list(inspect.signature(fn).parameters)
    assert params(mesh_holes.boundary_loops) == ["num_vertices", "faces", "keep", "adjacency"]
    assert params(mesh_holes.loop_vertices) == ["loops", "faces"]
    assert params(mesh_holes.fill_holes) == ["vertices", "faces", "max_loop_edges", "vertex_attributes", "attribute_valid", "keep", "loops"]
    defaults = {k: p.default for k, p in inspect.signature(mesh_holes.fill_holes).parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"max_loop_edges": None, "vertex_attributes": None, "attribute_valid": None, "keep": None, "loops": None}
    assert params(mesh_holes.fill_fused) == ["mesh", "max_loop_edges"]
    assert mesh_holes.BoundaryLoops._fields == ("half_edge_loop", "loop_offsets", "loop_half_edges", "stats")
    assert mesh_holes.FilledMesh._fields == ("vertices", "faces", "vertex_attributes", "attribute_valid", "new_vertex", "face_loop", "loop_status",
                                             "loops", "stats")
    assert mesh_holes.LOOP_STATUS == ref.STATUS
    # the neighbours keep their parameter lists
    assert params(mesh_simplify.simplify_fused) == ["mesh", "volume", "simplify_cell", "min_piece_faces"]
    assert params(mesh_smooth.smooth_fused) == ["mesh", "volume", "iterations", "max_move_voxels", "kw"]
    assert params(volume.fuse_mesh)[:4] == ["views", "vertices", "faces", "resolution"]
    assert params(color_volume.fuse_colored_mesh)[:5] == ["views", "vertices", "faces", "faces_color", "resolution"]
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_holes.boundary_loops(4, torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_holes.fill_holes(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="max_loop_edges"):
        mesh_holes.fill_holes(torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32), max_loop_edges=-1)
    with pytest.raises(ValueError, match="num_vertices"):
        mesh_holes.boundary_loops(-1, torch.zeros((2, 3), dtype=torch.int32))


def test_example_refuses_fill_holes_without_extract_mesh():
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--fill-holes", "16"], capture_output=True, text=True)
    assert r.returncode == 2 and "--fill-holes fills the holes of the mesh of --extract-mesh" in r.stderr
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--extract-mesh", "24", "--fill-holes", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--fill-holes needs a number of edges >= 0" in r.stderr
