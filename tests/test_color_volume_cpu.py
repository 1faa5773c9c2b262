"""CPU tests of the colour volume (no GPU): the numpy reference keeps the promises of include/ts_color.h (order-independent integer sums,
a sampler that is a function of position alone), the reference pipeline colours every vertex of the fused sphere, libts_color.so is a library
of its own with exactly the C ABI of the header, and every argument check answers before any HIP call."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_color_volume as cref
import ref_volume as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ts_color.h")
INVALID, CAPACITY = 1, 3  # TS2D_ERR_INVALID, TS2D_ERR_CAPACITY
NAMES = ["tsc_color_field", "tsc_integrate", "tsc_interpolate", "tsc_last_error", "tsc_sample"]
COLOR_ERROR_BOUND = 0.05  # measured below on the reference (0.0462), rounded up to one significant digit


def _load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "triangle-splatting_amd", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _abi_module():
    """diff_triangle_rasterization_2D/_abi.py by path: pure ctypes, so it loads before anything is built."""
    return _load("ts2d_abi_color", ("diff_triangle_rasterization_2D", "_abi.py"))


COLOR_SIGNATURES = _abi_module().COLOR_SIGNATURES  # the feature's ctypes table: without it nothing below means anything


@pytest.fixture(scope="module")
def color_path(hip_lib_built):
    path = os.path.join(ROOT, "triangle-splatting_amd", "diff_recon_hip", "libts_color.so")
    assert os.path.exists(path), "build.py's default build() did not produce libts_color.so"
    return path


@pytest.fixture(scope="module")
def lib(color_path):
    from diff_triangle_rasterization_2D import _abi
    return _abi.bind_color(ctypes.CDLL(color_path))


def _header_prototypes():
    """name -> number of parameters of every tsc_ prototype of the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = {}
    for name, params in re.findall(r"\b(tsc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, name
        found[name] = 0 if params.strip() == "void" else len(params.split(","))
    return found


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the reference: integration ----------------------------------------------------------------------------------------------------------------
DIMS, ORIGIN, H, TRUNC = (4, 3, 2), (-0.2, -0.1, -0.05), 0.1, 0.4
VIEW = ref.look_at_view((0, 0, -3))


def _integrate(depth, image, cs=None, cw=None, mask=None):
    n = DIMS[0] * DIMS[1] * DIMS[2]
    cs = np.zeros((n, 3), np.int64) if cs is None else cs
    cw = np.zeros(n, np.int32) if cw is None else cw
    count = cref.integrate(cs, cw, DIMS, ORIGIN, H, TRUNC, VIEW, 0.45, 0.45, 8, 8, depth, image, mask)
    return count, cs, cw


def test_integrate_colours_what_the_header_says():
    n = 24
    depth = np.full((8, 8), 3.0, np.float32)
    image = np.stack([np.full((8, 8), v, np.float32) for v in (0.25, 1.5, -0.5)])
    count, cs, cw = _integrate(depth, image)
    assert count == n and (cw == 1).all()
    assert (cs[:, 0] == 16384).all() and (cs[:, 1] == 65536).all() and (cs[:, 2] == 0).all()  # Q16, clamped to [0, 1]
    for bad in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):  # an uncovered or unusable pixel colours nothing
        assert _integrate(np.full((8, 8), bad, np.float32), image)[0] == 0
    for bad in (np.nan, np.inf, -np.inf):  # one bad channel drops the pixel
        for ch in range(3):
            im = image.copy()
            im[ch] = bad
            assert _integrate(depth, im)[0] == 0
    assert _integrate(np.full((8, 8), 2.0, np.float32), image)[0] == 0  # behind the surface: sd < -trunc
    assert _integrate(np.full((8, 8), 4.0, np.float32), image)[0] == 0  # far in front: sd > trunc, where the distance is clipped
    assert _integrate(depth, image, mask=np.zeros((8, 8), np.uint8))[0] == 0
    cw0 = np.zeros(n, np.int32)
    cw0[:5] = cref.INT32_MAX
    count, cs, cw = _integrate(depth, image, cw=cw0)
    assert count == n - 5 and (cw[:5] == cref.INT32_MAX).all() and (cs[:5] == 0).all()
    f = cref.color_field(np.array([[1 << 15, 3 << 16, 0], [5, 5, 5], [0, 0, 0]], np.int64), np.array([1, 4, 0], np.int32), 2)
    assert f.shape == (3, 3) and np.isnan(f[:, 0]).all() and np.isnan(f[:, 2]).all() and f[1, 1] == np.float32(5 / (4 * 65536.0))
    assert (_bits(f[:, 0]) == 0x7FC00000).all()


def test_integration_is_order_independent_and_volumes_add():
    a = cref.fuse_colored_sphere()
    b = cref.fuse_colored_sphere(order=(5, 3, 1, 4, 2, 0))
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    first, rest = cref.fuse_colored_sphere(order=(0, 1)), cref.fuse_colored_sphere(order=(2, 3, 4, 5))
    for k in range(4):
        assert np.array_equal(first[k] + rest[k], a[k])
    s, w = ref.fuse_sphere(carve=True)[:2]
    assert np.array_equal(a[0], s) and np.array_equal(a[1], w)  # the distances are ref_volume's
    assert (a[3] > 0).any() and (a[3] == 0).any() and a[3].max() <= 6


# ---- the reference: sampler ----------------------------------------------------------------------------------------------------------------------
def _lattice(dims, origin, h):
    (p0, p1, p2), _ = ref.sample_positions(dims, origin, h)
    return np.stack([p0, p1, p2], axis=1).astype(np.float32)


def test_sampler_at_a_lattice_point_returns_the_sample():
    """Power-of-two origin and spacing, so that the fp32 lattice positions are exact and g is an integer."""
    dims, origin, h = (6, 5, 4), (-1.5, 0.25, 2.0), 0.125
    rng = np.random.default_rng(3)
    grid = rng.normal(0, 1, (3, 120)).astype(np.float32)
    grid[:, rng.integers(0, 120, 15)] = np.nan
    grid[1, rng.integers(0, 120, 5)] = np.inf  # one bad channel: the sample has no data
    pts = _lattice(dims, origin, h)
    out, valid = cref.sample(grid, dims, origin, h, pts)
    has = np.isfinite(grid).all(axis=0)
    assert np.array_equal(valid.astype(bool), has) and has.any() and not has.all()
    assert np.array_equal(_bits(out[has]), _bits(grid.T[has]))
    assert (_bits(out[~has]) == 0x7FC00000).all()


def test_sampler_uses_the_last_cell_on_the_upper_face_and_refuses_outside():
    dims, origin, h = (3, 3, 3), (0.0, 0.0, 0.0), 1.0
    grid = np.arange(27, dtype=np.float32)  # f = i + 3 j + 9 k: trilinear reproduces it
    pts = np.array([[2, 2, 2], [2, 0.5, 1.25], [0.5, 2, 2], [1.5, 1.5, 1.5], [2.0000002, 1, 1], [-1e-7, 1, 1], [np.nan, 1, 1], [1, np.inf, 1],
                    [1, 1, -np.inf]], np.float32)
    out, valid = cref.sample(grid, dims, origin, h, pts)
    assert valid.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert out[:4, 0].tolist() == [26.0, 2 + 1.5 + 11.25, 0.5 + 6 + 18, 1.5 * 13]
    assert np.isnan(out[4:]).all()
    lonely = np.full(27, np.nan, np.float32)
    lonely[13] = 7.0  # only the centre sample has data
    out, valid = cref.sample(lonely, dims, origin, h, np.array([[0.5, 0.5, 0.5], [1, 1, 1], [0, 1, 1], [0.25, 1, 1], [0, 0, 0]], np.float32))
    assert valid.tolist() == [1, 1, 0, 1, 0] and out[[0, 1, 3], 0].tolist() == [7.0, 7.0, 7.0]  # renormalised; a weight-0 corner alone is no data


def test_sampler_works_with_a_dimension_of_one():
    dims, origin, h = (5, 1, 4), (0.5, -2.0, 1.0), 0.5
    grid = np.stack([np.arange(20, dtype=np.float32), -np.arange(20, dtype=np.float32)])
    pts = np.array([[0.5, -2, 1], [2.5, -2, 2.5], [1.25, -2, 1.75], [1, -1.999, 1], [1, -2.001, 1]], np.float32)
    out, valid = cref.sample(grid, dims, origin, h, pts)
    assert valid.tolist() == [1, 1, 1, 0, 0]
    assert out[:3, 0].tolist() == [0.0, 19.0, 1.5 + 5 * 1.5] and np.array_equal(out[:3, 1], -out[:3, 0])
    one = cref.sample(np.array([3.5], np.float32), (1, 1, 1), (1, 2, 3), 0.3, np.array([[1, 2, 3], [1, 2, 3.1]], np.float32))
    assert one[1].tolist() == [1, 0] and one[0][0, 0] == 3.5


def test_sampling_the_field_at_the_extracted_vertices_gives_the_level():
    """The sampler and the extraction agree on where the level set is.  The bound, derived here:
    a vertex on an edge (a, b) of the marching tetrahedra sits at g = ga + t (gb - ga) in grid units and is written as fl32(o + h g): its
    position moves by at most half an fp32 ulp, 2^-24 max|world|, per axis, that is dg = 2^-24 max|world| / h grid units (plus float64
    noise).  The sampled value is a convex combination of the eight corners, so it moves by at most R = max f - min f per grid unit and axis.
    On an axis-aligned edge the trilinear field is linear in t and equals iso at g, so |sample - iso| <= 3 R dg, plus the fp32 rounding of
    the result, 2^-24 max|f|, and float64 noise of a few 2^-53 R.  On a face or body diagonal the trilinear field is not linear along the
    edge; there convexity is what holds: the sample and iso both lie between the smallest and the largest corner of the cell (iso between
    the edge's two endpoints), so |sample - iso| <= D, the field's largest range over one cell, plus the same rounding terms."""
    dims, origin, h, iso = (9, 8, 7), (0.1, -0.7, 3.3), 0.3, 0.05
    f = ref.sphere_field(dims, (3.9, 3.4, 2.8), 2.3)
    tri, _ = ref.extract(f, dims, origin, h, iso=iso)
    pts = tri.reshape(-1, 3)
    out, valid = cref.sample(f, dims, origin, h, pts)
    assert len(pts) > 300 and valid.all()
    R = float(f.max()) - float(f.min())
    dg = 2.0 ** -24 * float(np.abs(pts).max()) / float(np.float32(h)) + 1e-12
    tight = 3.0 * R * dg + 2.0 ** -24 * float(np.abs(f).max()) + 16 * 2.0 ** -53 * R
    g = (pts.astype(np.float64) - np.asarray(origin, np.float32).astype(np.float64)) / float(np.float32(h))
    on_lattice = np.abs(g - np.rint(g)) <= dg
    axis_edge = on_lattice.sum(axis=1) >= 2  # two coordinates on the lattice: an axis-aligned edge
    err = np.abs(out[:, 0].astype(np.float64) - float(np.float32(iso)))
    vol = f.reshape(dims[::-1])
    corners = np.stack([vol[dz:dims[2] - 1 + dz, dy:dims[1] - 1 + dy, dx:dims[0] - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    D = float((corners.max(axis=0) - corners.min(axis=0)).max())
    print("axis-aligned", int(axis_edge.sum()), "max error", err[axis_edge].max(), "bound", tight, "| diagonal", int((~axis_edge).sum()), "max error",
          err[~axis_edge].max(), "bound", D + tight)
    assert axis_edge.sum() > 100 and (~axis_edge).sum() > 100 and D < R / 2
    assert err[axis_edge].max() <= tight
    assert err[~axis_edge].max() <= D + tight


# ---- the reference pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_sphere():
    s, w, cs, cw, dims, origin, h = cref.fuse_colored_sphere()
    tri, _ = ref.extract(ref.field(s, w), dims, origin, h)
    verts, faces = ref.weld_exact(tri)
    colour, valid = cref.sample(cref.color_field(cs, cw), dims, origin, h, verts)
    return dict(s=s, w=w, cs=cs, cw=cw, dims=dims, origin=origin, h=h, tri=tri, verts=verts, faces=faces, colour=colour, valid=valid)


def test_every_vertex_of_the_fused_sphere_is_coloured(fused_sphere):
    """A vertex is coloured iff a corner of its cell with positive weight carries colour; the crossed edge's inside endpoint lies within trunc
    behind the surface of at least one of the six views on this input."""
    m = fused_sphere
    assert len(m["verts"]) > 500 and m["valid"].all()
    assert np.isfinite(m["colour"]).all() and m["colour"].min() >= 0.0 and m["colour"].max() <= 1.0
    topo = ref.topology(m["faces"])
    assert topo["boundary"] == 0 and topo["euler"] == 2
    soup_colour, soup_valid = cref.sample(cref.color_field(m["cs"], m["cw"]), m["dims"], m["origin"], m["h"], m["tri"].reshape(-1, 3))
    _, inverse = np.unique(m["tri"].reshape(-1, 3) + np.float32(0.0), axis=0, return_inverse=True)
    assert soup_valid.all() and np.array_equal(_bits(soup_colour), _bits(m["colour"][inverse.reshape(-1)]))  # a function of position alone


def test_colour_error_of_the_fused_sphere_is_what_the_method_gives(fused_sphere):
    m = fused_sphere
    want = cref.sphere_color(m["verts"])
    err = np.abs(m["colour"].astype(np.float64) - want)
    print("largest colour error", err.max(), "mean", err.mean(), "vertices", len(want))
    assert err.max() <= COLOR_ERROR_BOUND
    assert err.max() > COLOR_ERROR_BOUND / 10  # the pin is one significant digit above the measurement, not a loose ceiling


# ---- the reference: interpolation ----------------------------------------------------------------------------------------------------------------
def test_interpolation_reproduces_a_linear_attribute_and_holds_the_weights_inside():
    view = ref.look_at_view((0.4, -0.3, -3.0))
    P = np.array([[-0.8, -0.6, 0.2], [0.9, -0.5, -0.3], [0.1, 0.8, 0.4], [5, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 0], [0, 1, 9]], np.int32)
    W, Hh = 16, 12
    fi = np.zeros((Hh, W), np.int32)
    fi[0, :4] = (-1, 3, -2 ** 31, 2)  # uncovered, F, INT32_MIN, a face with an index outside [0, V)
    fi[1] = 1
    attr = np.concatenate([P, np.ones((4, 1), np.float32)], axis=1)  # position and a constant
    out, bary = cref.interpolate(view, 0.45, 0.4, W, Hh, P, faces, fi, attr, np.array([9, 8, 7, 6], np.float32))
    assert (out[:, 0, :4] == np.array([9, 8, 7, 6], np.float32)[:, None]).all() and (bary[:, 0, :4] == 0).all()
    drawn = np.ones((Hh, W), bool)
    drawn[0, :4] = False
    assert (bary[:, drawn] >= 0).all() and np.abs(bary[:, drawn].astype(np.float64).sum(axis=0) - 1).max() <= 2 * 2.0 ** -23
    assert np.abs(out[3][drawn] - 1).max() <= 2.0 ** -22  # a constant attribute stays constant
    inside = (bary > 0).all(axis=0) & drawn
    assert inside.sum() > 20 and (~inside & drawn).sum() > 20  # pixels the face covers, and pixels held at its border (the clamp path)
    # inside the face the interpolated position lies on the pixel's ray
    M = view.astype(np.float64)
    hit = np.stack([out[k][inside] for k in range(3)], axis=1).astype(np.float64) @ M[:3, :3] + M[3, :3]
    rows, cols = np.nonzero(inside)
    assert np.abs(hit[:, 0] / hit[:, 2] - ((cols + 0.5) / (0.5 * W) - 1) * 0.45).max() < 1e-5
    assert np.abs(hit[:, 1] / hit[:, 2] - ((rows + 0.5) / (0.5 * Hh) - 1) * np.float32(0.4)).max() < 1e-5


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_loads_by_bare_cdll_in_a_fresh_process(color_path):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.tsc_last_error.restype = ctypes.c_char_p; "
            "print(l.tsc_color_field(0, 1, 1, None, None, 1, None, None), repr(l.tsc_last_error()))")
    r = subprocess.run([sys.executable, "-c", code, color_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[0] == "1" and ">= 1" in r.stdout


def test_library_exports_exactly_the_header(color_path):
    out = subprocess.run(["nm", "-D", "--defined-only", color_path], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))  # __hip_cuid_*: the toolchain's per-object markers
    assert sorted(_header_prototypes()) == NAMES
    assert ours == NAMES
    everything = subprocess.run(["nm", "-D", color_path], capture_output=True, text=True).stdout
    assert "rocprim" not in everything.lower() and "tsv_" not in everything
    dynamic = subprocess.run(["readelf", "-d", color_path], capture_output=True, text=True).stdout
    assert "libts_color.so" in dynamic
    for other in ("libts2d.so", "libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so"):
        assert other not in dynamic


def test_header_names_no_other_library_and_defines_no_struct():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert not re.findall(r"\b((?:ts2d|tsl|tsk|tsm|tso|tsg|tsb|tsr|tsv)_[a-z0-9_]+)\s*\(", text)
    assert "struct" not in text
    full = open(HEADER).read()
    for word in ("-ffp-contract=off", "INT32_MAX", "2^27", "0x7FC00000", "the first addend is assigned", "x1 y2 - x2 y1", "(r0 n0 + r1 n1) + n2",
                 "function of the point's position and the grid alone", "Purity", "caller-owned accumulators", "1.0 / 3.0"):
        assert word in full, word


def test_ctypes_table_matches_the_header_name_for_name_and_in_arity():
    declared = _header_prototypes()
    assert set(declared) == set(COLOR_SIGNATURES)
    for name, arity in declared.items():
        assert len(COLOR_SIGNATURES[name][1]) == arity, name
    assert declared["tsc_integrate"] == 20 and declared["tsc_sample"] == 14 and declared["tsc_interpolate"] == 16 and declared["tsc_color_field"] == 8
    abi = _abi_module()
    tables = [abi.SIGNATURES, abi.LAB_SIGNATURES, abi.GEOM_SIGNATURES, abi.BVH_SIGNATURES, abi.RAY_SIGNATURES, abi.VOLUME_SIGNATURES, abi.COLOR_SIGNATURES]
    for a in range(len(tables)):
        for b in range(a + 1, len(tables)):
            assert not set(tables[a]) & set(tables[b])  # no signature table overlaps another
    assert COLOR_SIGNATURES["tsc_integrate"][1][3:8] == [ctypes.c_float] * 5 and COLOR_SIGNATURES["tsc_sample"][1][3:7] == [ctypes.c_float] * 4


def test_build_tables_name_the_units_and_flags():
    build = _load("ts2d_build_color", ("build.py",))
    assert build.COLOR_SOURCES == {"color_volume.hip": ["-ffp-contract=off"], "api_color.hip": []}
    assert list(build.COLOR_SOURCES) == ["color_volume.hip", "api_color.hip"]
    assert build.color_units() == ["color_volume", "api_color"]
    cmd = build.color_command("color_volume", cc="hipcc")
    assert cmd[:1 + len(build.COMMON)] == ["hipcc", *build.COMMON] and "-ffp-contract=off" in cmd and "-fvisibility=hidden" in cmd
    assert build.color_objects() == [os.path.join(build.OBJ_DIR, n + ".o") for n in ("color_volume", "api_color")]  # no product object is reused
    for others in (build.units(), build.geom_units(), build.bvh_units(), build.ray_units(), build.volume_units()):
        assert not {"color_volume", "api_color"} & set(others)  # its own library only
    assert build.COLOR_LIB == os.path.join(build.HERE, "diff_recon_hip", "libts_color.so")
    for header in ("ts_color_launch.h", os.path.join("..", "..", "include", "ts_color.h")):
        assert header in build.HEADERS
    with pytest.raises(ValueError):
        build.color_command("volume")
    assert list(build.VOLUME_SOURCES) == ["volume.hip", "api_volume.hip"]  # the fifth library is left as it was


def test_built_objects_carry_the_flags(color_path):
    build = _load("ts2d_build_color2", ("build.py",))
    assert "-ffp-contract=off" in open(os.path.join(build.OBJ_DIR, "color_volume.o.cmd")).read()  # what the object on disk was compiled with
    assert "-soname,libts_color.so" in open(build.COLOR_LIB + ".cmd").read()


def test_the_projection_is_restated_word_for_word():
    """Steps 1-3 of the two integration kernels are the same text: the colour lands on the samples the distance landed on."""
    csrc = os.path.join(ROOT, "triangle-splatting_amd", "csrc")

    def projection(path):
        text = open(os.path.join(csrc, path)).read()
        return re.sub(r"\s+", " ", text[text.index("const int i = idx % nx"):text.index("const float d = depth[pix];")])

    assert projection("color_volume.hip") == projection("volume.hip")
    assert "mask[pix] != 0" in projection("volume.hip") and "floor(" in projection("volume.hip")


def test_argument_checks_answer_without_a_gpu(lib):
    P = 0x1000  # a non-null stand-in: an argument check never dereferences
    nan, inf = float("nan"), float("inf")

    def refused(rc, word, code=INVALID):
        assert rc == code, rc
        text = lib.tsc_last_error()
        assert text and word.encode() in text, text

    def integrate(nx=4, ny=4, nz=4, h=0.1, trunc=0.4, view=P, tx=0.5, ty=0.5, W=8, H=8, depth=P, mask=None, image=P, s=P, w=P, updated=None):
        return lib.tsc_integrate(nx, ny, nz, 0.0, 0.0, 0.0, h, trunc, view, tx, ty, W, H, depth, mask, image, s, w, updated, None)

    def field(nx=4, ny=4, nz=4, s=P, w=P, min_weight=1, out=P):
        return lib.tsc_color_field(nx, ny, nz, s, w, min_weight, out, None)

    def sample(nx=4, ny=4, nz=4, h=0.1, C=3, grid=P, N=5, points=P, out=P, valid=P):
        return lib.tsc_sample(nx, ny, nz, 0.0, 0.0, 0.0, h, C, grid, N, points, out, valid, None)

    def interpolate(view=P, tx=0.5, ty=0.5, W=8, H=8, V=4, vertices=P, F=2, faces=P, face_idx=P, C=3, attributes=P, background=P, out=P, bary=None):
        return lib.tsc_interpolate(view, tx, ty, W, H, V, vertices, F, faces, face_idx, C, attributes, background, out, bary, None)

    for call in (integrate, field, sample):
        for dims in ({"nx": 0}, {"ny": -1}, {"nz": 0}, {"nx": -(2 ** 31)}):
            refused(call(**dims), ">= 1")
        refused(call(nx=1 << 14, ny=1 << 13, nz=2), "2^27", CAPACITY)  # 2^28 samples
        refused(call(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), "2^27", CAPACITY)
        refused(call(nx=(1 << 27) + 1, ny=1, nz=1), "2^27", CAPACITY)
    for call in (integrate, sample):
        for bad in (0.0, -0.1, nan, inf, -inf):
            refused(call(h=bad), "h must be finite and > 0")
    for bad in (0.0, -1.0, nan, inf):
        refused(integrate(trunc=bad), "trunc must be finite and > 0")
        for call in (integrate, interpolate):
            refused(call(tx=bad), "tan_fovx")
            refused(call(ty=bad), "tan_fovy")
    for call in (integrate, interpolate):
        refused(call(W=0), "W and H")
        refused(call(H=-3), "W and H")
        refused(call(W=1 << 16, H=1 << 15), "2^31 - 1", CAPACITY)
    for name in ("view", "depth", "image", "s", "w"):
        refused(integrate(**{name: None}), "null")
    for name in ("s", "w", "out"):
        refused(field(**{name: None}), "null")
    refused(field(min_weight=0), "min_weight")
    refused(field(min_weight=-5), "min_weight")
    for call in (sample, interpolate):
        for bad in (0, 9, -1):
            refused(call(C=bad), "C must lie in [1, 8]")
    refused(sample(N=-1), "N must be >= 0")
    for name in ("grid", "points", "out", "valid"):
        refused(sample(**{name: None}), "null")
    assert sample(N=0, grid=None, points=None, out=None, valid=None) == 0  # a no-op
    refused(sample(N=0, C=0), "C must lie")  # ... after the checks of the scalars
    refused(interpolate(V=-1), "V and F")
    refused(interpolate(F=-1), "V and F")
    for name in ("view", "face_idx", "background", "out"):
        refused(interpolate(**{name: None}), "null")
    refused(interpolate(vertices=None), "null with V")
    refused(interpolate(attributes=None), "null with V")
    refused(interpolate(faces=None), "null with F")


def test_missing_library_is_an_import_error_and_the_package_still_imports(tmp_path, color_path):
    """Without libts_color.so, diff_recon_hip.color_volume raises and names the build command; everything else, the volume included, imports."""
    src = os.path.dirname(color_path)
    pkg = tmp_path / "diff_recon_hip"
    pkg.mkdir()
    for name in os.listdir(src):
        if name.endswith(".py") or name in ("libts_geom.so", "libts_bvh.so", "libts_ray.so", "libts_volume.so"):
            shutil.copy(os.path.join(src, name), pkg / name)
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(tmp_path), os.path.join(ROOT, "triangle-splatting_amd")])}
    code = ("import diff_recon_hip, sys\n"
            "assert str(diff_recon_hip.__file__).startswith(sys.argv[1]), diff_recon_hip.__file__\n"
            "print('others', callable(diff_recon_hip.weld_mesh), callable(diff_recon_hip.fuse_mesh), callable(diff_recon_hip.evaluate_vertex_colors))\n"
            "try:\n    diff_recon_hip.ColorTSDFVolume\nexcept ImportError as e:\n    print('lazy', e)\n"
            "import diff_recon_hip.color_volume\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, env=env)
    assert "others True True True" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "lazy" in r.stdout and "libts_color.so" in r.stdout
    assert r.returncode != 0 and "ImportError" in r.stderr
    assert "libts_color.so" in r.stderr and "no CPU fallback" in r.stderr and "triangle-splatting_amd/build.py" in r.stderr


def test_package_re_exports_the_feature(color_path):
    import inspect
    import diff_recon_hip
    from diff_recon_hip import color_volume, metrics, volume
    for name in ("ColorTSDFVolume", "ColoredMesh", "sample_grid", "interpolate_vertex_attributes", "render_vertex_colors", "fuse_colored_mesh",
                 "save_glb_mesh"):
        assert getattr(diff_recon_hip, name) is getattr(color_volume, name)
    assert diff_recon_hip.color_volume is color_volume and diff_recon_hip.evaluate_vertex_colors is metrics.evaluate_vertex_colors
    assert issubclass(color_volume.ColorTSDFVolume, volume.TSDFVolume)
    assert color_volume.ColoredMesh._fields == ("vertices", "faces", "vertex_color", "color_valid", "stats")
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(color_volume.ColorTSDFVolume.integrate)[1:7] == ["cam", "depth", "image", "mask", "carve_uncovered", "updated"]
    assert params(color_volume.ColorTSDFVolume.extract)[1:] == ["min_weight", "iso", "fill"]
    assert params(color_volume.sample_grid) == ["grid", "origin", "voxel_size", "points"]
    assert params(color_volume.interpolate_vertex_attributes) == ["cam", "vertices", "faces", "face_idx", "attributes", "background", "return_bary"]
    assert params(color_volume.render_vertex_colors) == ["cam", "vertices", "faces", "vertex_color", "bg_color"]
    assert params(metrics.evaluate_vertex_colors) == ["views", "vertices", "faces", "vertex_color", "bg_color"]
    assert params(color_volume.fuse_colored_mesh) == ["views", "vertices", "faces", "faces_color", "resolution", "trunc", "images", "return_volume"]
    assert params(volume.fuse_mesh)[:5] == ["views", "vertices", "faces", "resolution", "trunc"]  # the helper split left it alone
    assert params(metrics.evaluate_mesh) == ["views", "vertices", "faces", "faces_color", "bg_color"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        color_volume.ColorTSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, device="cpu")


def test_save_glb_mesh_round_trips_without_a_gpu(tmp_path, color_path):
    from diff_recon_hip import color_volume
    from diff_recon_hip.raw_triangle import _accessor, read_glb
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    colour = np.array([[0, 0.5, 1], [1.5, -1, 0.25], [np.nan, 1, 0], [0.2, 0.4, 0.6]], np.float32)
    path = tmp_path / "sub" / "mesh.glb"
    color_volume.save_glb_mesh(path, pos, faces, colour)
    doc, binary = read_glb(path)
    prim = doc["meshes"][0]["primitives"][0]
    assert np.array_equal(_accessor(doc, binary, prim["attributes"]["POSITION"]), pos)
    assert np.array_equal(_accessor(doc, binary, prim["indices"]).reshape(-1, 3), faces)
    acc = doc["accessors"][prim["attributes"]["COLOR_0"]]
    assert acc["componentType"] == 5121 and acc["type"] == "VEC4" and acc["normalized"] is True
    assert doc["accessors"][prim["indices"]]["componentType"] == 5125
    got = _accessor(doc, binary, prim["attributes"]["COLOR_0"])
    assert got.tolist() == [[0, 128, 255, 255], [255, 0, 64, 255], [0, 255, 0, 255], [51, 102, 153, 255]]


def test_example_refuses_extract_color_without_extract_mesh():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "--eval-mesh", "--extract-color"], capture_output=True,
                       text=True)
    assert r.returncode == 2 and "--extract-color" in r.stderr and "--extract-mesh" in r.stderr
