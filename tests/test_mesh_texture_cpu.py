"""CPU tests of the texture atlas (diff_recon_hip/mesh_texture.py, include/ts_atlas.h; no GPU): the integer layout of texels and cells, the
default atlas shape, the UVs under a NEAREST sampler, the reference against the census reference, the PNG and GLB writers, and the Python
errors that need no device."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import ref_mesh_census as cen
import ref_mesh_texture as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(hip_lib_built):
    from diff_recon_hip import mesh_texture
    return mesh_texture


@pytest.mark.parametrize("R", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("F", [0, 1, 2, 7])
def test_texels_map_one_to_one_onto_the_compact_range_and_the_half_cells(mt, R, F):
    lay = mt.atlas_layout(F, R)
    assert tuple(lay) == tref.layout(F, R)
    T = R * (R + 1) // 2
    ij = tref.face_texels(R)
    assert len(ij) == T == lay.texels_per_face
    f = np.repeat(np.arange(F, dtype=np.int64), T)
    i, j = np.tile(ij[:, 0], F), np.tile(ij[:, 1], F)
    n = tref.compact_index(f, i, j, R)
    assert np.array_equal(n, np.arange(F * T))  # in order, hence a bijection onto [0, F T)
    x, y = tref.texel_position(f, i, j, R, lay.cells_per_row)
    assert ((x >= 0) & (x < lay.width) & (y >= 0) & (y < lay.height)).all()
    flat = y * lay.width + x
    assert len(np.unique(flat)) == F * T  # no two texels share a position
    # ... and they are exactly the positions whose inverse names a face below F: the first F half-cells, each filled
    ys, xs = np.divmod(np.arange(lay.width * lay.height, dtype=np.int64), lay.width)
    f2, i2, j2 = tref.invert_position(xs, ys, R, lay.cells_per_row)
    assert np.array_equal(np.sort(flat), np.flatnonzero(f2 < F))
    assert np.array_equal(f2[flat], f) and np.array_equal(i2[flat], i) and np.array_equal(j2[flat], j)
    assert ((i2 >= 0) & (j2 >= 0) & (i2 + j2 <= R - 1)).all()
    if F == 7:  # a layout the caller chose: one row, and one column
        for Cx in (1, 4, 9):
            x, y = tref.texel_position(f, i, j, R, Cx)
            lay2 = mt.atlas_layout(F, R, Cx)
            assert lay2.cells_per_col == max(1, -(-4 // Cx)) and len(np.unique(y * lay2.width + x)) == F * T and x.max() < lay2.width and y.max() < lay2.height


@pytest.mark.parametrize("R", [1, 2, 3, 8, 64])
def test_the_default_atlas_is_the_smallest_near_square_one(mt, R):
    for F in (0, 1, 2, 3, 7, 8, 99, 1000, 12345, 2 * 10 ** 6 + 1):
        if F * (R * (R + 1) // 2) > 2 ** 31 - 1:
            continue
        lay = mt.atlas_layout(F, R)
        K, Cx = (F + 1) // 2, lay.cells_per_row
        assert Cx >= 1 and Cx * Cx * (R + 1) >= K * R and (Cx == 1 or (Cx - 1) * (Cx - 1) * (R + 1) < K * R)
        assert Cx == tref.default_cells_per_row(F, R) or F > 20000  # the reference counts up: only for small atlases
        assert lay.cells_per_col == max(1, -(-K // Cx)) and lay.width == Cx * (R + 1) and lay.height == lay.cells_per_col * R
        assert lay.cells_per_row * lay.cells_per_col >= K


@pytest.mark.parametrize("R,F,Cx", [(1, 8, None), (3, 7, None), (8, 7, 2), (8, 900, 455), (3, 2000, 1000), (1, 4096, 2048), (3, 1 + 2 * 1023 * 3, 1023)])
def test_uvs_hit_every_texel_under_a_nearest_sampler(mt, R, F, Cx):
    """The point of a face with barycentrics (1 - (i + j + 2/3) / R, (i + 1/3) / R, (j + 1/3) / R) -- the centroid of texel (i, j)'s own
    lower-left sub-triangle -- maps through the fp32 corner UVs, combined in float64, to floor(u Wa), floor(v Ha) = the texel's position:
    for every texel of a lower and of an upper face, in the first and in the last cell, in atlases up to 4096 texels wide."""
    lay = mt.atlas_layout(F, R, Cx)
    assert lay.width <= 4096
    uv = mt.face_uvs(lay, F)
    assert uv.dtype == torch.float32 and tuple(uv.shape) == (F, 3, 2)
    uv = uv.numpy()
    assert np.array_equal(uv.view(np.uint32), tref.face_uvs(F, R, lay.cells_per_row, lay.cells_per_col).view(np.uint32))
    ij = tref.face_texels(R)
    i, j = ij[:, 0].astype(np.float64), ij[:, 1].astype(np.float64)
    bary = np.stack([1.0 - (i + j + 2.0 / 3.0) / R, (i + 1.0 / 3.0) / R, (j + 1.0 / 3.0) / R], axis=1)  # (T, 3)
    for f in sorted({0, 1, F - 2, F - 1} & set(range(F))):  # a lower and an upper face of the first and of the last cell
        u = bary @ uv[f, :, 0].astype(np.float64)
        v = bary @ uv[f, :, 1].astype(np.float64)
        x, y = tref.texel_position(np.full(len(ij), f), ij[:, 0], ij[:, 1], R, lay.cells_per_row)
        assert np.array_equal(np.floor(u * lay.width).astype(np.int64), x), (f, R)
        assert np.array_equal(np.floor(v * lay.height).astype(np.int64), y), (f, R)
    assert (uv >= 0).all() and (uv <= 1).all()


def test_the_reference_with_one_texel_per_face_is_the_census_reference():
    rng = np.random.default_rng(3)
    F, H, W = 13, 9, 11
    key = rng.integers(-2, F + 2, (H, W)).astype(np.int32)
    target = rng.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    target[0, 0, :3] = np.nan
    mask = (rng.uniform(-1, 1, (H, W))).astype(np.float32)
    for tgt, m in ((None, None), (target, None), (target, mask)):
        acc = tref.accumulate(np.zeros((F * tref.texels_per_face(1), 4), np.int64), key, tgt, m)
        assert np.array_equal(acc, cen.census(F, key, tgt, m))
        assert np.array_equal(tref.face_totals(acc, F, 1), acc)
    # and with more texels the face totals are the census of the faces
    R = 3
    T = tref.texels_per_face(R)
    texel = np.where((key >= 0) & (key < F), key.astype(np.int64) * T + rng.integers(0, T, (H, W)), -1).astype(np.int32)
    acc = tref.accumulate(np.zeros((F * T, 4), np.int64), texel, target, mask)
    assert np.array_equal(tref.face_totals(acc, F, R), cen.census(F, key, target, mask))


def test_the_reference_resolve_applies_its_rules_in_order():
    F, R, Cx, Cy = 3, 2, 2, 1
    T = 3
    acc = np.zeros((F * T, 4), np.int64)
    acc[0] = (2, 65536, 0, 2 * 65536)  # face 0 texel 0: two pixels
    acc[1] = (1, 65536, 65536, 0)      # face 0 texel 1: one pixel; face 0 texel 2: none -> the face's mean; face 1: nothing; face 2: nothing
    fb = np.array([[9, 9, 9], [0.25, 2.0, -1.0], [np.nan, 0.5, 0.75]], np.float32)
    image, state, rgb8 = tref.resolve(acc, F, R, Cx, Cy, min_count=2, face_fallback=fb, fill=(0.1, 0.2, 0.3))
    x, y = tref.texel_position(np.array([0, 0, 0, 1, 2]), np.array([0, 1, 0, 0, 0]), np.array([0, 0, 1, 0, 0]), R, Cx)
    assert state[y, x].tolist() == [3, 2, 2, 1, 1] and (state == 0).sum() == Cx * Cy * (R + 1) * R - 9
    assert image[:, y[0], x[0]].tolist() == [0.5, 0.0, 1.0] and image[:, y[1], x[1]].tolist() == [np.float32(2 / 3), np.float32(1 / 3), np.float32(2 / 3)]
    assert image[:, y[3], x[3]].tolist() == [0.25, 2.0, -1.0] and rgb8[y[3], x[3]].tolist() == [64, 255, 0]
    assert rgb8[y[4], x[4]].tolist() == [0, 128, 191]  # NaN -> 0; 127.5 -> 128 (ties to even); 191.25 -> 191
    assert np.array_equal(image[:, state == 0], np.tile(np.float32([0.1, 0.2, 0.3])[:, None], (1, int((state == 0).sum()))))
    _, state2, _ = tref.resolve(acc, F, R, Cx, Cy, min_count=1, face_fallback=None)
    assert state2[y, x].tolist() == [3, 3, 2, 0, 0]


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (7, 65)])
def test_png_round_trips_through_a_reader_of_the_format(mt, shape):
    H, W = shape
    rgb = np.random.default_rng(H * W).integers(0, 256, (H, W, 3)).astype(np.uint8)
    data = mt.encode_png(torch.from_numpy(rgb))
    assert np.array_equal(tref.read_png_rgb8(data), rgb)
    assert data == mt.encode_png(rgb)  # arrays and tensors alike
    with pytest.raises(ValueError):
        mt.encode_png(rgb.astype(np.float32))
    with pytest.raises(ValueError):
        mt.encode_png(rgb[:, :, :2])


def _baked(mt, F, R, seed=0):
    lay = mt.atlas_layout(F, R)
    rgb8 = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (lay.height, lay.width, 3)).astype(np.uint8))
    image = (rgb8.permute(2, 0, 1).to(torch.float32) / 255.0).contiguous()
    return mt.BakedTexture(image, rgb8, torch.zeros((lay.height, lay.width), dtype=torch.uint8), mt.face_uvs(lay, F), lay)


def test_glb_holds_unshared_vertices_uvs_and_the_atlas_as_png(mt, tmp_path):
    from diff_recon_hip.mesh_renderer import load_glb_mesh
    from diff_recon_hip.raw_triangle import read_glb
    rng = np.random.default_rng(5)
    V, F, R = 6, 7, 3
    vertices = rng.normal(size=(V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    baked = _baked(mt, F, R)
    p = tmp_path / "t.glb"
    mt.save_glb_textured_mesh(str(p), torch.from_numpy(vertices), torch.from_numpy(faces), baked)
    raw = p.read_bytes()
    magic, version, total = struct.unpack_from("<4sII", raw, 0)
    assert (magic, version, total) == (b"glTF", 2, len(raw)) and total % 4 == 0
    jlen, jkind = struct.unpack_from("<I4s", raw, 12)
    assert jkind == b"JSON" and jlen % 4 == 0
    blen, bkind = struct.unpack_from("<I4s", raw, 20 + jlen)
    assert bkind == b"BIN\x00" and blen % 4 == 0 and 28 + jlen + blen == total
    doc, binary = read_glb(str(p))
    assert doc["asset"]["version"] == "2.0" and doc["buffers"][0]["byteLength"] == len(binary)
    prim = doc["meshes"][0]["primitives"][0]
    acc = doc["accessors"]
    assert doc["meshes"][0]["name"] == "geometry_0" and prim["mode"] == 4 and set(prim["attributes"]) == {"POSITION", "TEXCOORD_0"}
    a_pos, a_uv, a_idx = acc[prim["attributes"]["POSITION"]], acc[prim["attributes"]["TEXCOORD_0"]], acc[prim["indices"]]
    assert a_pos["count"] == a_uv["count"] == a_idx["count"] == 3 * F
    assert (a_pos["componentType"], a_pos["type"]) == (5126, "VEC3") and (a_uv["componentType"], a_uv["type"]) == (5126, "VEC2")
    assert (a_idx["componentType"], a_idx["type"]) == (5125, "SCALAR") and "normalized" not in a_uv
    for a in acc:  # every accessor fits its view, every view fits the buffer, views are 4-byte aligned
        v = doc["bufferViews"][a["bufferView"]]
        item = {5125: 4, 5126: 4}[a["componentType"]] * {"SCALAR": 1, "VEC2": 2, "VEC3": 3}[a["type"]]
        assert a["count"] * item == v["byteLength"] and v["byteOffset"] % 4 == 0 and v["byteOffset"] + v["byteLength"] <= len(binary)
    view = lambda a: doc["bufferViews"][a["bufferView"]]
    pos = np.frombuffer(binary, "<f4", 9 * F, view(a_pos)["byteOffset"]).reshape(-1, 3)
    assert np.array_equal(pos, vertices[faces.reshape(-1)])
    assert np.allclose(a_pos["min"], pos.min(axis=0)) and np.allclose(a_pos["max"], pos.max(axis=0))  # required for POSITION
    uv = np.frombuffer(binary, "<f4", 6 * F, view(a_uv)["byteOffset"]).reshape(F, 3, 2)
    assert np.array_equal(uv.view(np.uint32), baked.uv.numpy().view(np.uint32))
    assert np.array_equal(np.frombuffer(binary, "<u4", 3 * F, view(a_idx)["byteOffset"]), np.arange(3 * F))
    # the material chain: primitive -> material -> texture -> (sampler, image -> bufferView)
    tex = doc["materials"][prim["material"]]["pbrMetallicRoughness"]["baseColorTexture"]["index"]
    sampler, image = doc["samplers"][doc["textures"][tex]["sampler"]], doc["images"][doc["textures"][tex]["source"]]
    assert sampler == {"magFilter": 9728, "minFilter": 9728, "wrapS": 33071, "wrapT": 33071}
    assert image["mimeType"] == "image/png" and "uri" not in image
    iv = doc["bufferViews"][image["bufferView"]]
    assert iv["byteOffset"] % 4 == 0 and "target" not in iv and iv["byteOffset"] + iv["byteLength"] <= len(binary)
    png = binary[iv["byteOffset"]:iv["byteOffset"] + iv["byteLength"]]
    assert np.array_equal(tref.read_png_rgb8(png), baked.rgb8.numpy())
    # the geometry reads back through the loader of every other GLB here
    v2, f2, _ = load_glb_mesh(str(p), "cpu")
    assert np.array_equal(v2.numpy()[f2.numpy().astype(np.int64)], vertices[faces.astype(np.int64)])
    with pytest.raises(ValueError):
        mt.save_glb_textured_mesh(str(p), vertices, np.array([[0, 1, V]], np.int32), _baked(mt, 1, R))
    with pytest.raises(ValueError):
        mt.save_glb_textured_mesh(str(p), vertices, faces[:3], baked)  # the UVs of another face count


def test_glb_of_an_empty_mesh(mt, tmp_path):
    from diff_recon_hip.raw_triangle import read_glb
    p = tmp_path / "e.glb"
    mt.save_glb_textured_mesh(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), _baked(mt, 0, 2))
    doc, binary = read_glb(str(p))
    assert [a["count"] for a in doc["accessors"]] == [0, 0, 0] and len(binary) % 4 == 0


def test_python_errors_need_no_device(mt):
    for args in ((-1, 4), (4, 0), (4, 65), (4, 4, 0), (2 ** 31, 1), (2 ** 21, 64), (10, 64, 2 ** 26)):
        with pytest.raises(ValueError):
            mt.atlas_layout(*args)
    lay = mt.atlas_layout(4, 2)
    with pytest.raises(ValueError):
        mt.face_uvs(lay, 5)  # more faces than the layout has half-cells
    with pytest.raises(ValueError):
        mt.TextureAtlas(-1, 2, "cpu")
    with pytest.raises(ValueError):
        mt.TextureAtlas(3, 65, "cpu")
    cam = type("Cam", (), dict(image_width=4, image_height=3, tan_fovx=0.5, tan_fovy=0.5, world_view_transform=torch.eye(4), device="cpu"))()
    v, f, fi = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mt.texel_index(cam, v, f, fi, mt.atlas_layout(1, 2))
    atlas = mt.TextureAtlas(1, 2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        atlas.add(cam, v, f, fi)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        atlas.face_totals()
    with pytest.raises(ValueError):
        atlas.add(cam, v, torch.zeros((2, 3), dtype=torch.int32), fi)  # another face count
    with pytest.raises(ValueError):
        atlas.resolve(min_count=0)
    with pytest.raises(ValueError):
        atlas.resolve(face_fallback=torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        atlas.resolve(fill=(0.1, 0.2))
    with pytest.raises(ValueError):
        atlas += mt.TextureAtlas(1, 3, "cpu")
    other = mt.TextureAtlas(1, 2, "cpu")
    other.texels[1, 0] = 5
    atlas += other
    assert atlas.texels[1, 0] == 5 and atlas.texels.shape == (3, 4)


def test_the_package_exports_the_texture_names(mt):
    import diff_recon_hip
    for name in ("AtlasLayout", "BakedTexture", "TextureAtlas", "atlas_layout", "face_uvs", "texel_index", "render_textured", "bake_texture",
                 "evaluate_textured", "save_glb_textured_mesh"):
        assert getattr(diff_recon_hip, name) is getattr(mt, name)


def test_the_library_exports_exactly_its_header_and_the_table_matches_it(mt):
    """libts_atlas.so: the five tsa_ entry points of include/ts_atlas.h and nothing else of ours, no rocPRIM, its own soname; and
    _abi.ATLAS_SIGNATURES has the header's names and arities."""
    from diff_triangle_rasterization_2D import _abi
    lib = mt.library_path()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if l.split()[-2:-1] and l.split()[-2] in ("T", "D", "B", "R")]
    ours = sorted(n for n in exported if not n.startswith("__hip_"))
    assert ours == ["tsa_face_totals", "tsa_last_error", "tsa_render", "tsa_resolve", "tsa_texel_index"]
    assert "rocprim" not in subprocess.run(["nm", "-D", lib], capture_output=True, text=True).stdout.lower()
    assert "libts_atlas.so" in subprocess.run(["readelf", "-d", lib], capture_output=True, text=True).stdout
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ts_atlas.h")).read(), flags=re.S)
    protos = {name: params for name, params in re.findall(r"\b(tsa_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert set(protos) == set(_abi.ATLAS_SIGNATURES) == set(ours)
    for name, params in protos.items():
        n = 0 if params.strip() == "void" else len(params.split(","))
        assert n == len(_abi.ATLAS_SIGNATURES[name][1]), name


def test_example_refuses_bake_texture_without_extract_mesh():
    import sys
    example = os.path.join(ROOT, "examples", "train_synthetic.py")
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--bake-texture", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "--bake-texture" in r.stderr and "--extract-mesh" in r.stderr
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--extract-mesh", "32", "--bake-texture", "65"], capture_output=True, text=True)
    assert r.returncode == 2 and "1 .. 64" in r.stderr
    r = subprocess.run([sys.executable, example, "--eval-mesh", "--extract-mesh", "32", "--out", "x.glb"], capture_output=True, text=True)
    assert r.returncode == 2 and "--out" in r.stderr and "--bake-texture" in r.stderr
