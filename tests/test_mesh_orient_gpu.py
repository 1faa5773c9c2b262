"""GPU tests of the consistent orientation against tests/ref_mesh_orient.py, everything bit for bit: face_piece, face_flip, out_faces and the
ten counts in all three modes; the promises on the device's own output by a second call; the no-ops; determinism and purity; the chain
simplify -> split -> scramble -> orient -> fans -> fill -> normals; orient_fused on the device's own fusion; the example's line."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_mesh_manifold
import ref_mesh_orient as ref
import ref_mesh_simplify as fixtures
import ref_volume
from test_mesh_smooth_gpu import _soup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.nonzero(np.ascontiguousarray(got).reshape(-1) != np.ascontiguousarray(want).reshape(-1))[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], got.reshape(-1)[diff[:5]], want.reshape(-1)[diff[:5]])


def _gpu_orient(v, f, keep, mode):
    """tsw_orient's four arrays; v is handed over in every mode (the library reads it in mode 2 only)."""
    from diff_recon_hip import mesh_orient
    fd = f if isinstance(f, torch.Tensor) else _faces(f)
    vd = _dev(np.asarray(v, np.float32).reshape(-1, 3))
    return mesh_orient._orient_arrays(vd, vd.shape[0], fd, None if keep is None else _dev(np.asarray(keep, np.uint8)), ref.MODES[mode], fd.device)


def _assert_everything(v, f, keep=None, modes=tuple(ref.MODES)):
    """Every output against the reference in every mode, then the promises, by calling the device a second time on its own output."""
    V, wants = len(v), {}
    for mode in modes:
        want = ref.orient(V, f, keep, mode, v)
        face_piece, face_flip, out_faces, counts = _gpu_orient(v, f, keep, mode)
        _same(face_piece, want["face_piece"], ("face_piece", mode))
        _same(face_flip, want["face_flip"], ("face_flip", mode))
        _same(out_faces, want["out_faces"], ("out_faces", mode))
        assert counts.tolist() == want["counts"] and counts.dtype == torch.int64, (mode, counts.tolist(), want["counts"])
        piece2, flip2, again, counts2 = _gpu_orient(v, out_faces, keep, mode)
        c1, c2 = counts.tolist(), counts2.tolist()
        assert c2[5] == c1[6] == c2[6] and (c1[2] > 0 or c1[6] == 0)         # what is left is what a second call finds; only where a piece is twisted
        assert torch.equal(again, out_faces) and c2[7] == 0 and c2[8] == 0 and not flip2.any()  # a second call flips nothing, bit for bit
        assert torch.equal(piece2, face_piece) and c2[:5] == c1[:5]          # the pieces do not depend on the winding
        non = _dev(want["nonorientable"])
        assert torch.equal(out_faces[non], _faces(f)[non])                   # a non-orientable piece comes back bit for bit
        wants[mode] = want
    return wants


# ---- strips: runs and union chains across blocks, one piece takes every per-piece add ----------------------------------------------------------------
@pytest.mark.parametrize("twist", [False, True])
@pytest.mark.parametrize("n", [3, 128, 129, 1025, 4097])
def test_strips_match_the_reference_bit_for_bit(n, twist):
    v, f = ref.strip(n, twist)
    g, mask, order = ref.scramble(f, 10 * n + twist)
    wants = _assert_everything(v, g)
    for mode, want in wants.items():
        assert want["counts"][:5] == [2 * n, 1, int(twist), 2 * n * int(twist), 2 * n] and (want["face_piece"] == 0).all()
        if twist:
            assert np.array_equal(want["out_faces"], g.astype(np.int32)) and want["counts"][6] == want["counts"][5] > 0
        else:
            assert want["counts"][6] == 0 and want["counts"][5] > 0
    if not twist:  # one of the two consistent windings: the fewer flips by majority
        flips = wants["majority"]["face_flip"].astype(bool)
        assert np.array_equal(flips, mask) or np.array_equal(flips, ~mask)
        assert 2 * flips.sum() <= 2 * n


# ---- one mesh of several pieces ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    return ref.mixed_mesh()


@pytest.mark.parametrize("kept", [False, True])
def test_mixed_mesh_matches_the_reference_bit_for_bit(kept):
    v, f, keep, parts = _mixed()
    wants = _assert_everything(v, f, keep if kept else None)
    part = ref_mesh_manifold.participation(len(v), f, keep if kept else None)
    assert (~part).sum() >= 5
    for mode, want in wants.items():
        c = want["counts"]
        print(f"mixed mesh, keep {'on' if kept else 'off'}, {mode}: {dict(zip(ref.COUNT_NAMES, c))}")
        assert c[2] >= 1 and c[6] > 0 and c[5] > c[6] and c[1] > 257
        for name in ("klein", "moebius") if not kept else ():  # whole, both are twisted (with faces dropped a piece of one may not be)
            rows = parts[name][1]
            assert np.array_equal(want["out_faces"][rows], f[rows].astype(np.int32)) and want["nonorientable"][rows].all()
        rows = parts["book"][1][part[parts["book"][1]]]
        assert len(np.unique(want["face_piece"][rows])) == len(rows)  # a book's spine links nothing: one-face pieces
    if not kept:
        vol = wants["volume"]
        for name in ("sphere", "small", "torus"):  # closed and orientable: outward, whatever the scrambler did
            rows = parts[name][1]
            assert len(np.unique(vol["face_piece"][rows])) == 1 and ref.signed_volume(v, vol["out_faces"][rows]) > 0
        first, rows = parts["small"]
        centred = v.astype(np.float64) - np.array([50.0, 0, 0])
        assert ref.signed_volume(centred, vol["out_faces"][rows]) > 0 and vol["face_flip"][rows].all()  # the 2 mm sphere 50 units away was inward
        assert 2 ** 40 < vol["S"][int(vol["face_piece"][rows[0]])] * -1 < 2 ** 59  # as given its volume is negative, and well resolved


# ---- random soups -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 63, 257, 1025, 4097])
def test_random_soups_match_the_reference_bit_for_bit(V):
    """ref_mesh_manifold's soups, and test_mesh_smooth_gpu's: indices -1 and V, repeated indices, duplicated, rotated and reversed triples, a hub,
    NaN and inf among the vertices (mode 2 counts their faces)."""
    sizes = tuple(s for s in ref_mesh_manifold.SOUP_SIZES + (4097,) if s <= V)
    plain = ref_mesh_manifold.soups(sizes)[V]
    v, f, keep, _ = _soup(V)
    for faces, k in ((plain, None), (f, None), (f, keep)):
        wants = _assert_everything(v, faces, k)
        c = wants["volume"]["counts"]
        print(f"soup V = {V}, keep {'on' if k is not None else 'off'}: {dict(zip(ref.COUNT_NAMES, c))}")
        part = ref_mesh_manifold.participation(V, faces, k)
        assert np.array_equal(wants["volume"]["out_faces"][~part], np.asarray(faces, np.int32)[~part])
        if V >= 63 and faces is f:
            assert c[9] > 0 and c[4] > 0 and (~part).sum() > 0


def test_nonfinite_vertices_are_counted_and_a_piece_of_zero_terms_is_unchanged():
    v, f = ref.latlong_sphere()
    inward = f[:, [0, 2, 1]]
    w = v.copy()
    w[5], w[9, 1], w[200, 2] = np.nan, np.inf, -np.inf
    touched = int(np.isin(f, [5, 9, 200]).any(1).sum())
    want = _assert_everything(w, inward, modes=("volume",))["volume"]
    assert want["counts"][9] == touched and want["counts"][7:9] == [len(f), 1]
    w[0] = np.nan  # the anchor vertex: every term is 0, S_p == 0 changes nothing
    want = _assert_everything(w, inward, modes=("volume",))["volume"]
    assert want["counts"][9] == len(f) and want["counts"][7:9] == [0, 0] and np.array_equal(want["out_faces"], inward.astype(np.int32))
    flat = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    want = _assert_everything(flat, np.array([[0, 1, 2], [0, 3, 2]]), modes=("volume",))["volume"]
    assert want["S"] == {0: 0} and want["counts"][5:9] == [1, 0, 1, 0] and want["out_faces"].tolist() == [[0, 1, 2], [0, 2, 3]]
    huge = (v.astype(np.float64) * 1e38).astype(np.float32)  # differences up to 2^127: the terms stay finite in float64, the scale absorbs them
    want = _assert_everything(huge, inward, modes=("volume",))["volume"]
    assert want["counts"][7:10] == [len(f), 1, 0]
    tiny = (v.astype(np.float64) * 1e-38).astype(np.float32)  # subnormal fp32 coordinates
    want = _assert_everything(tiny, inward, modes=("volume",))["volume"]
    assert want["counts"][7:10] == [len(f), 1, 0]


def test_no_faces_and_no_vertices_are_no_ops():
    from diff_recon_hip import orient_faces
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    zero = dict.fromkeys(ref.COUNT_NAMES, 0)
    for V in (0, 5):
        for outward in ref.MODES:
            out = orient_faces(torch.zeros((V, 3), device=DEV), f0, outward=outward)
            assert out.faces.shape == (0, 3) and out.face_flip.shape == (0,) and out.face_piece.shape == (0,) and out.stats == zero
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    wants = _assert_everything(np.zeros((0, 3), np.float32), f)
    for want in wants.values():
        assert want["counts"] == [0] * 10 and (want["face_piece"] == -1).all() and np.array_equal(want["out_faces"], f.astype(np.int32))


# ---- determinism and purity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(ref.MODES))
def test_the_call_is_pure_and_deterministic(mode):
    v, f, keep, _ = _mixed()
    want = ref.orient(len(v), f, keep, mode, v)

    def call(pattern):  # the workspace and every output come from torch.empty and are poisoned, with guard bytes either side
        face_piece, face_flip, out_faces, counts = _gpu_orient(v, f, keep, mode)
        return {"face_piece": face_piece, "face_flip": face_flip, "out_faces": out_faces, "counts": counts}

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    for key in ("face_piece", "face_flip", "out_faces"):
        assert base[key].numpy().tobytes() == want[key].tobytes(), key
    assert base["counts"].numpy().view(np.int64).tolist() == want["counts"]


# ---- the public wrappers ------------------------------------------------------------------------------------------------------------------------
def test_chain_simplify_split_scramble_orient_fans_fill_normals():
    from diff_recon_hip import fill_holes, orient_faces, simplify_mesh, split_nonmanifold, vertex_fans, vertex_normals
    v, f = fixtures.sphere_mesh()
    origin = tuple((v.min(0) - 0.01).tolist())
    s = simplify_mesh(_dev(v), _faces(f), 2.0, origin=origin)
    clean = split_nonmanifold(s.vertices, s.faces)
    V, F = clean.vertices.shape[0], clean.faces.shape[0]
    hv, hf = clean.vertices.cpu().numpy(), clean.faces.cpu().numpy()
    base = ref.orient(V, hf, None, "volume", hv)
    assert base["counts"][5:9] == [0, 0, 0, 0] and (V, F) == (419, 719)  # the split mesh is consistent and no piece faces inward
    # Flat pieces (the lone flap faces of the pinched cells: S_p == 0) have no outward side and keep whatever winding they are given, so the
    # mask reverses faces of the pieces that enclose a volume only; the faces keep their order, which fill_holes and vertex_normals read.
    solid = np.array([base["S"][int(p)] > 0 for p in base["face_piece"]])
    mask = (np.random.default_rng(17).random(F) < 0.5) & solid
    assert solid.sum() > 600 and (~solid).sum() > 0 and mask.sum() > 250
    scrambled = np.where(mask[:, None], hf[:, [0, 2, 1]], hf)
    assert vertex_fans(V, _faces(scrambled)).stats["same_direction_edges"] > 300
    out = orient_faces(clean.vertices, _faces(scrambled), outward="volume")
    want = ref.orient(V, scrambled, None, "volume", hv)
    assert [out.stats[k] for k in ref.COUNT_NAMES] == want["counts"] and out.stats["same_direction_before"] > 300
    _same(out.faces, want["out_faces"], "orient_faces faces")
    assert torch.equal(out.faces, clean.faces) and torch.equal(out.face_flip, _dev(mask)) and out.face_flip.dtype == torch.bool
    assert vertex_fans(V, out.faces).stats["same_direction_edges"] == 0
    a, b = fill_holes(clean.vertices, clean.faces), fill_holes(clean.vertices, out.faces)
    assert a.stats == b.stats and a.stats["filled_loops"] > 0 and torch.equal(a.faces, b.faces) and torch.equal(a.loop_status, b.loop_status)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    broken = fill_holes(clean.vertices, _faces(scrambled))
    assert broken.stats != a.stats  # the fill takes the winding on trust: the scrambled mesh does not close the same way
    (na, va), (nb, vb) = vertex_normals(clean.vertices, clean.faces), vertex_normals(clean.vertices, out.faces)
    assert torch.equal(na.view(torch.int32), nb.view(torch.int32)) and torch.equal(va, vb) and va.any()
    ns, _ = vertex_normals(clean.vertices, _faces(scrambled))
    assert not torch.equal(ns.view(torch.int32), na.view(torch.int32))


def _cams():
    return [SimpleNamespace(world_view_transform=_dev(np.asarray(ref_volume.look_at_view(eye), np.float32)), tan_fovx=0.45, tan_fovy=0.45,
                            image_width=48, image_height=48, device="cuda:0") for eye in ref_volume.AXIS_EYES]


def test_orient_fused_restores_the_fusion_of_both_kinds():
    """The six axis views of the fusion's end-to-end test, fused with and without colour; half the faces reversed; orient_fused by volume."""
    from diff_recon_hip import fuse_colored_mesh, fuse_mesh, orient_fused
    v, f = ref.latlong_sphere()
    vd, fd = _dev(v), _faces(f)
    colour = _dev(np.full((len(f), 3), 0.25, np.float32))
    for mesh in (fuse_mesh(_cams(), vd, fd, 24), fuse_colored_mesh(_cams(), vd, fd, colour, 24)):
        F, hv, hf = mesh.faces.shape[0], mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
        base = ref.orient(len(hv), hf, None, "volume", hv)
        assert base["counts"][2:4] == [0, 0] and base["counts"][5:9] == [0, 0, 0, 0] and F > 500  # consistent and outward as extracted
        solid = np.array([base["S"][int(p)] > 0 for p in base["face_piece"]])  # a flat piece has no outward side to restore
        mask = _dev((np.random.default_rng(F).random(F) < 0.5) & solid)
        assert solid.sum() > 500 and int(mask.sum()) > 200
        broken = mesh._replace(faces=torch.where(mask[:, None], mesh.faces[:, [0, 2, 1]], mesh.faces))
        for outward in ("volume", "anchor"):
            out = orient_fused(broken, outward)
            assert type(out) is type(mesh) and out._fields == mesh._fields
            s = out.stats["orient"]
            print(f"{type(mesh).__name__}, {outward}: {s}")
            want = ref.orient(len(hv), broken.faces.cpu().numpy(), None, outward, hv)
            assert [s[k] for k in ref.COUNT_NAMES] == want["counts"]
            _same(out.faces, want["out_faces"], ("orient_fused faces", outward))
            assert s["outward"] == outward and s["pieces"] == base["counts"][1] and s["same_direction_before"] > F // 4 and s["same_direction_after"] == 0
            assert {k: x for k, x in out.stats.items() if k != "orient"} == mesh.stats
            for name in mesh._fields:
                if name not in ("faces", "stats"):
                    assert getattr(out, name) is getattr(broken, name), name  # every other field is the same object
            assert out.faces.dtype == torch.int32 and out.faces.shape == mesh.faces.shape
            if outward == "volume":
                assert torch.equal(out.faces, mesh.faces) and s["faces_flipped"] == int(mask.sum())  # restored
            else:  # every anchor keeps its direction: its piece is restored, or turned inside out as a whole
                piece = _dev(want["face_piece"]).to(torch.int64)
                turned = mask[piece]
                assert torch.equal(out.faces, torch.where(turned[:, None], mesh.faces[:, [0, 2, 1]], mesh.faces))


def test_example_reports_the_oriented_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    res = train_synthetic.mesh_scores(m, "2D", extract=24, simplify=3.0, fill=16, split=True, weld=0.02, orient="majority", **cfg)
    fused, welded = res["fused"], res["welded"]
    for s, what in ((fused["oriented"], "fused"), (welded["oriented"], "welded")):
        lines = train_synthetic.oriented_report(s, what)
        print("\n".join(lines))
        assert len(lines) == 1 and lines[0].startswith(f"oriented {what} mesh, outward by majority: {s['pieces']} pieces, {s['nonorientable_pieces']} non-orientable; ")
        assert f"{s['same_direction_before']} -> {s['same_direction_after']} same-direction edges, {s['faces_flipped']} of {s['faces']} faces flipped" in lines[0]
        assert s["same_direction_after"] <= s["same_direction_before"] and (s["nonorientable_pieces"] > 0 or s["same_direction_after"] == 0)
    assert fused["oriented"]["same_direction_before"] >= fused["manifold"]["same_direction_edges"]  # it follows the split, which keeps every edge used twice
    assert welded["oriented"]["same_direction_before"] > 0  # a welded soup has no preferred winding: conflicts are the rule
    plain = train_synthetic.mesh_scores(m, "2D", extract=24, simplify=3.0, fill=16, split=True, weld=0.02, **cfg)  # without the flag: nothing else changes
    assert "oriented" not in plain["fused"] and "oriented" not in plain["welded"]
    assert plain["fused"]["manifold"] == fused["manifold"] and plain["fused"]["topology"] == fused["topology"]
    assert {k: x for k, x in welded.items() if k != "oriented"}.keys() == plain["welded"].keys() and plain["welded"]["topology"] == welded["topology"]
