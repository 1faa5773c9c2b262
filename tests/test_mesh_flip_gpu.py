"""GPU tests of the edge flip against tests/ref_mesh_flip.py, everything bit for bit and to its capacity: out_faces, face_flipped,
edge_vertices, edge_state, edge_opposite with their fill values, and totals; the hand constructions, sheared and stretched grids round by
round to convergence, more scan tiles than a workgroup has lanes, the ends of the binary search, rounding noise on a sphere, the output of
split_edges, keep masks, seeds, flip_fused, the empty calls, purity."""
import numpy as np
import pytest
import torch

import poison
import ref_mesh_flip as ref
import ref_mesh_subdivide
from test_mesh_smooth_gpu import _latlong_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("out_faces", "face_flipped", "edge_vertices", "edge_state", "edge_opposite")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _faces(f):
    return _dev(np.asarray(f, np.int32).reshape(-1, 3))


def _same(got, want, what):
    """Equal shapes, dtypes and BYTES."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.nonzero(np.ascontiguousarray(got).reshape(-1) != np.ascontiguousarray(want).reshape(-1))[0]
    assert len(diff) == 0, (what, len(diff), diff[:5], got.reshape(-1)[diff[:5]], want.reshape(-1)[diff[:5]])


def _gpu_round(v, f, keep=None, min_cos=1.0, seed=0, classify_only=False):
    from diff_recon_hip import mesh_flip
    fd = _faces(f)
    k = None if keep is None else _dev(np.asarray(keep, np.uint8))
    return mesh_flip._flip_arrays(_dev(np.asarray(v, np.float32).reshape(-1, 3)), fd, k, float(min_cos), seed, classify_only, fd.device)


def _assert_round(v, f, keep=None, deg=30.0, seed=0, what=""):
    """tse_flip against the reference, every output to its capacity, with and without the face outputs."""
    min_cos = ref.min_cos_of(deg)
    want = ref.flip_round(v, f, keep, min_cos, seed)
    for classify_only in (False, True):
        got = _gpu_round(v, f, keep, min_cos, seed, classify_only)
        assert got[5].tolist() == want["totals"] and got[5].dtype == torch.int64, (what, got[5].tolist(), want["totals"])
        for name, t in zip(NAMES, got[:5]):
            if classify_only and name in NAMES[:2]:
                assert t is None
            else:
                _same(t, want[name], (what, name, classify_only))
    return want


def _assert_all_rounds(v, f, keep=None, deg=30.0, max_rounds=64, what=""):
    """Round by round with seed = round index until one flips nothing; then delaunay_flips as a whole against the same."""
    from diff_recon_hip import delaunay_flips
    f0, per_round, union = np.asarray(f, np.int32).reshape(-1, 3), [], np.zeros(len(f), bool)
    g, converged = f0, False
    for r in range(max_rounds):
        want = _assert_round(v, g, keep, deg, r, (what, "round", r))
        if want["totals"][3] == 0:
            converged = True
            break
        per_round.append(want["totals"])
        union |= want["face_flipped"] != 0
        g = want["out_faces"]
    out = delaunay_flips(_dev(np.asarray(v, np.float32)), _faces(f0), None if keep is None else _dev(np.asarray(keep, np.uint8)), deg, max_rounds)
    _same(out.faces, g, (what, "faces"))
    assert out.converged == converged == out.stats["converged"] and out.stats["rounds"] == len(per_round)
    assert [[t[k] for k in ("edges", "nondelaunay", "candidates", "flipped")] for t in out.stats["per_round"]] == per_round
    assert np.array_equal(out.face_flipped.cpu().numpy(), union) and out.face_flipped.dtype == torch.bool
    assert out.stats["flipped"] == sum(t[3] for t in per_round)
    return g, per_round, converged


# ---- the hand constructions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.hand_constructions()))
def test_hand_constructions_match_the_reference_bit_for_bit(name):
    v, f, keep, deg = ref.hand_constructions()[name]
    for seed in (0, 7):
        want = _assert_round(v, f, keep, deg, seed, name)
    if name in ("long diagonal", "cap"):
        assert want["out_faces"].tolist() == [[0, 3, 2], [3, 1, 2]] and want["totals"] == [5, 1, 1, 1]
    if name == "two quads over one vertex pair":
        assert want["totals"] == [10, 2, 2, 1] and sorted(want["edge_state"][:10].tolist())[-2:] == [ref.DUPLICATE, ref.FLIPPED]


# ---- grids, all rounds to convergence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(1, 1), (1, 2), (2, 2), (3, 3), (7, 7), (17, 17)])
def test_sheared_grids_match_round_by_round_until_they_converge(cells):
    """F = 2, 4, 8, 18, 98, 578: sheared by two cells per row and jittered by 3 in a spacing of 8, so that it takes several rounds."""
    v, f = ref.sheared_grid(*cells, 8, 8, 3, seed=cells[0], shear=2)
    assert len(f) == 2 * cells[0] * cells[1]
    g, per_round, converged = _assert_all_rounds(v, f, what=cells)
    assert converged and len(per_round) >= (3 if cells[0] >= 3 else 1)
    print(f"F = {len(f)}: {len(per_round)} rounds, flips {[t[3] for t in per_round]}")


@pytest.mark.parametrize("cells", [(7, 7), (17, 17)])
def test_stretched_grids_have_candidates_that_lose(cells):
    v, f = ref.stretched_grid(*cells)
    first = ref.flip_round(v, f, min_cos=ref.min_cos_of(30.0))
    assert (first["edge_state"] == ref.LOST).sum() > 0
    g, per_round, converged = _assert_all_rounds(v, f, what=cells)
    assert converged and len(per_round) >= 3


def test_more_scan_blocks_than_one_workgroup_has_lanes():
    """180000 faces: 264 scan tiles of half-edges, so a lane of the offsets kernel owns two; 43 tiles of winners."""
    v, f = ref.sheared_grid(300, 300, 8, 8, 3, seed=5, shear=2)
    assert len(f) == 180000 and -(-3 * len(f) // 2048) > 256
    want = _assert_round(v, f, None, 30.0, 0, "large")
    assert want["totals"][3] > 50000
    again = _assert_round(v, want["out_faces"], None, 30.0, 1, "large, second round")
    assert 0 < again["totals"][3] < want["totals"][3]


# ---- small tables, the ends of the binary search ----------------------------------------------------------------------------------------------
def test_small_tables_and_the_ends_of_the_binary_search():
    """A face that takes part has three edges, so the smallest tables are E = 3 (one face: the winners' list has one slot) and E = 5.  The
    quad relabelled so that the new edge (c, d) sorts in front of the first entry of the table, (0, 1), and behind the last, (2, 3); and the
    closed flattened tetrahedron, where those two ARE the first and the last entry; each also with a masked face behind, whose sentinel
    keys end the sorted columns."""
    assert _assert_round(ref.QUAD, [[0, 1, 2]], what="E = 3")["totals"] == [3, 0, 0, 0]
    front = ref.QUAD[[2, 3, 0, 1]]  # a = 2, b = 3, c = 0, d = 1
    for v, f, new in ((ref.QUAD, ref.LONG, (2, 3)), (front, [[2, 3, 0], [3, 2, 1]], (0, 1))):
        for extra, keep in (([], None), ([[0, 1, 2]], [1, 1, 0])):
            want = _assert_round(v, f + extra, keep, what=("E = 5", new))
            assert want["totals"] == [5, 1, 1, 1]
            table = [tuple(e) for e in want["edge_vertices"][:5].tolist()]
            assert new not in table and (new < table[0] or new > table[-1])
    tet = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    for extra, keep in (([], None), ([[0, 1, 2]], [1, 1, 1, 1, 0])):
        want = _assert_round(ref.QUAD, tet + extra, keep, deg=180.0, what="tetrahedron")
        assert want["totals"][0] == 6 and want["totals"][2] == 0 and want["edge_state"][0] == ref.GUARDED  # (0, 1) proposes (2, 3), the last entry
        assert want["edge_vertices"][0].tolist() == [0, 1] and want["edge_vertices"][5].tolist() == [2, 3]


# ---- rounding noise -----------------------------------------------------------------------------------------------------------------------
def test_latlong_sphere_flips_come_from_rounding_and_still_match():
    """The quads of a lat-long sphere are cocircular up to the rounding of their fp32 vertices: which of them flip is rounding noise, and
    the device decides every one as the reference does."""
    v, f = _latlong_sphere()
    g, per_round, converged = _assert_all_rounds(v, f, deg=30.0, max_rounds=8, what="sphere")
    print(f"lat-long sphere, {len(f)} faces: {len(per_round)} rounds, converged {converged}, flips {[t[3] for t in per_round]}")


# ---- behind split_edges -----------------------------------------------------------------------------------------------------------------------
def test_flips_behind_a_partial_split_keep_every_count():
    from diff_recon_hip import delaunay_flips, mesh_edges, mesh_topology, split_edges, subdivide_mesh, triangle_quality
    v, f = ref_mesh_subdivide.cube_grid(4, 4)
    v = v.copy()
    v[:, 0] += 0.5 * v[:, 1]  # sheared: on the cube itself every quad is a rectangle, cocircular, and nothing would flip
    fine = subdivide_mesh(_dev(v), _faces(f), levels=1)
    lengths = mesh_edges(fine.vertices.shape[0], fine.faces, vertices=fine.vertices).length
    mid = 0.5 * (float(lengths.min()) + float(lengths.max()))
    s = split_edges(fine.vertices, fine.faces, max_edge=mid)  # a third of the edges: every face is cut from a corner to a midpoint
    assert 0 < s.stats["marked"] < s.stats["edges"]
    V = s.vertices.shape[0]
    before_e, before_t = mesh_edges(V, s.faces).stats, mesh_topology(V, s.faces)
    out = delaunay_flips(s.vertices, s.faces)
    sv, sf = s.vertices.cpu().numpy(), s.faces.cpu().numpy()
    g, per_round, converged, union = ref.delaunay_flips(sv, sf, None, ref.min_cos_of(30.0))
    _same(out.faces, g, "faces")
    assert out.converged and converged and out.stats["rounds"] == len(per_round) >= 1 and out.stats["flipped"] > 0
    assert mesh_edges(V, out.faces).stats == before_e and mesh_topology(V, out.faces) == before_t
    q0, q1 = triangle_quality(s.vertices, s.faces), triangle_quality(s.vertices, out.faces)
    print(f"split cube grid, {sf.shape[0]} faces: {out.stats['rounds']} rounds, {out.stats['flipped']} flips, {out.stats['guarded']} guarded, "
          f"smallest quality {float(q0.min()):.3f} -> {float(q1.min()):.3f}, median {float(q0.median()):.3f} -> {float(q1.median()):.3f}")
    assert float(q1.min()) >= float(q0.min())


# ---- keep masks, seeds --------------------------------------------------------------------------------------------------------------------
def test_keep_masks_and_broken_faces_match_the_reference():
    v, f = ref.stretched_grid(17, 17)
    rng = np.random.default_rng(3)
    keep = (rng.integers(0, 5, len(f)) != 0).astype(np.uint8)
    f = f.copy()
    f[rng.integers(0, len(f), 6)] = [[0, 0, 1], [-1, 2, 3], [1, 2, len(v)], [5, 6, 5], [2 ** 31 - 1, 0, 1], [7, 7, 7]]
    v = v.copy()
    v[rng.integers(0, len(v), 4)] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    for k in (None, keep, np.zeros(len(f), np.uint8)):
        for seed in (0, 1, 0xFFFFFFFF):
            want = _assert_round(v, f, k, 30.0, seed, "keep")
        if k is keep:
            assert want["totals"][3] > 0 and np.array_equal(want["out_faces"][keep == 0], f[keep == 0])


def test_seed_changes_the_winners_but_not_the_candidates():
    from diff_recon_hip import flip_edges, nondelaunay_edges
    v, f = ref.stretched_grid(17, 17)
    vd, fd = _dev(v), _faces(f)
    first, states = flip_edges(vd, fd, seed=0), set()
    for seed in range(4):
        r, c = flip_edges(vd, fd, seed=seed), nondelaunay_edges(vd, fd, seed=seed)
        want = ref.flip_round(v, f, None, ref.min_cos_of(30.0), seed)
        E = want["E"]
        assert r.stats == dict(edges=want["totals"][0], nondelaunay=want["totals"][1], candidates=want["totals"][2], flipped=want["totals"][3],
                               guarded=want["totals"][1] - want["totals"][2])
        _same(r.edge_state, want["edge_state"][:E], "edge_state")
        _same(r.edge_vertices, want["edge_vertices"][:E], "edge_vertices")
        _same(r.edge_opposite, want["edge_opposite"][:E], "edge_opposite")
        _same(r.faces, want["out_faces"], "faces")
        assert np.array_equal(r.face_flipped.cpu().numpy(), want["face_flipped"] != 0)
        assert c.faces is None and c.face_flipped is None and torch.equal(c.edge_state, r.edge_state) and c.stats == r.stats
        assert torch.equal(r.edge_state >= ref.LOST, first.edge_state >= ref.LOST)  # the same candidates
        assert int(r.face_flipped.sum()) == 2 * r.stats["flipped"]
        states.add(r.edge_state.cpu().numpy().tobytes())
    assert len(states) > 1


# ---- flip_fused -------------------------------------------------------------------------------------------------------------------------------
def test_flip_fused_returns_the_kind_of_mesh_it_was_given():
    from diff_recon_hip import flip_fused, weld_mesh
    from diff_recon_hip.color_volume import ColoredMesh
    v, f = ref.stretched_grid(7, 7)
    g, per_round, converged, union = ref.delaunay_flips(v, f, None, ref.min_cos_of(30.0))
    colour = np.random.default_rng(3).uniform(0, 1, (len(f), 3)).astype(np.float32)
    w = weld_mesh(_dev(v), _faces(f), _dev(colour), eps=0.0)
    assert torch.equal(w.faces.cpu(), torch.from_numpy(f))  # nothing to weld: the indexed mesh is the input
    out = flip_fused(w)
    assert type(out) is type(w) and out.vertices is w.vertices and out.faces_color is w.faces_color and out.vertex_map is w.vertex_map
    _same(out.faces, g, "faces")
    assert out.stats["flip"]["converged"] and out.stats["flip"]["rounds"] == len(per_round)
    assert np.array_equal(out.stats["flip"]["face_flipped"].cpu().numpy(), union) and "flip" not in w.stats
    vc = np.random.default_rng(4).uniform(0, 1, (len(v), 3)).astype(np.float32)
    c = ColoredMesh(_dev(v), _faces(f), _dev(vc), _dev(np.ones(len(v), bool)), {"num_vertices": len(v), "num_faces": len(f)})
    out = flip_fused(c, max_dihedral_deg=30.0, max_rounds=1)
    assert type(out) is ColoredMesh and out.vertex_color is c.vertex_color and not out.stats["flip"]["converged"]
    _same(out.faces, ref.flip_round(v, f, None, ref.min_cos_of(30.0), 0)["out_faces"], "one round")


def test_example_reports_the_flipped_mesh():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    plain = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, **cfg)["welded"]
    res = train_synthetic.mesh_scores(m, "2D", weld=0.02, split_edges=20.0, flip_edges=True, **cfg)["welded"]
    t = res["split"]["flipped"]
    lines = train_synthetic.flip_edges_report(res["split"])
    print("\n".join(lines))
    assert "flipped" not in plain["split"] and {k: v for k, v in res["split"].items() if k != "flipped"} == plain["split"]  # no other entry changes
    assert {k: v for k, v in res.items() if k != "split"} == {k: v for k, v in plain.items() if k != "split"}
    assert len(lines) == 3 and lines[0].startswith(f"flipped mesh: {t['flips']} flips in {t['rounds']} rounds")
    assert f"mean PSNR {res['split']['mean_psnr']:.2f} -> {t['mean_psnr']:.2f} dB" in lines[2]
    assert t["flips"] > 0 and t["slots"] <= 2 * t["flips"] and 0.0 <= t["quality"][0] <= t["quality"][1] <= 1.0


# ---- the empty calls --------------------------------------------------------------------------------------------------------------------------
def test_no_faces_and_no_vertices_write_the_empty_result():
    from diff_recon_hip import delaunay_flips, flip_edges, nondelaunay_edges
    f0 = torch.zeros((0, 3), device=DEV, dtype=torch.int32)
    for V in (0, 5):
        vd = torch.ones((V, 3), device=DEV)
        for call in (flip_edges, nondelaunay_edges):
            r = call(vd, f0)
            assert r.edge_vertices.shape == (0, 2) and r.edge_state.shape == (0,) and r.edge_opposite.shape == (0, 2)
            assert r.stats == dict(edges=0, nondelaunay=0, candidates=0, flipped=0, guarded=0)
        assert flip_edges(vd, f0).faces.shape == (0, 3) and flip_edges(vd, f0).face_flipped.shape == (0,)
        d = delaunay_flips(vd, f0)
        assert d.converged and d.faces.shape == (0, 3) and d.stats["rounds"] == 0
    f = np.array([[0, 1, 2], [3, 4, 5], [-1, 7, 2 ** 31 - 1], [0, 0, 0]])  # faces without vertices: nothing takes part, everything is still written
    want = _assert_round(np.zeros((0, 3), np.float32), f, what="V = 0")
    assert want["totals"] == [0, 0, 0, 0] and np.array_equal(want["out_faces"], f.astype(np.int32)) and not want["face_flipped"].any()


# ---- determinism and purity -------------------------------------------------------------------------------------------------------------------
def test_the_round_is_pure_and_deterministic():
    v, f = ref.stretched_grid(17, 17)
    keep = (np.random.default_rng(8).integers(0, 6, len(f)) != 0).astype(np.uint8)
    min_cos = ref.min_cos_of(30.0)

    def call(pattern):  # the workspace and every output come from torch.empty and are poisoned, with guard bytes either side
        out = {}
        for tag, k, classify_only in (("all", None, False), ("kept", keep, False), ("classified", keep, True)):
            got = _gpu_round(v, f, k, min_cos, 5, classify_only)
            out.update({f"{tag}.{n}": t for n, t in zip(NAMES + ("totals",), got) if t is not None})
        small = _gpu_round(ref.QUAD, [[0, 1, 2]], None, min_cos, 0, False)  # one slot of winners
        out.update({f"one.{n}": t for n, t in zip(NAMES + ("totals",), small)})
        return out

    base = poison.assert_pure(call)  # twice on zeros first: the same call repeated gives identical bytes
    want = ref.flip_round(v, f, keep, min_cos, 5)
    for name in NAMES:
        assert base[f"kept.{name}"].numpy().tobytes() == want[name].tobytes(), name
    assert base["classified.edge_state"].numpy().tobytes() == want["edge_state"].tobytes() and "classified.out_faces" not in base
    assert want["totals"][2] > want["totals"][3] > 0
