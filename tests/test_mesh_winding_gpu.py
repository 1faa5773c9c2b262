"""GPU tests of the generalised winding number (diff_recon_hip/mesh_winding.py, libts_winding.so) against tests/ref_mesh_winding.py.

Tolerance, derived (include/ts_winding.h): + - x / and sqrt are correctly rounded on both sides, so every accept decision, every node term
and every moment is bit-equal; only atan2 may differ, by a few ulp, which moves a quantised face term by at most one unit.  Hence
|wq_gpu - wq_ref| <= terms[:, 0] (the faces evaluated), the terms are equal exactly, a query that evaluated no face is equal bit for bit
and the moments buffer equals ref.moments bit for bit."""
import functools

import numpy as np
import pytest
import torch

import poison
import ref_mesh_distance as refd
import ref_mesh_inside as refi
import ref_mesh_surface as refs
import ref_mesh_winding as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TURN, HALF = 1 << 38, 1 << 37
INF = float("inf")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bvh(v, f, keep=None):
    from diff_recon_hip import MeshBVH
    return MeshBVH(_dev(v), _dev(f), None if keep is None else _dev(keep))


def _gwn(p, bvh, beta):
    from diff_recon_hip import generalized_winding_number
    w, wq, terms = generalized_winding_number(_dev(p), bvh, beta=beta, return_terms=True)
    assert w.dtype == torch.float64 and wq.dtype == torch.int64 and terms.dtype == torch.int32
    assert w.shape == wq.shape == (len(p),) and terms.shape == (len(p), 2)
    w, wq, terms = w.cpu().numpy(), wq.cpu().numpy(), terms.cpu().numpy()
    assert np.array_equal(np.isnan(w), wq == ref.BAD) and np.array_equal(w[wq != ref.BAD], wq[wq != ref.BAD] / 2.0 ** 38)
    return wq, terms


def _close(got, want, faces, what=""):
    diff = np.abs(got - want)
    print(f"{what}: largest |wq_gpu - wq_ref| = {int(diff.max()) if len(diff) else 0} units, faces evaluated up to {int(faces.max()) if len(faces) else 0}")
    bad = np.nonzero(diff > np.maximum(faces, 0))[0]
    assert not len(bad), (what, bad[:10], got[bad[:10]], want[bad[:10]], faces[bad[:10]])


@functools.lru_cache(maxsize=None)
def _soup(F):
    return refd.heavy_tailed_soup(F, seed=F)


@functools.lru_cache(maxsize=None)
def _grid(F):
    v, f = refs.grid_mesh(max(1, int(np.ceil(np.sqrt(F / 2)))), seed=F)
    return v, f[:F]


def _queries(Q, v, seed, reach=3.0):
    """Q points around the finite vertices: most within the box grown `reach` times (far enough for whole nodes to be accepted), every
    fourth close to a vertex."""
    rng = np.random.default_rng(seed)
    fin = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    p = mid + rng.uniform(-reach, reach, (Q, 3)) * half
    near = np.arange(Q) % 4 == 3
    p[near] = fin[rng.integers(0, len(fin), near.sum())] + rng.normal(size=(near.sum(), 3)) * 1e-3 * half
    return p.astype(np.float32)


def _tree_check(p, v, f, keep, betas, what):
    """The library on its own tree against the reference fed that tree's leaf-face table; returns (bvh, table)."""
    from diff_recon_hip import leaf_faces, winding_moments
    bvh = _bvh(v, f, keep)
    table = leaf_faces(bvh).cpu().numpy()
    eligible = refs.eligible_faces(v, f, keep)
    assert table.dtype == np.int32 and len(table) == 8 * ((len(f) + 7) // 8)
    assert np.array_equal(np.sort(table[table >= 0]), eligible) and (table[table < 0] == -1).all()  # a permutation of the eligible faces, and -1s
    got_m = winding_moments(bvh).cpu().numpy()
    want_m = ref.moments(v, f, table)
    assert got_m.shape == want_m.shape and np.array_equal(got_m.view(np.int64), want_m.view(np.int64)), what  # bit for bit
    for beta in betas:
        wq, terms = _gwn(p, bvh, beta)
        want, want_terms = ref.winding_tree(p, v, f, table, beta)
        assert np.array_equal(terms, want_terms), (what, beta, np.nonzero((terms != want_terms).any(axis=1))[0][:10])
        _close(wq, want, terms[:, 0], f"{what} beta {beta}")
        none = terms[:, 0] <= 0
        assert np.array_equal(wq[none], want[none])  # node terms only (or a bad point): bit for bit
    return bvh, table


# ---- parity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 8, 9, 65, 600])  # one leaf; one full leaf; two leaves; two levels; four levels (75 -> 10 -> 2 -> 1)
@pytest.mark.parametrize("Q", [1, 63, 65, 1000])
def test_exact_form_matches_brute_force(Q, F):
    for kind in (_soup, _grid):
        v, f = kind(F)
        assert len(f) == F
        p = _queries(Q, v, seed=Q + F, reach=1.5)
        wq, terms = _gwn(p, _bvh(v, f), INF)
        assert (terms[:, 0] == F).all() and (terms[:, 1] == 0).all()  # beta = inf accepts nothing: every face, whatever the tree
        _close(wq, ref.winding_exact(p, v, f), terms[:, 0], f"{kind.__name__} Q {Q} F {F}")


@pytest.mark.parametrize("F", [1, 8, 9, 65, 600])
@pytest.mark.parametrize("Q", [1, 63, 65, 1000])
def test_tree_form_matches_the_reference_on_the_librarys_own_tree(Q, F):
    accepted = 0
    for kind in (_soup, _grid):
        v, f = kind(F)
        p = _queries(Q, v, seed=3 * Q + F)
        bvh, _ = _tree_check(p, v, f, None, (1.0, 2.0, 3.0), f"{kind.__name__} Q {Q} F {F}")
        accepted += int(_gwn(p, bvh, 1.0)[1][:, 1].sum())
    assert Q < 63 or accepted > 0  # the far field was used


def test_exact_form_on_masks_ineligible_and_zero_area_faces_and_queries_on_the_mesh():
    v, f = _grid(600)
    v, f = v.copy(), f.copy()
    rng = np.random.default_rng(4)
    f[5] = (0, 1, len(v))            # an index out of range
    f[6] = (-1, 2, 3)
    v[f[7, 0]] = np.nan              # a non-finite vertex takes every face at it out
    f[8] = (f[8, 0], f[8, 0], f[8, 1])   # zero area: an edge
    f[9] = (f[9, 0],) * 3                # zero area: a point
    keep = rng.random(600) < 0.7
    eligible = refs.eligible_faces(v, f, keep)
    assert 350 < len(eligible) < 500 and 8 in refs.eligible_faces(v, f) and 5 not in refs.eligible_faces(v, f)
    tri = v[f[eligible[:200]]].astype(np.float64)
    on_vertex = v[np.isfinite(v).all(axis=1)][:200]
    on_edge = (0.5 * tri[:, 0] + 0.5 * tri[:, 1]).astype(np.float32)
    in_face = tri.mean(axis=1).astype(np.float32)
    flat_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    flat_f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    in_plane = np.array([[0.25, 0.25, 0], [0.75, 0.75, 0], [0.5, 0.5, 0], [3, 3, 0], [0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 1]], np.float32)
    for keep_ in (keep, None):
        p = np.concatenate([on_vertex, on_edge, in_face, _queries(200, v, 9, reach=1.2)])
        for beta in (INF, 2.0):
            wq, terms = _gwn(p, _bvh(v, f, keep_), beta)
            if beta == INF:
                assert (terms[:, 0] == len(refs.eligible_faces(v, f, keep_))).all()
                _close(wq, ref.winding_exact(p, v, f, keep_), terms[:, 0], "masked grid, exact")
        _tree_check(p, v, f, keep_, (2.0,), "masked grid")
    wq, terms = _gwn(in_plane, _bvh(flat_v, flat_f), INF)
    want = ref.winding_exact(in_plane, flat_v, flat_f)
    assert want[:6].tolist() == [0] * 6 and np.array_equal(wq[:6], want[:6])  # det == 0 exactly: the face counts nothing, on both sides
    _close(wq, want, terms[:, 0], "in the plane")


def test_coordinates_near_the_fp32_range_stay_finite():
    v, f = _soup(65)
    scale = np.float32(3e38) / np.abs(v).max()
    big = (v * scale).astype(np.float32)
    assert np.isfinite(big).all() and np.abs(big).max() > 2.9e38
    p = np.concatenate([(_queries(100, v, 1, reach=1.0) * scale).astype(np.float32), big[:30]])
    p = np.clip(p, -3.4e38, 3.4e38).astype(np.float32)
    wq, terms = _gwn(p, _bvh(big, f), INF)
    _close(wq, ref.winding_exact(p, big, f), terms[:, 0], "near the fp32 range, exact")
    _tree_check(p, big, f, None, (1.0, 2.0), "near the fp32 range")
    tiny = (v * np.float32(1e-30)).astype(np.float32)
    q = (_queries(100, v, 2, reach=2.0) * np.float32(1e-30)).astype(np.float32)
    _tree_check(q, tiny, f, None, (INF, 2.0), "tiny coordinates")


# ---- closed meshes -----------------------------------------------------------------------------------------------------------------------------
def test_closed_meshes_count_whole_turns():
    rng = np.random.default_rng(11)
    p = rng.uniform(-1.6, 1.6, (1000, 3)).astype(np.float32)
    inside = (np.abs(p) < 1).all(axis=1)
    assert 150 < inside.sum() < 400
    cube = refi.cube()
    for name, (v, f), k in (("cube", cube, 1), ("doubled", refi.join(cube, cube), 2), ("inside out", refi.cube(reverse=True), -1),
                            ("gridded", ref.cube_grid(7), 1)):
        wq, terms = _gwn(p, _bvh(v, f), INF)
        F = len(f)
        assert F == {"cube": 12, "doubled": 24, "inside out": 12, "gridded": 588}[name] and (terms[:, 0] == F).all()
        worst_in, worst_out = np.abs(wq[inside] - k * TURN).max(), np.abs(wq[~inside]).max()
        print(f"{name}: exact wq within {worst_in} units of {k} turn(s) inside, {worst_out} of 0 outside (bound F = {F})")
        assert worst_in <= F and worst_out <= F


@pytest.mark.parametrize("drop", [False, True])
def test_far_field_decides_like_the_exact_sum_away_from_the_threshold(drop):
    """The gridded cube, closed and without its bottom, on the 16^3 grid over [-1.6, 1.6]^3: w_beta >= 1/2 equals w_exact >= 1/2 wherever
    |w_exact - 1/2| >= m, m twice the largest deviation that the REFERENCE's tree form shows from the reference's exact form on the
    library's own leaf order; the samples left out are at most 5 %."""
    from diff_recon_hip import leaf_faces
    v, f = ref.cube_grid(7, drop)
    assert len(f) == (490 if drop else 588)
    p = refi.grid_points((-1.6, -1.6, -1.6), 3.2 / 15, (16, 16, 16))
    bvh = _bvh(v, f)
    table = leaf_faces(bvh).cpu().numpy()
    exact_ref = ref.to_turns(ref.winding_exact(p, v, f))
    exact, _ = _gwn(p, bvh, INF)
    for beta in (1.5, 2.0, 3.0):
        deviation = np.abs(ref.to_turns(ref.winding_tree(p, v, f, table, beta)[0]) - exact_ref).max()
        m = 2 * deviation
        judged = np.abs(exact_ref - 0.5) >= m
        wq, terms = _gwn(p, bvh, beta)
        print(f"{'open' if drop else 'closed'} gridded cube, beta {beta}: reference deviation {deviation:.3g}, left out {100 * (1 - judged.mean()):.2f} %, "
              f"gpu max |w_beta - w_exact| {np.abs(wq - exact).max() / TURN:.3g}, mean faces {terms[:, 0].mean():.1f}, mean nodes {terms[:, 1].mean():.1f}")
        assert 1 - judged.mean() <= 0.05
        assert np.array_equal((wq >= HALF)[judged], (exact >= HALF)[judged])
        assert terms[:, 1].sum() > 0 and terms[:, 0].mean() < len(f)  # and it is an approximation that saves work


# ---- the point of the feature --------------------------------------------------------------------------------------------------------------------
def _open_cube():
    v, f = refi.cube()
    keep = ~(v[f][:, :, 2] == -1).all(axis=1)
    assert keep.sum() == 10
    return v, f[keep]


GRID = ((-1.6, -1.6, -1.6), 3.2 / 23, (24, 24, 24))


def test_the_open_cube_gets_a_signed_distance_volume_a_closed_remesh_and_an_iou_of_one():
    from diff_recon_hip import (contains_points, mesh_to_sdf, mesh_to_sdf_winding, mesh_topology, mesh_volume_iou, remesh, remesh_winding,
                                signed_distance)
    v, f = _open_cube()
    mesh = (_dev(v), _dev(f))
    p = refi.grid_points(*GRID)
    strictly_in = (np.abs(p) < 1).all(axis=1)
    field = mesh_to_sdf_winding(mesh, *GRID)
    assert field.shape == (24, 24, 24) and field.dtype == torch.float32
    sdf = field.cpu().numpy().reshape(-1)
    assert not np.isnan(sdf).any()
    assert strictly_in.sum() == 14 ** 3 and np.array_equal(sdf < 0, strictly_in)        # exactly the samples inside the cube
    idx = np.indices((24, 24, 24)).reshape(3, -1)
    border = ((idx == 0) | (idx == 23)).any(axis=0)
    assert (sdf[border] > 0).all()
    want_d = np.sqrt(refs.closest(p[::7], v, f)[1]).astype(np.float32)                   # the magnitude is the closest-point distance
    assert np.array_equal(np.abs(sdf[::7]), want_d)
    via, _, decided = signed_distance(_dev(p), mesh, method="winding")                  # the keyword of mesh_inside.py is the same path
    assert bool(decided.all()) and np.array_equal(via.cpu().numpy(), sdf)
    inside, decided = contains_points(_dev(p), mesh, method="winding")
    assert bool(decided.all()) and np.array_equal(inside.cpu().numpy(), strictly_in)
    rays = mesh_to_sdf(mesh, *GRID).cpu().numpy().reshape(-1)                            # the contrast: rays see an open sheet
    assert np.isnan(rays).any() or not np.array_equal(rays < 0, strictly_in)

    again = remesh_winding(mesh, 24, pad_voxels=2.5)  # half a voxel off: no sample plane lies in the plane of the hole, where w is 1/2
    topo = mesh_topology(again.vertices.shape[0], again.faces)
    print("remesh_winding(open cube, 24):", topo, {k: again.stats[k] for k in ("dims", "voxel_size", "undecided", "inside", "method")})
    assert topo["faces"] > 100 and topo["boundary"] == 0 and topo["pieces"] == 1 and topo["euler"] == 2 and again.stats["undecided"] == 0
    by_rays = remesh(mesh, 24, pad_voxels=2.5)
    topo_rays = mesh_topology(by_rays.vertices.shape[0], by_rays.faces)
    print("remesh(open cube, 24), rays:", topo_rays)
    assert topo_rays["boundary"] > 0

    closed = refi.cube()
    res = mesh_volume_iou(mesh, (_dev(closed[0]), _dev(closed[1])), None, origin=GRID[0], voxel_size=GRID[1], dims=GRID[2], method="winding")
    print("mesh_volume_iou(open cube, cube, winding):", res)
    assert res["iou"] == 1.0 and res["inside_a"] == res["inside_b"] == res["inside_both"] == res["inside_either"] == 14 ** 3 and res["undecided"] == 0


# ---- bad and empty inputs, the sign-distance call ------------------------------------------------------------------------------------------------
def test_bad_points_no_faces_and_no_points():
    from diff_recon_hip import contains_points_winding, generalized_winding_number, leaf_faces, signed_distance_winding, winding_moments
    v, f = refi.cube()
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [3, 0, 0], [0, 0, -np.inf]], np.float32)
    bad = np.array([False, True, True, False, True])
    for beta in (INF, 2.0):
        wq, terms = _gwn(p, _bvh(v, f), beta)
        assert (wq[bad] == ref.BAD).all() and (terms[bad] == -1).all() and abs(wq[0] - TURN) <= 12 and abs(wq[3]) <= 12
    inside, decided = contains_points_winding(_dev(p), (_dev(v), _dev(f)))
    assert inside.cpu().tolist() == [True, False, False, False, False] and decided.cpu().tolist() == (~bad).tolist()
    sdf, face, decided = signed_distance_winding(_dev(p), (_dev(v), _dev(f)))
    assert sdf.cpu().numpy()[[0, 3]].tolist() == [-1.0, 2.0] and np.isnan(sdf.cpu().numpy()[bad]).all() and decided.cpu().tolist() == (~bad).tolist()
    assert face.cpu().numpy()[bad].tolist() == [-1, -1, -1]
    # no face at all, and none eligible
    for mesh in ((v, np.zeros((0, 3), np.int32), None), (v, f, np.zeros(12, bool))):
        bvh = _bvh(*mesh)
        wq, terms = _gwn(p, bvh, 2.0)
        assert (wq[~bad] == 0).all() and (terms[~bad] == 0).all() and (wq[bad] == ref.BAD).all() and (terms[bad] == -1).all()
        assert winding_moments(bvh).shape == (3 if len(mesh[1]) else 0, 8) and (leaf_faces(bvh) == -1).all()
        sdf, _, decided = signed_distance_winding(_dev(p), bvh)
        assert np.isnan(sdf.cpu().numpy()).all() and not bool(decided.any())  # no distance: nothing to sign
    # no point
    w, wq, terms = generalized_winding_number(_dev(np.zeros((0, 3), np.float32)), (_dev(v), _dev(f)), return_terms=True)
    assert w.shape == wq.shape == (0,) and terms.shape == (0, 2)
    sdf, face, decided = signed_distance_winding(_dev(np.zeros((0, 3), np.float32)), (_dev(v), _dev(f)))
    assert sdf.shape == face.shape == decided.shape == (0,)
    for beta in (0.5, float("nan")):
        with pytest.raises(ValueError):
            generalized_winding_number(_dev(p), (_dev(v), _dev(f)), beta=beta)


def test_sign_distance_cases_of_the_header():
    from diff_recon_hip import mesh_winding
    d2 = np.array([0.0, 0.0, 4.0, 4.0, 4.0, 2.0, np.nan, np.inf, 9.0, 1e-300], np.float64)
    wq = np.array([TURN, ref.BAD, HALF, HALF - 1, -TURN, TURN, TURN, TURN, ref.BAD, HALF + 1], np.int64)
    out, decided = torch.empty(10, device=DEV, dtype=torch.float32), torch.empty(10, device=DEV, dtype=torch.uint8)
    dd2, dwq = _dev(d2), _dev(wq)
    rc = mesh_winding._lib.tsn_sign_distance(10, dd2.data_ptr(), dwq.data_ptr(), HALF, out.data_ptr(), decided.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    want = np.array([0.0, 0.0, -2.0, 2.0, 2.0, -np.sqrt(2.0), np.nan, np.nan, np.nan, -np.sqrt(1e-300)], np.float64).astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.where(np.isnan(want), np.float32(np.nan), want).view(np.uint32))  # +0, and 0x7FC00000
    assert decided.cpu().tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 1]
    out2 = torch.empty(10, device=DEV, dtype=torch.float32)
    assert mesh_winding._lib.tsn_sign_distance(10, dd2.data_ptr(), dwq.data_ptr(), -TURN, out2.data_ptr(), decided.data_ptr(), None) == 0
    assert out2.cpu().numpy()[[3, 4]].tolist() == [-2.0, -2.0]  # the threshold is the caller's


def test_every_refused_call_leaves_its_text():
    from diff_recon_hip import leaf_faces, mesh_winding, winding_moments
    lib = mesh_winding._lib
    v, f = refi.cube()
    bvh = _bvh(v, f)
    m, p = winding_moments(bvh), _dev(np.zeros((4, 3), np.float32))
    wq = torch.empty(4, device=DEV, dtype=torch.int64)
    ws = torch.empty(lib.tsn_winding_workspace_bytes(4), device=DEV, dtype=torch.uint8)

    def call(beta=2.0, F=12, bvh_bytes=bvh.bvh.numel(), m_bytes=m.numel() * 8, ws_bytes=ws.numel()):
        return lib.tsn_winding(4, p.data_ptr(), beta, F, bvh.bvh.data_ptr(), bvh_bytes, m.data_ptr(), m_bytes, wq.data_ptr(), None, ws.data_ptr(),
                               ws_bytes, None)

    assert call() == 0
    for kw, code, word in ((dict(beta=0.5), 1, b"at least 1"), (dict(beta=float("nan")), 1, b"NaN"), (dict(F=1 << 24), 3, b"must not wrap"),
                           (dict(bvh_bytes=bvh.bvh.numel() - 1), 1, b"bvh too small"), (dict(m_bytes=m.numel() * 8 - 1), 1, b"moments too small"),
                           (dict(ws_bytes=ws.numel() - 1), 1, b"workspace too small")):
        assert call(**kw) == code and word in lib.tsn_last_error(), kw
    short = torch.empty(leaf_faces(bvh).numel() - 1, device=DEV, dtype=torch.int32)
    assert lib.tsn_moments(12, bvh.bvh.data_ptr(), bvh.bvh.numel(), m.data_ptr(), m.numel() * 8, short.data_ptr(), short.numel() * 4, None) == 1
    assert b"leaf_faces too small" in lib.tsn_last_error()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="one HIP device"):
        mesh_winding.generalized_winding_number(torch.zeros(2, 3), bvh)


# ---- the keyword, the defaults, the order --------------------------------------------------------------------------------------------------------
def test_method_rays_is_the_default_and_winding_takes_no_rule():
    from diff_recon_hip import contains_points, mesh_volume_iou, signed_distance
    v, f = refi.cube()
    mesh = (_dev(v), _dev(f))
    p = _dev(np.random.default_rng(3).uniform(-1.5, 1.5, (500, 3)).astype(np.float32))
    for rule in refi.RULES:
        for a, b in zip(contains_points(p, mesh, rule), contains_points(p, mesh, rule, method="rays")):
            assert torch.equal(a, b)
        for a, b in zip(signed_distance(p, mesh, rule), signed_distance(p, mesh, rule, method="rays", beta=3.0)):
            assert torch.equal(a, b)
    assert mesh_volume_iou(mesh, mesh, 16) == mesh_volume_iou(mesh, mesh, 16, method="rays")
    # on a closed mesh both methods say the same
    for a, b in zip(contains_points(p, mesh), contains_points(p, mesh, method="winding")):
        assert torch.equal(a, b)
    assert torch.equal(signed_distance(p, mesh)[0], signed_distance(p, mesh, method="winding", beta=INF)[0])
    for fn in (contains_points, signed_distance):
        with pytest.raises(ValueError):
            fn(p, mesh, rule="odd", method="winding")
        with pytest.raises(ValueError):
            fn(p, mesh, method="scanline")
    with pytest.raises(ValueError):
        mesh_volume_iou(mesh, mesh, 16, method="scanline")


def test_results_do_not_depend_on_the_order_or_the_company_of_the_points_and_the_tree_is_the_same_every_time():
    from diff_recon_hip import MeshBVH, leaf_faces, winding_moments
    v, f = _soup(600)
    p = _queries(1000, v, 8)
    a, b = _bvh(v, f), _bvh(v, f)
    assert torch.equal(leaf_faces(a), leaf_faces(b)) and torch.equal(winding_moments(a).view(torch.int64), winding_moments(b).view(torch.int64))
    assert winding_moments(a) is winding_moments(a) and isinstance(a, MeshBVH)  # built once, kept on the index
    wq, terms = _gwn(p, a, 2.0)
    perm = np.random.default_rng(0).permutation(1000)
    wq2, terms2 = _gwn(p[perm], b, 2.0)
    assert np.array_equal(wq2, wq[perm]) and np.array_equal(terms2, terms[perm])
    alone, terms3 = _gwn(p[:37], a, 2.0)   # other neighbours in the wave: the same sums
    assert np.array_equal(alone, wq[:37]) and np.array_equal(terms3, terms[:37])
    w, wq4 = a.winding_number(_dev(p))
    assert np.array_equal(wq4.cpu().numpy(), wq)


# ---- purity ----------------------------------------------------------------------------------------------------------------------------------------
def test_moments_winding_and_sign_distance_are_pure():
    """Workspace, moments, leaf_faces and every output start out poisoned (tests/poison.py); the results do not change and no guard byte
    around a buffer of exactly its size query is written."""
    from diff_recon_hip import MeshBVH, generalized_winding_number, leaf_faces, signed_distance_winding, winding_moments
    v, f = _soup(65)
    keep = np.arange(65) % 5 != 0
    p = _queries(300, v, 6)
    p[17] = np.nan
    dv, df, dk, dp = _dev(v), _dev(f), _dev(keep), _dev(p)

    def call(pattern):
        bvh = MeshBVH(dv, df, dk)
        out = {"moments": winding_moments(bvh), "leaf_faces": leaf_faces(bvh)}
        for beta in (2.0, INF):
            _, wq, terms = generalized_winding_number(dp, bvh, beta=beta, return_terms=True)
            out[f"wq{beta}"], out[f"terms{beta}"] = wq, terms
        out["sdf"], out["face"], out["decided"] = signed_distance_winding(dp, bvh)
        return out

    base = poison.assert_pure(call)
    assert len(base["moments"]) == 8 * 8 * (9 + 2 + 1) and len(base["leaf_faces"]) == 4 * 72


# ---- example ---------------------------------------------------------------------------------------------------------------------------------------
def test_example_remeshes_its_open_fused_mesh_without_boundary_edges():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    r = train_synthetic.mesh_scores(m, "2D", extract=32, remesh=40, remesh_method="winding", **cfg)["fused"]["remeshed"]
    lines = train_synthetic.remeshed_report(r)
    print("\n".join(lines))
    assert r is not None and r["method"] == "winding" and r["undecided"] == 0 and r["inside"] > 0
    assert r["topology"]["faces"] > 0 and r["topology"]["boundary"] == 0  # a level set of a field without NaN that is positive at the border
    assert len(lines) == 2 and "signed by the generalised winding number" in lines[0]
    with pytest.raises(ValueError):
        train_synthetic.mesh_scores(m, "2D", extract=32, remesh=40, remesh_method="scanline", **cfg)
