"""GPU tests of the triangle-overlap query (diff_recon_hip/mesh_overlap.py, libts_overlap.so) against tests/ref_mesh_overlap.py.

Tolerance: none.  + - x are correctly rounded on both sides and the unit is built with -ffp-contract=off, so every plane value and every
segment test is the reference's bit for bit; counts, stats and the sorted pair list are compared for equality."""
import functools

import numpy as np
import pytest
import torch

import poison
import ref_mesh_overlap as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 2, 8, 9, 65, 521)  # one lane; one leaf and one leaf plus one; a second wave; three levels
GENERATORS = {"soup": ref.soup, "sheets": ref.sheets}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases stay as the reference saw them


def _bvh(v, f, keep=None):
    from diff_recon_hip import MeshBVH
    return MeshBVH(_dev(v), _dev(f), None if keep is None else _dev(keep))


@functools.lru_cache(maxsize=None)
def _case(gen, F, seed=11):
    """(vertices, faces, the reference's answer in self mode), computed once and shared."""
    v, f = GENERATORS[gen](F, seed)
    return v, f, ref.overlap(v, f)


def _same(got, want, what, capacity=None):
    """A MeshOverlap against the reference's dict: every output."""
    stats = dict(want["stats"])
    if capacity is not None:
        stats["stored"] = min(stats["stored"], capacity)
    assert got.stats == stats, (what, got.stats, stats)
    assert np.array_equal(got.count.cpu().numpy(), want["count_a"]), what
    if want["count_b"] is None:
        assert got.count_b is None, what
    else:
        assert np.array_equal(got.count_b.cpu().numpy(), want["count_b"]), what
    if capacity is None:
        assert got.pairs.dtype == torch.int32 and got.kind.dtype == torch.uint8
        assert np.array_equal(got.pairs.cpu().numpy(), want["pairs"]), what
        assert np.array_equal(got.kind.cpu().numpy(), want["kind"]), what


@pytest.mark.parametrize("F", SIZES)
@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_self_mode_matches_brute_force(gen, F):
    v, f, want = _case(gen, F)
    got = _bvh(v, f).overlap()
    print(gen, F, got.stats)
    _same(got, want, f"{gen} F {F}")
    assert got.stats["stored"] == len(got.pairs) == got.stats["crossing"] + got.stats["coplanar"] + got.stats["duplicate"]


def test_the_large_cases_hold_every_kind():
    kinds = set()
    for gen in GENERATORS:
        kinds |= set(_case(gen, 521)[2]["kind"].tolist())
    assert kinds == {ref.KIND_CROSSING, ref.KIND_COPLANAR, ref.KIND_DUPLICATE}
    assert _case("sheets", 521)[2]["stats"]["degenerate"] > 0 and _case("sheets", 521)[2]["stats"]["adjacent"] > 0


def test_masks_nan_vertices_no_eligible_face_and_no_face():
    from diff_recon_hip import self_intersection_report, self_intersections
    v, f, _ = _case("soup", 521)
    keep = (np.arange(521) % 4 == 0)
    got = _bvh(v, f, keep.astype(np.uint8)).overlap()
    want = ref.overlap(v, f, keep)
    _same(got, want, "keep one in four")
    assert got.stats["degenerate"] == 521 - int(keep.sum()) and got.stats["crossing"] > 0
    bad = np.array(v)
    bad[f[5, 2]] = np.nan
    bad[f[300, 0], 1] = np.inf
    _same(_bvh(bad, f).overlap(), ref.overlap(bad, f), "NaN vertex")
    assert ref.overlap(bad, f)["stats"]["degenerate"] == 2
    none = _bvh(v, f, np.zeros(521, np.uint8)).overlap()
    _same(none, ref.overlap(v, f, np.zeros(521, bool)), "no eligible face")
    assert none.stats == dict(dict.fromkeys(ref.STATS_KEYS, 0), degenerate=521) and none.pairs.shape == (0, 2)
    out_of_range = np.array(f)
    out_of_range[7, 1] = 3 * 521
    out_of_range[8, 0] = -1
    _same(_bvh(v, out_of_range).overlap(), ref.overlap(v, out_of_range), "indices outside [0, V)")
    empty = self_intersections((_dev(v), _dev(np.zeros((0, 3), np.int32))))
    assert empty.stats == dict.fromkeys(ref.STATS_KEYS, 0) and empty.pairs.shape == (0, 2) and empty.count.shape == (0,)
    assert self_intersection_report((_dev(v), _dev(np.zeros((0, 3), np.int32)))) == {
        "faces": 0, "crossing_pairs": 0, "crossing_faces": 0, "coplanar_pairs": 0, "duplicate_pairs": 0, "degenerate_faces": 0}


def _raw_cross(a, b, with_count_b):
    """tsx_overlap itself, capacity 0: (count_a, count_b or None, stats)."""
    from diff_recon_hip import mesh_overlap
    count_a = torch.full((a.num_faces,), -7, device=DEV, dtype=torch.int32)
    count_b = torch.full((b.num_faces,), -7, device=DEV, dtype=torch.int32) if with_count_b else None
    stats = torch.full((8,), -7, device=DEV, dtype=torch.int64)
    rc = mesh_overlap._lib.tsx_overlap(a.num_faces, a.bvh.data_ptr(), a.bvh.numel(), None, b.num_faces, b.bvh.data_ptr(), b.bvh.numel(),
                                       count_a.data_ptr(), count_b.data_ptr() if with_count_b else None, stats.data_ptr(), 0, None, None, None, None)
    assert rc == 0, mesh_overlap._lib.tsx_last_error()
    return count_a.cpu().numpy(), count_b.cpu().numpy() if with_count_b else None, stats.cpu().tolist()


@pytest.mark.parametrize("FB", (8, 521))
@pytest.mark.parametrize("FA", (1, 9, 65))
def test_cross_mode_matches_brute_force_in_both_orders(FA, FB):
    from diff_recon_hip import mesh_intersections
    va, fa = ref.soup(FA, 3, edge=0.3)
    vb, fb = (ref.sheets if FB > 8 else ref.soup)(FB, 5)
    if FB == 521:  # a bad face on either side: degenerate counts both meshes
        fb = np.array(fb)
        fb[17, 1] = -1
    a, b = _bvh(va, fa), _bvh(vb, fb)
    for (x, vx, fx), (y, vy, fy) in (((a, va, fa), (b, vb, fb)), ((b, vb, fb), (a, va, fa))):
        want = ref.overlap(vx, fx, None, vy, fy)
        got = x.overlap(y)
        print(FA, FB, got.stats)
        _same(got, want, f"cross {len(fx)} x {len(fy)}")
        assert got.count_a is got.count
        ca, cb, st = _raw_cross(x, y, True)
        assert np.array_equal(ca, want["count_a"]) and np.array_equal(cb, want["count_b"])
        ca2, none, st2 = _raw_cross(x, y, False)
        assert none is None and np.array_equal(ca2, want["count_a"]) and st2 == st
        assert st == [want["stats"][k] for k in ref.STATS_KEYS[:6]] + [0, 0]
    assert ref.overlap(va, fa, None, vb, fb)["stats"]["candidates"] > 0 or FA == 1
    got = mesh_intersections((_dev(va), _dev(fa)), (_dev(vb), _dev(np.zeros((0, 3), np.int32))))   # F == 0 on either side: zeros
    assert got.stats == dict.fromkeys(ref.STATS_KEYS, 0) and not got.count.any() and got.count_b.shape == (0,)
    got = mesh_intersections((_dev(vb), _dev(np.zeros((0, 3), np.int32))), (_dev(va), _dev(fa)))
    assert got.stats == dict.fromkeys(ref.STATS_KEYS, 0) and got.count.shape == (0,) and not got.count_b.any()


def test_cross_mode_of_a_mesh_with_itself_pairs_every_face_with_itself():
    v, f, _ = _case("soup", 65)
    a = _bvh(v, f)
    got = a.overlap(_bvh(v, f))
    want = ref.overlap(v, f, None, v, f)
    _same(got, want, "soup against itself")
    # a face against itself: b0 = a0 has the plane value 0 exactly, the other two only up to rounding (the header's note on shared
    # vertices), so the pair is never apart; whether it reads as coplanar or as crossing is the reference's to say
    diag = got.pairs[:, 0] == got.pairs[:, 1]
    assert int(diag.sum()) == int((want["pairs"][:, 0] == want["pairs"][:, 1]).sum()) > 0


@pytest.mark.parametrize("name", sorted(ref.constructions()))
def test_constructions_give_the_geometric_answer(name):
    v, f, want_kind, want_stats = ref.constructions()[name]
    got = _bvh(v, f).overlap()
    _same(got, ref.overlap(v, f), name)
    assert got.kind.tolist() == ([want_kind] if want_kind else []) and got.pairs.tolist() == ([[0, 1]] if want_kind else [])
    assert got.count.tolist() == ([1, 1] if want_kind == 1 else [0, 0])
    for key, value in want_stats.items():
        assert got.stats[key] == value, (name, key, got.stats)


@pytest.mark.parametrize("solid", ["tetrahedron", "cube", "octahedron"])
def test_closed_convex_solids_have_no_pair(solid):
    v, f = getattr(ref, solid)()
    got = _bvh(v, f).overlap()
    _same(got, ref.overlap(v, f), solid)
    assert got.pairs.shape == (0, 2) and not got.count.any() and got.stats["adjacent"] == 3 * len(f) // 2


def test_overflow_keeps_counts_and_stats_exact_and_the_wrapper_calls_again():
    from diff_recon_hip import mesh_overlap
    v, f, want = _case("soup", 521)
    total = want["stats"]["stored"]
    assert total > 8
    bvh = _bvh(v, f)
    listed = {tuple(p): k for p, k in zip(want["pairs"].tolist(), want["kind"].tolist())}
    for capacity in (0, 1, total - 1, total):
        count, _, st, pairs, kind = mesh_overlap._query(bvh, None, capacity, None)
        assert st == [want["stats"][k] for k in ref.STATS_KEYS[:6]] + [min(total, capacity), 0], capacity
        assert np.array_equal(count.cpu().numpy(), want["count_a"]), capacity
        held = [tuple(p) for p in pairs[:min(total, capacity)].tolist()]
        assert len(set(held)) == len(held) and all(listed[p] == k for p, k in zip(held, kind.tolist())), capacity  # valid pairs, each once
    for capacity in (0, 1, total, None):  # the wrapper: one more call with the exact total where the list overflowed
        visits = torch.zeros(1, device=DEV, dtype=torch.int64)
        got = bvh.overlap(capacity=capacity, leaf_visits=visits)
        _same(got, want, f"capacity {capacity}")
    with pytest.raises(ValueError, match="capacity"):
        bvh.overlap(capacity=-1)


def test_sort_orders_by_first_then_second_and_carries_the_kinds():
    from diff_recon_hip import mesh_overlap
    lib = mesh_overlap._lib
    rng = np.random.default_rng(2)
    for P, hi_a, hi_b in ((1, 1, 1), (2, 2, 300), (1000, 521, 70000), (5000, 1 << 20, 3)):
        pairs = np.stack([rng.integers(0, hi_a, P), rng.integers(0, hi_b, P)], axis=1).astype(np.int32)
        kind = rng.integers(1, 4, P).astype(np.uint8)
        key = pairs[:, 0].astype(np.int64) * (1 << 32) + pairs[:, 1]
        kind = (key % 3 + 1).astype(np.uint8)  # a function of the pair: equal pairs carry equal kinds, so the sorted form is unique
        order = np.argsort(key, kind="stable")
        dp, dk = _dev(pairs), _dev(kind)
        ws = torch.empty(lib.tsx_sort_workspace_bytes(P), device=DEV, dtype=torch.uint8)
        rc = lib.tsx_sort_pairs(P, mesh_overlap._bits(hi_a), mesh_overlap._bits(hi_b), dp.data_ptr(), dk.data_ptr(), ws.data_ptr(), ws.numel(), None)
        assert rc == 0, lib.tsx_last_error()
        assert np.array_equal(dp.cpu().numpy(), pairs[order]) and np.array_equal(dk.cpu().numpy(), kind[order]), P


def test_two_distant_clusters_stay_in_their_own_leaves():
    va, fa = ref.soup(64, 21, edge=0.02, lo=0.0, hi=0.1)
    vb, fb = ref.soup(64, 22, edge=0.02, lo=0.9, hi=1.0)
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    assert va.min() >= 0.0 and va.max() <= 0.1 and vb.min() >= 0.9 and vb.max() <= 1.0
    visits = torch.zeros(1, device=DEV, dtype=torch.int64)
    got = _bvh(v, f).overlap(leaf_visits=visits)
    _same(got, ref.overlap(v, f), "two clusters")
    print("leaf visits of two clusters of 64 faces:", int(visits.item()), got.stats)
    assert 2 <= int(visits.item()) <= 16  # 16 leaves; each cluster is one wave, which can enter only its own 8
    across = (got.pairs[:, 0] < 64) != (got.pairs[:, 1] < 64)
    assert not across.any()


def _sphere_field(res, centre, radius):
    g = torch.arange(res, device=DEV, dtype=torch.float32) / (res - 1)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    d = [((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2).sqrt() - radius for c in centre]
    return torch.stack(d).amin(dim=0).contiguous()


def test_level_sets_do_not_cross_themselves_and_two_spheres_do():
    from diff_recon_hip import drop_intersecting_faces, extract_isosurface, intersecting_face_mask, mesh_topology, self_intersection_report, weld_mesh
    res, h = 14, 1.0 / 13
    c, r = (0.47, 0.51, 0.49), 0.31
    sv, sf = extract_isosurface(_sphere_field(res, [c], r), (0.0, 0.0, 0.0), h)
    one = weld_mesh(sv, sf, eps=0.0)
    report = self_intersection_report((one.vertices, one.faces))
    print("welded level set of a sphere:", report)
    assert report["faces"] == one.faces.shape[0] > 500 and report["crossing_pairs"] == 0 and report["crossing_faces"] == 0
    assert not intersecting_face_mask((one.vertices, one.faces)).any()
    # the same sphere and a copy shifted by half a radius, as one mesh
    shifted = one.vertices + torch.tensor([0.5 * r, 0.0, 0.0], device=DEV)
    v = torch.cat([one.vertices, shifted])
    f = torch.cat([one.faces, one.faces + one.vertices.shape[0]])
    colour = torch.arange(v.shape[0], device=DEV, dtype=torch.float32)[:, None].repeat(1, 3)
    got = _bvh(v.cpu().numpy(), f.cpu().numpy()).overlap()
    _same(got, ref.overlap(v.cpu().numpy(), f.cpu().numpy()), "two spheres")
    F = one.faces.shape[0]
    crossing = got.pairs[got.kind == ref.KIND_CROSSING]
    assert got.stats["crossing"] > 0 and ((crossing[:, 0] < F) & (crossing[:, 1] >= F)).all()  # every crossing is between the two copies
    mask = intersecting_face_mask((v, f))
    assert torch.equal(mask, got.count > 0) and 0 < int(mask.sum()) < 2 * F
    clean = drop_intersecting_faces((v, f), vertex_attributes=colour)
    assert torch.equal(clean.face_keep, ~mask) and clean.faces.shape[0] == 2 * F - int(mask.sum()) == clean.stats["num_faces"]
    assert torch.equal(clean.vertices[clean.faces.long()], v[f[clean.face_keep].long()])       # the same triangles, in their order
    assert torch.equal(clean.vertex_attributes, colour[clean.vertex_keep]) and torch.equal(clean.vertices, v[clean.vertex_keep])
    assert clean.stats["dropped_faces"] == int(mask.sum()) and clean.stats["crossing"] == got.stats["crossing"]
    assert self_intersection_report((clean.vertices, clean.faces))["crossing_pairs"] == 0
    assert mesh_topology(clean.vertices.shape[0], clean.faces)["boundary"] > 0                 # the holes it leaves are fill_holes' job


def test_purity_of_the_overlap_and_the_sort():
    """As tests/test_purity_gpu.py: the outputs, the list buffers and the sort's workspace come from a poisoned torch.empty between guard
    bands; what the calls specify is equal byte for byte whatever they held."""
    v, f, want = _case("sheets", 521)
    va, fa = ref.soup(65, 3, edge=0.3)
    total = want["stats"]["stored"]
    dv, df, dva, dfa = _dev(v), _dev(f), _dev(va), _dev(fa)

    def call(pattern):
        from diff_recon_hip import MeshBVH
        a, b = MeshBVH(dv, df), MeshBVH(dva, dfa)
        own = a.overlap()                      # overflows the first capacity or not: both calls are poisoned
        tight = a.overlap(capacity=total)
        short = a.overlap(capacity=3)          # the wrapper's second call
        cross = b.overlap(a)
        out = {}
        for name, r in (("own", own), ("tight", tight), ("short", short), ("cross", cross)):
            out.update({f"{name}.pairs": r.pairs, f"{name}.kind": r.kind, f"{name}.count": r.count, f"{name}.stats": tuple(sorted(r.stats.items()))})
        out["cross.count_b"] = cross.count_b
        return out

    base = poison.assert_pure(call)
    assert np.array_equal(base["own.pairs"].numpy().view(np.int32).reshape(-1, 2), want["pairs"])
    assert np.array_equal(base["tight.kind"].numpy(), want["kind"]) and np.array_equal(base["short.pairs"].numpy(), base["own.pairs"].numpy())


def test_every_refused_call_leaves_its_text_and_host_tensors_are_refused():
    from diff_recon_hip import mesh_overlap
    v, f, _ = _case("soup", 9)
    bvh = _bvh(v, f)
    lib = mesh_overlap._lib
    count = torch.zeros(9, device=DEV, dtype=torch.int32)
    stats = torch.zeros(8, device=DEV, dtype=torch.int64)
    rc = lib.tsx_overlap(9, bvh.bvh.data_ptr(), bvh.bvh.numel() - 1, bvh.faces.data_ptr(), 0, None, 0, count.data_ptr(), None, stats.data_ptr(), 0, None, None,
                         None, None)
    assert rc == 1 and b"bvh_a too small" in lib.tsx_last_error()
    rc = lib.tsx_overlap(9, bvh.bvh.data_ptr(), bvh.bvh.numel(), bvh.faces.data_ptr(), 0, None, 0, count.data_ptr(), None, stats.data_ptr(), 5, None, None,
                         None, None)
    assert rc == 1 and b"pairs/kind is null" in lib.tsx_last_error()
    with pytest.raises(RuntimeError, match="one HIP device"):
        bvh.overlap(leaf_visits=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError):
        bvh.overlap((_dev(v), _dev(f)))
