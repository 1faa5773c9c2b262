"""Every enqueuing entry point of the mesh and geometry headers, captured in a graph and replayed against eager runs (tests/replay.py;
DESIGN.md "Stream order of the mesh entry points").  One test per header; chains of calls go into one graph, the later call reading the
device outputs of the earlier one at their documented capacity, with no host step between.  Two sizes per unit: one that spans at least
two 2048-element tiles of ts_mesh_scan.h (3 F > 2048), and the smallest table the unit accepts, where A and B differ in whether the one
face takes part.  Every comparison is raw bytes, to the capacity of every output, totals included."""
import numpy as np
import pytest
import torch

import ref_mesh_flip
import ref_mesh_manifold
import ref_mesh_subdivide
import replay
from test_mesh_smooth_gpu import _latlong_sphere
from test_replay_cpu import check_positive_controls

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPLAYS = len(replay.SEQUENCE) * len(replay.PATTERNS)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _mesh(v, f, keep=None, **more):
    """The inputs of one case: vertices (V, 3) float32, faces (F, 3) int32, keep (F,) uint8, and whatever else the unit reads."""
    f = np.asarray(f).reshape(-1, 3)
    case = {"v": _dev(np.asarray(v, np.float32).reshape(-1, 3)), "f": _dev(f.astype(np.int32)),
            "keep": _dev(np.ones(len(f), np.uint8) if keep is None else np.asarray(keep, np.uint8))}
    case.update({k: _dev(x) for k, x in more.items()})
    return case


def _i64(snapshot, name):
    return snapshot[name].view(torch.int64).tolist()


def _check(call, a, b, differ, outputs=None):
    base_a, base_b, n = replay.assert_replays(call, a, b, outputs=outputs, differ=differ)
    assert n == REPLAYS
    return base_a, base_b


# ---- the fixtures: the units' own, at the two sizes ---------------------------------------------------------------------------------------------
def _punched(keep_every, F, first=0):
    keep = np.ones(F, np.uint8)
    keep[first::keep_every] = 0
    return keep


def grid_pair():
    """A 20 x 20 sheared grid (V = 441, F = 800, 3 F = 2400 > 2048): A whole; B the grid of another seed with every 7th face dropped, so
    edge, boundary, loop and flip counts all differ."""
    va, f = ref_mesh_flip.sheared_grid(20, 20)
    vb, fb = ref_mesh_flip.sheared_grid(20, 20, seed=5)
    assert np.array_equal(f, fb) and len(f) == 800 and not np.array_equal(va, vb)
    return _mesh(va, f), _mesh(vb, f, _punched(7, 800, 3))


def sphere_pair():
    """The lat-long sphere of the smoothing tests at 20 rings of 24 segments (V = 458, F = 912, 3 F = 2736 > 2048): closed (A); scaled,
    jittered and with every 11th face dropped (B)."""
    v, f = _latlong_sphere(rings=20, segments=24)
    assert len(f) == 912
    rng = np.random.default_rng(11)
    vb = (v * np.float32(1.25) + rng.uniform(-0.004, 0.004, v.shape)).astype(np.float32)
    return _mesh(v, f), _mesh(vb, f, _punched(11, len(f), 5))


def one_face_pair(**more):
    """The smallest table: one face, which takes part in A and is dropped in B."""
    q = ref_mesh_flip.QUAD[:3]
    return _mesh(q, [[0, 1, 2]], [1], **more), _mesh(q[::-1] * np.float32(0.5), [[0, 1, 2]], [0], **more)


# ---- the harness rejects what it must, on the device -----------------------------------------------------------------------------------------------
def test_positive_controls_on_the_device():
    check_positive_controls(DEV)
    a, b = replay.control_cases(DEV)
    other = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    unit = replay.other_stream_unit(other)
    with pytest.raises(replay.ReplayMismatch, match=r"replay 1 of 4 \(inputs A, captured on B, poison ones.*out: "):
        replay.assert_replays(unit, a, b)
    torch.cuda.synchronize(DEV)


# ---- ts_smooth.h: tss_adjacency -> tss_smooth; tss_face_normals; tss_vertex_normals --------------------------------------------------------------
def smooth_call(inputs):
    from diff_recon_hip import mesh_smooth
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_smooth._lib
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    V, F = v.shape[0], f.shape[0]
    offsets, neighbors, edge_faces, cls, counts = mesh_smooth._adjacency_arrays(V, f, keep, DEV)
    smoothed = torch.empty((V, 3), device=DEV, dtype=torch.float32)
    ws = mesh_smooth._workspace(V, 0, DEV)
    # the table at its capacity of 6 F entries, not trimmed to counts[0]: the rows are cut by offsets
    mesh_smooth._check(lib.tss_smooth(V, v.data_ptr(), offsets.data_ptr(), neighbors.data_ptr(), edge_faces.data_ptr(), 6 * F, cls.data_ptr(),
                                      inputs["pinned"].data_ptr(), 0.5, -0.53, 3, mesh_smooth.BOUNDARY_MODES["curve"], 0.05, smoothed.data_ptr(),
                                      ws.data_ptr(), ws.numel(), native.stream()), "tss_smooth")
    face_normal = torch.empty((F, 3), device=DEV, dtype=torch.float32)
    face_valid = torch.empty((F,), device=DEV, dtype=torch.uint8)
    mesh_smooth._check(lib.tss_face_normals(V, F, v.data_ptr(), f.data_ptr(), keep.data_ptr(), face_normal.data_ptr(), face_valid.data_ptr(),
                                            native.stream()), "tss_face_normals")
    out = {"offsets": offsets, "neighbors": neighbors, "edge_faces": edge_faces, "vertex_class": cls, "counts": counts, "smoothed": smoothed,
           "face_normal": face_normal, "face_valid": face_valid}
    for name, weighting in mesh_smooth.NORMAL_WEIGHTINGS.items():
        normal = torch.empty((V, 3), device=DEV, dtype=torch.float32)
        valid = torch.empty((V,), device=DEV, dtype=torch.uint8)
        sums = torch.empty((V, 3), device=DEV, dtype=torch.float64)
        ws = mesh_smooth._workspace(V, F, DEV)
        mesh_smooth._check(lib.tss_vertex_normals(V, F, v.data_ptr(), f.data_ptr(), keep.data_ptr(), weighting, normal.data_ptr(), valid.data_ptr(),
                                                  sums.data_ptr(), ws.data_ptr(), ws.numel(), native.stream()), "tss_vertex_normals")
        out.update({f"vertex_normal_{name}": normal, f"vertex_valid_{name}": valid, f"normal_sum_{name}": sums})
    return out


def _pinned(case, seed):
    V = case["v"].shape[0]
    case["pinned"] = _dev((np.random.default_rng(seed).integers(0, 6, V) == 0).astype(np.uint8))
    return case


def test_ts_smooth_h():
    a, b = sphere_pair()
    base_a, base_b = _check(smooth_call, _pinned(a, 1), _pinned(b, 2), differ=("counts", "smoothed", "face_valid"))
    F = a["f"].shape[0]
    assert _i64(base_a, "counts") == [3 * F, 0, 3 * F, 0] and _i64(base_b, "counts")[1] > 0  # closed; B has boundary entries
    a, b = one_face_pair()
    base_a, base_b = _check(smooth_call, _pinned(a, 1), _pinned(b, 1), differ=("counts", "face_valid"))
    assert _i64(base_a, "counts") == [6, 6, 0, 0] and _i64(base_b, "counts") == [0, 0, 0, 0]


# ---- ts_holes.h: tss_adjacency -> tsh_loops -> tsh_fill ------------------------------------------------------------------------------------------
def holes_call(inputs):
    from diff_recon_hip import mesh_holes, mesh_smooth
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    V, F = v.shape[0], f.shape[0]
    offsets, neighbors, edge_faces, _, adjacency_counts = mesh_smooth._adjacency_arrays(V, f, keep, DEV)
    half_edge_loop, loop_offsets, loop_half_edges, counts = mesh_holes._loops_arrays(V, f, keep, offsets, neighbors, edge_faces, 6 * F, DEV)
    # the documented bounds as capacities: at most F loops and 3 F members; the loops past their number are empty (TSH_DEAD, nothing emitted)
    fill = mesh_holes._fill_arrays(v, f, loop_offsets, loop_half_edges, F, 3 * F, 8, inputs["attributes"], inputs["attr_valid"], DEV)
    names = ("loop_status", "new_vertices", "new_attributes", "new_attr_valid", "new_faces", "new_face_loop", "totals")
    return {"adjacency_counts": adjacency_counts, "half_edge_loop": half_edge_loop, "loop_offsets": loop_offsets,
            "loop_half_edges": loop_half_edges, "counts": counts, **dict(zip(names, fill))}


def _attributes(case, seed):
    V = case["v"].shape[0]
    rng = np.random.default_rng(seed)
    case["attributes"] = _dev(rng.uniform(0, 1, (V, 3)).astype(np.float32))
    case["attr_valid"] = _dev(rng.integers(0, 2, V).astype(np.uint8))
    return case


def test_ts_holes_h():
    a, b = sphere_pair()
    a["keep"][40::97] = 0  # A has holes of three of its own; B's dropped faces are other ones and more
    base_a, base_b = _check(holes_call, _attributes(a, 3), _attributes(b, 4), differ=("counts", "totals", "loop_offsets", "new_faces"))
    (_, _, loops_a, _), (_, _, loops_b, _) = _i64(base_a, "counts"), _i64(base_b, "counts")
    assert 0 < loops_a < loops_b and _i64(base_a, "totals")[0] == loops_a and _i64(base_b, "totals")[0] > 0
    a, b = grid_pair()  # the outline of the grid is a loop of 80, longer than the limit of 8: TSH_TOO_LONG in both
    b["keep"] = _dev(_punched(37, 800, 45))  # sparse enough for the holes to stay apart: 17 loops of three beside the outline's open chains
    base_a, base_b = _check(holes_call, _attributes(a, 5), _attributes(b, 6), differ=("counts", "totals"))
    assert _i64(base_a, "counts")[:3] == [80, 80, 1] and _i64(base_a, "totals") == [0, 0, 0] and _i64(base_b, "totals")[0] > 0
    a, b = one_face_pair()
    base_a, base_b = _check(holes_call, _attributes(a, 7), _attributes(b, 7), differ=("counts", "loop_status"))
    assert _i64(base_a, "counts") == [3, 3, 1, 0] and _i64(base_b, "counts") == [0, 0, 0, 0]  # the lone face's outline against nothing


# ---- ts_manifold.h: tsf_fans -> tsf_split -----------------------------------------------------------------------------------------------------------
def manifold_call(inputs):
    from diff_recon_hip import mesh_manifold
    f, keep = inputs["f"], inputs["keep"]
    V, F = inputs["v"].shape[0], f.shape[0]
    corner_fan, vertex_fans, counts = mesh_manifold._fans_arrays(V, f, keep, DEV)
    out_faces, source, label, totals = mesh_manifold._split_arrays(V, f, keep, corner_fan, 3 * F, DEV)  # 3 F: no more corners than that
    return {"corner_fan": corner_fan, "vertex_fans": vertex_fans, "counts": counts, "out_faces": out_faces, "new_vertex_source": source,
            "new_vertex_fan": label, "totals": totals}


def test_ts_manifold_h():
    _, grid = ref_mesh_flip.sheared_grid(20, 20)
    Vh, hub = ref_mesh_manifold.hub(40)  # 40 lone triangles on vertex 0: 39 new vertices
    f = np.concatenate([grid + Vh, hub, [[Vh, Vh + 1, 5], [Vh + 30, Vh + 31, 7]]]).astype(np.int32)  # ... and two faces that bridge both
    V = Vh + 441
    v = np.zeros((V, 3), np.float32)
    keep_b = _punched(5, len(f), 2)
    keep_b[800:820] = 0  # half of the hub
    base_a, base_b = _check(manifold_call, _mesh(v, f), _mesh(v, f[::-1].copy(), keep_b[::-1].copy()), differ=("counts", "totals"))
    assert _i64(base_a, "totals")[0] >= 39 and 0 < _i64(base_b, "totals")[0] < _i64(base_a, "totals")[0]
    a, b = one_face_pair()
    base_a, base_b = _check(manifold_call, a, b, differ=("counts", "corner_fan"))
    assert _i64(base_a, "counts")[:2] == [3, 3] and _i64(base_b, "counts") == [0] * 6 and _i64(base_a, "totals") == [0, 0]


# ---- ts_subdivide.h: tsd_edges -> tsd_split ---------------------------------------------------------------------------------------------------------
def subdivide_call(inputs):
    from diff_recon_hip import mesh_subdivide
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    edges = mesh_subdivide._edges_arrays(v.shape[0], f, keep, v, DEV)
    out = dict(zip(("edge_vertices", "edge_use", "edge_length2", "half_edge_edge", "counts"), edges))
    names = ("new_vertices", "new_attributes", "new_attr_valid", "new_vertex_edge", "out_faces", "out_face_parent", "totals")
    for mode, what in ((0, "all"), (1, "longer"), (2, "limit")):  # TSD_MARK_ALL, TSD_MARK_LONGER (edges above 5), TSD_MARK_VERTEX_LIMIT
        split = mesh_subdivide._split_arrays(v, f, keep, mode, 5.0, inputs["limit"], inputs["attributes"], inputs["attr_valid"], DEV)
        out.update({f"{n}_{what}": t for n, t in zip(names, split)})
    return out


def _limit(case, seed):
    case["limit"] = _dev(np.random.default_rng(seed).uniform(2.0, 9.0, case["v"].shape[0]).astype(np.float32))
    return _attributes(case, seed)


def test_ts_subdivide_h():
    v, f = ref_mesh_subdivide.cube_grid(8, 4)  # F = 768, 3 F = 2304: cell edges of 4, diagonals of 5.66
    assert len(f) == 768
    b = _mesh(v * np.float32(0.75), f[::-1].copy(), _punched(9, 768, 1))  # edges of 3, diagonals of 4.24: nothing is longer than 5
    differ = ("counts", "totals_all", "totals_longer", "totals_limit")
    base_a, base_b = _check(subdivide_call, _limit(_mesh(v, f), 8), _limit(b, 9), differ=differ)
    assert _i64(base_a, "counts") == [1152, 0, 1152, 0] and _i64(base_b, "counts")[1] > 0
    assert _i64(base_a, "totals_all")[1:3] == [1152, 4 * 768] and _i64(base_a, "totals_longer")[1] == 384 and _i64(base_b, "totals_longer")[1] == 0
    a, b = one_face_pair()
    base_a, base_b = _check(subdivide_call, _limit(a, 8), _limit(b, 8), differ=("counts", "totals_all"))
    assert _i64(base_a, "counts") == [3, 3, 0, 0] and _i64(base_a, "totals_all") == [3, 3, 4, 1] and _i64(base_b, "counts") == [0, 0, 0, 0]


# ---- ts_orient.h: tsw_orient in its three modes ----------------------------------------------------------------------------------------------------
def orient_call(inputs):
    from diff_recon_hip import mesh_orient
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    out = {}
    for name, mode in mesh_orient.OUTWARD.items():
        got = mesh_orient._orient_arrays(v, v.shape[0], f, keep, mode, DEV)
        out.update({f"{n}_{name}": t for n, t in zip(("face_piece", "face_flip", "out_faces", "counts"), got)})
    return out


def _scrambled(f, seed, share):
    f = np.array(f, np.int32)
    turn = np.random.default_rng(seed).random(len(f)) < share
    f[turn] = f[turn][:, ::-1]
    return f


def test_ts_orient_h():
    v, f = _latlong_sphere(rings=20, segments=24)
    a = _mesh(v, _scrambled(f, 1, 0.3))
    keep = _punched(9, len(f), 4)
    keep[24 + 48 * 8:24 + 48 * 9] = 0  # one whole band between two rings: two pieces
    b = _mesh(v * np.float32(-1.0), _scrambled(f, 2, 0.6), keep)  # mirrored: the volume rule turns the other way
    differ = tuple(f"counts_{name}" for name in ("anchor", "majority", "volume"))
    base_a, base_b = _check(orient_call, a, b, differ=differ)
    assert _i64(base_a, "counts_majority")[:2] == [len(f), 1] and _i64(base_b, "counts_majority")[1] == 2
    a, b = one_face_pair()
    base_a, base_b = _check(orient_call, a, b, differ=("counts_majority",))
    assert _i64(base_a, "counts_majority")[:2] == [1, 1] and _i64(base_b, "counts_majority")[:2] == [0, 0]


# ---- ts_flip.h: tse_flip, a round and the classification alone ---------------------------------------------------------------------------------------
def flip_call(inputs):
    from diff_recon_hip import mesh_flip
    v, f, keep = inputs["v"], inputs["f"], inputs["keep"]
    names = ("out_faces", "face_flipped", "edge_vertices", "edge_state", "edge_opposite", "totals")
    out = dict(zip(names, mesh_flip._flip_arrays(v, f, keep, mesh_flip.min_cos_of(30.0), 7, False, DEV)))
    again = mesh_flip._flip_arrays(v, out["out_faces"], keep, mesh_flip.min_cos_of(30.0), 8, False, DEV)  # a second round on the first one's faces
    out.update({f"{n}_2": t for n, t in zip(names, again)})
    only = mesh_flip._flip_arrays(v, f, keep, mesh_flip.min_cos_of(30.0), 7, True, DEV)
    out.update({f"{n}_classified": t for n, t in zip(names[2:], only[2:])})
    return out


def test_ts_flip_h():
    a, b = grid_pair()  # every cell of A is cut by its long diagonal; B loses candidates with its faces
    vs, fs = ref_mesh_flip.stretched_grid(20, 20)  # ... and takes the stretched grid's competing candidates instead
    b["v"], b["f"] = _dev(vs), _dev(fs.astype(np.int32))
    assert b["f"].shape == a["f"].shape
    base_a, base_b = _check(flip_call, a, b, differ=("totals", "totals_2", "totals_classified", "edge_state"))
    assert _i64(base_a, "totals")[3] > 100 and _i64(base_b, "totals")[3] > 0  # flips in both, and not the same number (differ)
    q = ref_mesh_flip.QUAD
    a, b = _mesh(q, ref_mesh_flip.LONG), _mesh(q, ref_mesh_flip.LONG, [1, 0])  # the smallest table with an interior edge: it flips in A
    base_a, base_b = _check(flip_call, a, b, differ=("totals", "face_flipped"))
    assert _i64(base_a, "totals")[3] == 1 and _i64(base_b, "totals")[3] == 0
    a, b = one_face_pair()
    _check(flip_call, a, b, differ=("totals", "edge_state"))


# ---- ts_weld.h: the large size is tests/test_mesh_weld_gpu.py::test_the_calls_can_be_captured_in_a_graph; here the smallest table -----------------
def test_ts_weld_h():
    from test_mesh_weld_gpu import weld_call
    q = ref_mesh_flip.QUAD[:3]
    a, b = {"v": _dev(q), "f": _dev(np.array([[0, 1, 2]], np.int32))}, {"v": _dev(np.zeros((3, 3), np.float32)), "f": _dev(np.array([[2, 0, 1]], np.int32))}
    base_a, base_b = _check(weld_call, a, b, differ=("count", "counts", "keep"))  # B: all coincident, one cluster, the face collapses
    assert base_a["count"].view(torch.int32).tolist() == [3] and _i64(base_a, "counts") == [3, 3, 0, 0]
    assert base_b["count"].view(torch.int32).tolist() == [1] and _i64(base_b, "counts") == [0, 0, 0, 0]


# ---- ts_simplify.h: tsq_cluster_labels -> ts2d_weld_compact -> tsq_place -> ts2d_weld_remap_faces -> tsq_unique_faces ------------------------------
SIMPLIFY_ORIGIN, SIMPLIFY_CELL = (-1.0, -1.0, -1.0), 0.25


def simplify_call(inputs):
    from diff_recon_hip import mesh_simplify, mesh_weld
    from diff_triangle_rasterization_2D import _C as native
    lib, weld = mesh_simplify._lib, mesh_weld._lib
    v, f, attributes, attr_valid = inputs["v"], inputs["f"], inputs["attributes"], inputs["attr_valid"]
    V, F, C = v.shape[0], f.shape[0], attributes.shape[1]
    s = native.stream()
    i32 = lambda *shape: torch.empty(shape, device=DEV, dtype=torch.int32)
    u8 = lambda *shape: torch.empty(shape, device=DEV, dtype=torch.uint8)
    label, remap, first_vertices, count = i32(V), i32(V), torch.empty((V, 3), device=DEV), i32(1)
    ws = mesh_simplify._workspace(V, F, DEV)
    mesh_simplify._check(lib.tsq_cluster_labels(V, v.data_ptr(), *SIMPLIFY_ORIGIN, SIMPLIFY_CELL, label.data_ptr(), ws.data_ptr(), ws.numel(), s),
                         "tsq_cluster_labels")
    weld_ws = mesh_weld._workspace(V, 0, DEV)
    native._check(weld.ts2d_weld_compact(V, label.data_ptr(), v.data_ptr(), 0, remap.data_ptr(), first_vertices.data_ptr(), count.data_ptr(),
                                         weld_ws.data_ptr(), weld_ws.numel(), s), "ts2d_weld_compact")
    out = {"label": label, "remap": remap, "count": count}
    for name, mode in mesh_simplify.PLACEMENT_MODES.items():
        placed, out_attributes, out_valid, members = torch.empty((V, 3), device=DEV), torch.empty((V, C), device=DEV), u8(V), i32(V)
        mesh_simplify._check(lib.tsq_place(V, F, v.data_ptr(), f.data_ptr(), remap.data_ptr(), *SIMPLIFY_ORIGIN, SIMPLIFY_CELL, 1e-3, mode,
                                           attributes.data_ptr(), attr_valid.data_ptr(), C, placed.data_ptr(), out_attributes.data_ptr(),
                                           out_valid.data_ptr(), members.data_ptr(), ws.data_ptr(), ws.numel(), s), "tsq_place")
        out.update({f"vertices_{name}": placed, f"attributes_{name}": out_attributes, f"valid_{name}": out_valid, f"members_{name}": members})
    new_faces, keep_remap, keep, counts = i32(F, 3), u8(F), u8(F), torch.empty((2,), device=DEV, dtype=torch.int64)
    native._check(weld.ts2d_weld_remap_faces(V, F, f.data_ptr(), remap.data_ptr(), new_faces.data_ptr(), keep_remap.data_ptr(), s), "remap_faces")
    # V, the bound on the number of clusters that the host knows without reading `count`
    mesh_simplify._check(lib.tsq_unique_faces(V, F, new_faces.data_ptr(), keep_remap.data_ptr(), keep.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                              ws.numel(), s), "tsq_unique_faces")
    out.update(faces=new_faces, keep_remap=keep_remap, keep=keep, counts=counts)
    return out


def test_ts_simplify_h():
    a, b = sphere_pair()
    b["f"] = torch.cat([b["f"][:900], b["f"][100:112].flip(1)])  # twelve faces once more, turned over: flaps
    base_a, base_b = _check(simplify_call, _attributes(a, 12), _attributes(b, 13), differ=("count", "counts", "keep"))
    assert _i64(base_a, "counts")[1] == 0 and _i64(base_b, "counts")[1] > 0
    a, b = one_face_pair()
    b["v"] = b["v"] * 0.01 + 0.1  # B: the three vertices in one cell, the face collapses
    base_a, base_b = _check(simplify_call, _attributes(a, 12), _attributes(b, 12), differ=("count", "keep"))
    assert base_a["count"].view(torch.int32).tolist() == [3] and base_b["count"].view(torch.int32).tolist() == [1]


# ---- ts_geom.h: tsg_face_areas -> tsg_sample_surface -> tsg_nearest_cross -------------------------------------------------------------------------
def geom_call(inputs, N=1000):
    import importlib
    from diff_triangle_rasterization_2D import _C as native
    G = importlib.import_module("diff_recon_hip.mesh_distance")._lib  # (the package also exports a FUNCTION of that name)

    def ok(rc, what):
        assert rc == 0, f"{what}: error {rc}: {G.tsg_last_error().decode()}"
    v, f, keep, refs = inputs["v"], inputs["f"], inputs["keep"], inputs["refs"]
    V, F, R, s = v.shape[0], f.shape[0], refs.shape[0], native.stream()
    area = torch.empty((F,), device=DEV, dtype=torch.float64)
    points, face = torch.empty((N, 3), device=DEV), torch.empty((N,), device=DEV, dtype=torch.int32)
    ok(G.tsg_face_areas(V, F, v.data_ptr(), f.data_ptr(), keep.data_ptr(), area.data_ptr(), s), "tsg_face_areas")
    nbytes = G.tsg_sample_workspace_bytes(F)
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    ok(G.tsg_sample_surface(V, F, v.data_ptr(), f.data_ptr(), area.data_ptr(), N, 1234, points.data_ptr(), face.data_ptr(), ws.data_ptr(), nbytes, s),
       "tsg_sample_surface")
    nearest, dist2 = torch.empty((N,), device=DEV, dtype=torch.int32), torch.empty((N,), device=DEV)
    visits = torch.zeros((1,), device=DEV, dtype=torch.int64)  # the caller clears it
    nbytes = G.tsg_cross_workspace_bytes(N, R)
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    ok(G.tsg_nearest_cross(N, points.data_ptr(), R, refs.data_ptr(), nearest.data_ptr(), dist2.data_ptr(), visits.data_ptr(), ws.data_ptr(), nbytes, s),
       "tsg_nearest_cross")
    return {"area": area, "points": points, "face": face, "nearest": nearest, "dist2": dist2, "box_visits": visits}


def _refs(case, R, seed, scale=1.0, shift=0.0, far_from=None):
    refs = np.random.default_rng(seed).uniform(-1, 1, (R, 3)) * scale + shift
    if far_from is not None:
        refs[far_from:] += 50.0  # boxes of their own, which a query near the first ones never visits
    case["refs"] = _dev(refs.astype(np.float32))
    return case


def test_ts_geom_h():
    a, b = sphere_pair()  # 1000 samples of F = 912 faces against 2500 refs: three boxes of 1024 refs, one box of queries
    base_a, base_b = _check(geom_call, _refs(a, 2500, 1, far_from=1024), _refs(b, 2500, 2, 0.25, 3.0), differ=("box_visits", "face", "nearest"))
    assert _i64(base_a, "box_visits")[0] > 0 and (base_a["face"].view(torch.int32) >= 0).all()
    a, b = one_face_pair()  # B: the one face is dropped, so the largest area is 0: every face is -1 and every point 0
    base_a, base_b = _check(geom_call, _refs(a, 1, 1), _refs(b, 1, 2), differ=("area", "face"))
    assert not base_a["face"].any() and (base_b["face"].view(torch.int32) == -1).all() and not base_b["points"].any()


# ---- the queries on the triangle index: tsb_build first in every graph, the query reading the index it wrote ------------------------------------------
Q = 1000


def _queries(case, seed, spread):
    """Q points around the mesh and Q ray directions; A and B differ in how far the points lie from it, and so in every hit count."""
    rng = np.random.default_rng(seed)
    case["points"] = _dev((rng.uniform(-1, 1, (Q, 3)) * spread).astype(np.float32))
    case["directions"] = _dev(rng.normal(size=(Q, 3)).astype(np.float32))
    case["t_limit"] = _dev(rng.uniform(0.2, 3.0, Q).astype(np.float32))
    return case


def _index(inputs):
    """tsb_build, the index and its workspace from torch.empty.  The bytes of the index are no documented output (include/ts_bvh.h documents
    what the queries return on it), so no call below returns them: the index is compared through every query that reads it.  The small
    case B drops its one face: an index without an eligible face, on which every query must say "no face", is part of what is replayed."""
    from diff_recon_hip.mesh_surface import MeshBVH
    return MeshBVH(inputs["v"], inputs["f"], inputs["keep"])


def _visits():
    return torch.zeros((1,), device=DEV, dtype=torch.int64)  # the caller clears it


def bvh_call(inputs):
    bvh, visits = _index(inputs), _visits()
    face, dist2, point = bvh.closest(inputs["points"], leaf_visits=visits)
    return {"face": face, "dist2": dist2, "point": point, "leaf_visits": visits}


def ray_call(inputs):
    from diff_recon_hip import mesh_ray
    bvh, visits = _index(inputs), _visits()
    first = mesh_ray.ray_cast(bvh, inputs["points"], inputs["directions"], leaf_visits=visits)
    culled = mesh_ray.ray_cast(bvh, inputs["points"], inputs["directions"], tmin=0.05, tmax=2.5, t_limit=inputs["t_limit"], cull_back=True)
    out = {"leaf_visits": visits}
    for name, hits in (("first", first), ("culled", culled)):
        out.update({f"{k}_{name}": t for k, t in zip(("face", "t", "bary", "side"), hits)})
    return out


def inside_call(inputs):
    from diff_recon_hip import mesh_inside
    lib = mesh_inside._lib
    from diff_triangle_rasterization_2D import _C as native
    bvh, visits = _index(inputs), _visits()
    _, dist2, _ = bvh.closest(inputs["points"])
    per_ray = mesh_inside.ray_crossings(bvh, inputs["points"], inputs["directions"], t_limit=inputs["t_limit"], leaf_visits=visits)
    shared = mesh_inside.ray_crossings(bvh, inputs["points"], inputs["directions"][0].contiguous())
    out = {"leaf_visits": visits, "hits_limited": per_ray.hits, "winding2_limited": per_ray.winding2, "touches_limited": per_ray.touches,
           "hits": shared.hits, "winding2": shared.winding2, "touches": shared.touches}
    for rule in (0, 1, 2):
        signed, decided = torch.empty((Q,), device=DEV), torch.empty((Q,), device=DEV, dtype=torch.uint8)
        mesh_inside._check(lib.tsi_signed_distance(Q, dist2.data_ptr(), shared.winding2.data_ptr(), shared.touches.data_ptr(), shared.hits.data_ptr(),
                                                   rule, 0, signed.data_ptr(), decided.data_ptr(), native.stream()), "tsi_signed_distance")
        out.update({f"signed_{rule}": signed, f"decided_{rule}": decided})
    return out


def winding_call(inputs):
    from diff_recon_hip import mesh_winding
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_winding._lib
    bvh = _index(inputs)
    _, dist2, _ = bvh.closest(inputs["points"])
    moments, leaf_faces = mesh_winding._build(bvh)  # tsn_moments
    out = {"moments": moments, "leaf_faces": leaf_faces}
    for name, beta in (("beta2", 2.0), ("exact", float("inf"))):
        wq, terms = mesh_winding._winding(bvh, inputs["points"], beta, True)  # tsn_winding
        signed, decided = torch.empty((Q,), device=DEV), torch.empty((Q,), device=DEV, dtype=torch.uint8)
        mesh_winding._check(lib.tsn_sign_distance(Q, dist2.data_ptr(), wq.data_ptr(), mesh_winding.threshold_units(0.5), signed.data_ptr(),
                                                  decided.data_ptr(), native.stream()), "tsn_sign_distance")
        out.update({f"wq_{name}": wq, f"terms_{name}": terms, f"signed_{name}": signed, f"decided_{name}": decided})
    return out


OVERLAP_CAPACITY = 8192  # above the total of every case below (asserted there): a list that overflows holds an unspecified choice of pairs


def _sorted_list(pairs, kind, stats):
    """The first stats[6] rows of (pairs, kind) ascending by (first, second, kind), the rows behind them -1 / 0xFF: every byte a function of
    the SET of rows the call wrote.  One 64-bit key per row, first * 2^39 + second * 2^8 + kind (face indices below 2^24 here), the rows
    that were not written under a sentinel that sorts last; sorted on the device and taken apart again."""
    stored = stats[6]
    written = torch.arange(pairs.shape[0], device=DEV) < stored
    key = (pairs[:, 0].to(torch.int64) << 39) | (pairs[:, 1].to(torch.int64) << 8) | kind.to(torch.int64)
    key = torch.sort(torch.where(written, key, torch.full_like(key, torch.iinfo(torch.int64).max))).values
    written = torch.arange(pairs.shape[0], device=DEV) < stored  # after the sort the written rows come first again
    first, second, k = (key >> 39).to(torch.int32), ((key >> 8) & 0x7FFFFFFF).to(torch.int32), (key & 0xFF).to(torch.uint8)
    minus = torch.full_like(first, -1)
    return (torch.stack([torch.where(written, first, minus), torch.where(written, second, minus)], dim=1),
            torch.where(written, k, torch.full_like(k, 0xFF)))


def overlap_call(inputs):
    """tsx_overlap in both modes.  The ORDER of its list is unspecified, the rows from stats[6] on are not written, and tsx_sort_pairs takes
    the number of pairs, which the host knows only from stats.  So the graph itself puts the list into an order (_sorted_list: torch
    operators on the device, no host step), and the sort call is captured separately (sort_pairs_call)."""
    from diff_recon_hip import mesh_overlap
    from diff_recon_hip.mesh_surface import MeshBVH
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_overlap._lib
    a, visits = _index(inputs), _visits()
    b = MeshBVH(inputs["v2"], inputs["f"], None)
    F, capacity = a.num_faces, OVERLAP_CAPACITY
    out = {"leaf_visits": visits}
    for name, other in (("self", None), ("cross", b)):
        count_a, stats = torch.empty((F,), device=DEV, dtype=torch.int32), torch.empty((8,), device=DEV, dtype=torch.int64)
        count_b = torch.empty((F,), device=DEV, dtype=torch.int32) if other is not None else None
        pairs, kind = torch.empty((capacity, 2), device=DEV, dtype=torch.int32), torch.empty((capacity,), device=DEV, dtype=torch.uint8)
        mesh_overlap._check(lib.tsx_overlap(F, a.bvh.data_ptr(), a.bvh.numel(), a.faces.data_ptr() if other is None else None,
                                            F if other is not None else 0, other.bvh.data_ptr() if other is not None else None,
                                            other.bvh.numel() if other is not None else 0, count_a.data_ptr(), native._ptr(count_b), stats.data_ptr(),
                                            capacity, pairs.data_ptr(), kind.data_ptr(), visits.data_ptr(), native.stream()), "tsx_overlap")
        out.update({f"count_a_{name}": count_a, f"stats_{name}": stats})
        out[f"pairs_{name}"], out[f"kind_{name}"] = _sorted_list(pairs, kind, stats)
        if count_b is not None:
            out["count_b_cross"] = count_b
    return out


def sort_pairs_call(inputs):
    from diff_recon_hip import mesh_overlap
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_overlap._lib
    P = inputs["pairs"].shape[0]
    pairs, kind = torch.empty((P, 2), device=DEV, dtype=torch.int32), torch.empty((P,), device=DEV, dtype=torch.uint8)
    pairs.copy_(inputs["pairs"])  # the call reorders in place
    kind.copy_(inputs["kind"])
    nbytes = lib.tsx_sort_workspace_bytes(P)
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    mesh_overlap._check(lib.tsx_sort_pairs(P, 12, 12, pairs.data_ptr(), kind.data_ptr(), ws.data_ptr(), nbytes, native.stream()), "tsx_sort_pairs")
    return {"pairs": pairs, "kind": kind}


def _index_pairs():
    a, b = sphere_pair()
    return _queries(a, 21, 0.3), _queries(b, 22, 1.5), _queries(one_face_pair()[0], 23, 4.0), _queries(one_face_pair()[1], 24, 9.0)


def _above(case):
    """Every ray from one point above the one face, straight down through it."""
    case["points"][:, :] = torch.tensor([0.0, 0.5, 1.0], device=DEV)
    case["directions"][:, :] = torch.tensor([0.0, 0.0, -1.0], device=DEV)


def test_ts_bvh_h():
    a, b, small_a, small_b = _index_pairs()
    base_a, base_b = _check(bvh_call, a, b, differ=("leaf_visits", "face", "dist2"))
    assert (base_a["face"].view(torch.int32) >= 0).all() and _i64(base_a, "leaf_visits")[0] > 0
    base_a, base_b = _check(bvh_call, small_a, small_b, differ=("face",))  # the one face, and no face at all
    assert not base_a["face"].any() and (base_b["face"].view(torch.int32) == -1).all()


def test_ts_ray_h():
    a, b, small_a, small_b = _index_pairs()
    base_a, base_b = _check(ray_call, a, b, differ=("leaf_visits", "face_first", "face_culled"))
    hit_a, hit_b = (int((s["face_first"].view(torch.int32) >= 0).sum()) for s in (base_a, base_b))
    assert hit_a == Q and 0 < hit_b < Q  # A's origins lie inside the closed sphere; B's in and around a punched one
    _above(small_a)
    _check(ray_call, small_a, small_b, differ=("face_first",))


def test_ts_inside_h():
    a, b, small_a, small_b = _index_pairs()
    base_a, base_b = _check(inside_call, a, b, differ=("leaf_visits", "hits", "hits_limited", "signed_0"))
    assert int(base_a["hits"].view(torch.int32).min()) >= 1  # from inside a closed sphere every ray leaves
    _above(small_a)
    _check(inside_call, small_a, small_b, differ=("hits",))


def test_ts_winding_h():
    a, b, small_a, small_b = _index_pairs()
    _check(winding_call, a, b, differ=("moments", "leaf_faces", "wq_beta2", "wq_exact"))
    _check(winding_call, small_a, small_b, differ=("leaf_faces", "wq_exact"))


def test_ts_overlap_h():
    a, b = sphere_pair()
    rng = np.random.default_rng(31)
    for case, shift in ((a, 0.3), (b, 0.05)):  # the same sphere again, pushed aside: the two cross along a circle
        case["v2"] = (case["v"] + torch.tensor([shift, 0.0, 0.02], device=DEV)).contiguous()
    a["v"][torch.from_numpy(rng.choice(458, 5, replace=False)).to(DEV)] *= -0.9  # five vertices of A pushed through to the far side: their faces cross others
    differ = ("leaf_visits", "stats_self", "stats_cross", "count_a_cross", "pairs_self", "pairs_cross", "kind_cross")
    base_a, base_b = _check(overlap_call, a, b, differ=differ)
    for base in (base_a, base_b):
        for mode in ("self", "cross"):  # the whole list fits, and the graph's own ordering kept exactly the rows that were stored
            st = _i64(base, f"stats_{mode}")
            listed = base[f"pairs_{mode}"].view(torch.int32).reshape(-1, 2)
            assert st[6] == sum(st[2:5]) <= OVERLAP_CAPACITY and int((listed[:, 0] >= 0).sum()) == st[6]
            assert (listed[:st[6], 1] >= 0).all() and (base[f"kind_{mode}"][:st[6]] != 0xFF).all() and (base[f"kind_{mode}"][:st[6]] != 0).all()
    listed = base_a["pairs_self"].view(torch.int32).reshape(-1, 2)[:_i64(base_a, "stats_self")[6]].to(torch.int64)
    assert (listed[:, 0] < listed[:, 1]).all() and ((listed[1:, 0] << 32 | listed[1:, 1]) > (listed[:-1, 0] << 32 | listed[:-1, 1])).all()  # lo < hi, no pair twice
    assert _i64(base_a, "stats_self")[2] > 0 and _i64(base_b, "stats_self")[2] == 0  # [2]: crossing pairs
    assert sum(_i64(base_a, "stats_cross")[2:5]) > 0 and sum(_i64(base_b, "stats_cross")[2:5]) > 0
    small_a, small_b = one_face_pair()
    small_a["v2"], small_b["v2"] = small_a["v"].flip(1).contiguous(), small_b["v"].flip(1).contiguous()  # the one face against its mirror image
    base_a, base_b = _check(overlap_call, small_a, small_b, differ=("stats_cross", "pairs_cross", "kind_cross"))
    assert base_a["pairs_cross"].view(torch.int32)[:2].tolist() == [0, 0] and _i64(base_a, "stats_cross")[6] == 1 and _i64(base_b, "stats_cross")[6] == 0
    # tsx_sort_pairs on its own: P is a host value
    for P in (2500, 1):
        lists = []
        for seed in (41, 42):
            r = np.random.default_rng(seed + P)
            lists.append({"pairs": _dev(r.integers(0, 4096, (P, 2)).astype(np.int32)), "kind": _dev(r.integers(1, 4, P).astype(np.uint8))})
        _check(sort_pairs_call, lists[0], lists[1], differ=("pairs",))


# ---- ts_volume.h: tsv_integrate (two views) -> tsv_field -> tsv_extract; ts_color.h: tsc_integrate -> tsc_color_field -> tsc_sample / tsc_interpolate --
GRID, VOXEL, GRID_ORIGIN, IMG, TAN = 24, 0.08, (-0.95, -0.95, -0.95), 32, 0.45
TRIANGLE_CAPACITY = 40000
SMALL_EYES = ((-3, 0, 0), (0, -3, 0))  # both see the corner at GRID_ORIGIN from its own side


class _Cam:
    def __init__(self, view):
        self.world_view_transform, self.tan_fovx, self.tan_fovy, self.image_width, self.image_height, self.device = view, TAN, TAN, IMG, IMG, DEV


def _fusion_case(radius, eyes, seed, dims=(GRID, GRID, GRID)):
    """Two 32 x 32 views of a sphere of `radius` from `eyes`, with their depth, a colour image each, and sample points in the grid."""
    import ref_volume
    rng = np.random.default_rng(seed)
    views = np.stack([np.asarray(ref_volume.look_at_view(eye), np.float32) for eye in eyes])
    depth = np.stack([ref_volume.sphere_depth(view, TAN, IMG, IMG, radius) for view in views])
    extent = VOXEL * (np.array(dims) - 1)
    return {"views": _dev(views), "depth": _dev(depth), "image": _dev(rng.uniform(0, 1, (2, 3, IMG, IMG)).astype(np.float32)),
            "points": _dev((np.array(GRID_ORIGIN) + rng.uniform(-0.05, 1.05, (Q, 3)) * extent).astype(np.float32))}


def _dims(inputs):
    return tuple(int(n) for n in inputs["dims"].shape)  # carried by a shape: a host value that both cases share


def volume_call(inputs):
    from diff_recon_hip import volume
    from diff_triangle_rasterization_2D import _C as native
    lib = volume._lib
    nx, ny, nz = dims = _dims(inputs)
    vol = volume.TSDFVolume(GRID_ORIGIN, VOXEL, dims, 4 * VOXEL, DEV)  # sum and weight cleared by torch.zeros: fill nodes of the graph
    updated = torch.zeros((1,), device=DEV, dtype=torch.int64)
    for i in range(2):
        vol.integrate(_Cam(inputs["views"][i]), inputs["depth"][i], carve_uncovered=bool(i), updated=updated)
    field = vol.field()
    nbytes = lib.tsv_extract_workspace_bytes(nx, ny, nz)
    out = {"sum": vol.sum, "weight": vol.weight, "updated": updated, "field": field}
    for name, capacity in (("count", 0), ("list", TRIANGLE_CAPACITY)):  # the counting call, then the bound as the capacity
        ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
        total = torch.empty((1,), device=DEV, dtype=torch.int64)
        triangles = torch.empty((capacity, 9), device=DEV) if capacity else None
        cell = torch.empty((capacity,), device=DEV, dtype=torch.int32) if capacity else None
        volume._check(lib.tsv_extract(nx, ny, nz, *GRID_ORIGIN, VOXEL, field.data_ptr(), 0.0, capacity, native._ptr(triangles), native._ptr(cell),
                                      total.data_ptr(), ws.data_ptr(), nbytes, native.stream()), "tsv_extract")
        out[f"total_{name}"] = total
    # the call writes the first `total` rows and leaves the rest alone (include/ts_volume.h): what lies behind them is no output
    written = torch.arange(TRIANGLE_CAPACITY, device=DEV) < total
    out["triangles"] = torch.where(written[:, None], triangles, torch.zeros((), device=DEV))
    out["cell"] = torch.where(written, cell, torch.zeros((), device=DEV, dtype=torch.int32))
    return out


def _with_dims(case, dims):
    case["dims"] = torch.zeros(dims, device=DEV, dtype=torch.uint8)
    return case


def test_ts_volume_h():
    import ref_volume
    a = _with_dims(_fusion_case(0.6, ref_volume.AXIS_EYES[0:2], 51), (GRID,) * 3)
    b = _with_dims(_fusion_case(0.4, ref_volume.AXIS_EYES[2:4], 52), (GRID,) * 3)
    base_a, base_b = _check(volume_call, a, b, differ=("updated", "total_count", "total_list", "weight", "triangles"))
    assert _i64(base_a, "total_count") == _i64(base_a, "total_list") and 0 < _i64(base_a, "total_list")[0] < TRIANGLE_CAPACITY
    assert 0 < _i64(base_b, "total_list")[0] < _i64(base_a, "total_list")[0]
    # the smallest grid with a cell, at the corner of the large one (1.5 to 1.65 from the centre): a sphere of 1.57 passes through it in A
    a = _with_dims(_fusion_case(1.57, SMALL_EYES, 53), (2, 2, 2))
    b = _with_dims(_fusion_case(1.57, SMALL_EYES, 54), (2, 2, 2))
    b["depth"].zero_()  # B: nothing covered, nothing integrated by the first view, free space by the second
    _check(volume_call, a, b, differ=("updated", "sum"))


def color_call(inputs):
    from diff_recon_hip import color_volume
    dims = _dims(inputs)
    vol = color_volume.ColorTSDFVolume(GRID_ORIGIN, VOXEL, dims, 4 * VOXEL, DEV)
    updated, colored = torch.zeros((1,), device=DEV, dtype=torch.int64), torch.zeros((1,), device=DEV, dtype=torch.int64)
    for i in range(2):
        vol.integrate(_Cam(inputs["views"][i]), inputs["depth"][i], image=inputs["image"][i], updated=updated, colored=colored)
    field = vol.color_field()
    values, valid = color_volume.sample_grid(field, GRID_ORIGIN, VOXEL, inputs["points"])
    image, bary = color_volume.interpolate_vertex_attributes(_Cam(inputs["views"][0]), inputs["v"], inputs["f"], inputs["face_idx"], inputs["attributes"],
                                                             inputs["background"], return_bary=True)
    return {"csum": vol.csum, "cweight": vol.cweight, "updated": updated, "colored": colored, "color_field": field, "values": values,
            "valid": valid, "image": image, "bary": bary}


def _color_case(case, mesh, seed):
    rng = np.random.default_rng(seed)
    F, V = mesh["f"].shape[0], mesh["v"].shape[0]
    case.update(v=mesh["v"], f=mesh["f"], face_idx=_dev(rng.integers(-1, F, (IMG, IMG)).astype(np.int32)),
                attributes=_dev(rng.uniform(0, 1, (V, 3)).astype(np.float32)), background=_dev(rng.uniform(0, 1, 3).astype(np.float32)))
    return case


def test_ts_color_h():
    import ref_volume
    mesh_a, mesh_b = sphere_pair()
    a = _color_case(_with_dims(_fusion_case(0.6, ref_volume.AXIS_EYES[0:2], 61), (GRID,) * 3), mesh_a, 62)
    b = _color_case(_with_dims(_fusion_case(0.4, ref_volume.AXIS_EYES[2:4], 63), (GRID,) * 3), mesh_b, 64)
    base_a, base_b = _check(color_call, a, b, differ=("updated", "colored", "cweight", "valid", "image"))
    assert _i64(base_a, "colored")[0] > 2048 and _i64(base_b, "colored")[0] > 0
    small_a, small_b = one_face_pair()
    a = _color_case(_with_dims(_fusion_case(1.57, SMALL_EYES, 65), (2, 2, 2)), small_a, 66)
    b = _color_case(_with_dims(_fusion_case(1.57, SMALL_EYES, 67), (2, 2, 2)), small_b, 68)
    b["depth"].zero_()
    b["face_idx"].fill_(-1)  # B: no pixel covered, the background everywhere
    _check(color_call, a, b, differ=("colored", "image"))


# ---- ts_knn.h: tsk_mean_dist3, tsk_nearest_other -------------------------------------------------------------------------------------------------------
def knn_call(inputs):
    from diff_triangle_rasterization_2D import _C as native
    lib = native._lib
    points = inputs["points"]
    P = points.shape[0]
    nbytes = lib.tsk_workspace_bytes(P)
    mean, nearest = torch.empty((P,), device=DEV), torch.empty((P,), device=DEV, dtype=torch.int32)
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    native._check(lib.tsk_mean_dist3(P, points.data_ptr(), mean.data_ptr(), ws.data_ptr(), nbytes, native.stream()), "tsk_mean_dist3")
    ws = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
    native._check(lib.tsk_nearest_other(P, inputs["batch"].shape[0], points.data_ptr(), nearest.data_ptr(), ws.data_ptr(), nbytes, native.stream()),
                  "tsk_nearest_other")
    return {"mean_dist2": mean, "nearest": nearest}


def test_ts_knn_h():
    for P, batch in ((1025, 5), (4, 1)):  # two boxes of 1024 sorted points, the second with one point; the smallest set with three neighbours each
        cases = []
        for seed, scale in ((71, 1.0), (72, 30.0)):
            points = np.random.default_rng(seed + P).uniform(-1, 1, (P, 3)) * scale
            cases.append({"points": _dev(points.astype(np.float32)), "batch": torch.zeros(batch, device=DEV, dtype=torch.uint8)})
        _check(knn_call, cases[0], cases[1], differ=("mean_dist2", "nearest") if P > 4 else ("mean_dist2",))


# ---- ts_atlas.h: tsa_texel_index -> tsa_render; tsa_face_totals -> tsa_resolve -> tsa_render -------------------------------------------------------
ATLAS_RES = 3


def atlas_call(inputs):
    import ctypes
    from diff_recon_hip import mesh_texture
    from diff_triangle_rasterization_2D import _C as native
    lib = mesh_texture._lib
    v, f, texels = inputs["v"], inputs["f"], inputs["texels"]
    F = f.shape[0]
    lay = mesh_texture.atlas_layout(F, ATLAS_RES)
    texel_idx, atlas_idx, bary = mesh_texture.texel_index(_Cam(inputs["views"][0]), v, f, inputs["face_idx"], lay, return_atlas_idx=True, return_bary=True)
    totals = torch.empty((F, 4), device=DEV, dtype=torch.int64)
    mesh_texture._check(lib.tsa_face_totals(F, lay.res, texels.data_ptr(), totals.data_ptr(), native.stream()), "tsa_face_totals")
    image = torch.empty((3, lay.height, lay.width), device=DEV)
    state = torch.empty((lay.height, lay.width), device=DEV, dtype=torch.uint8)
    rgb8 = torch.empty((lay.height, lay.width, 3), device=DEV, dtype=torch.uint8)
    mesh_texture._check(lib.tsa_resolve(F, lay.res, lay.cells_per_row, lay.cells_per_col, texels.data_ptr(), totals.data_ptr(), 2,
                                        inputs["fallback"].data_ptr(), (ctypes.c_float * 3)(0.25, 0.5, 0.75), image.data_ptr(), state.data_ptr(),
                                        rgb8.data_ptr(), native.stream()), "tsa_resolve")
    render = torch.empty((3, IMG, IMG), device=DEV)
    mesh_texture._check(lib.tsa_render(IMG, IMG, lay.width, lay.height, atlas_idx.data_ptr(), image.data_ptr(), inputs["background"].data_ptr(),
                                       render.data_ptr(), native.stream()), "tsa_render")
    return {"texel_idx": texel_idx, "atlas_idx": atlas_idx, "bary": bary, "face_totals": totals, "image": image, "state": state, "rgb8": rgb8,
            "render": render}


def _atlas_case(mesh, eye, seed, seen):
    """The mesh from `eye`, a face_idx of random faces of it, and an accumulator in which about `seen` of the texels were seen 1 to 3 times."""
    import ref_volume
    rng = np.random.default_rng(seed)
    F = mesh["f"].shape[0]
    rows = F * ATLAS_RES * (ATLAS_RES + 1) // 2
    count = rng.integers(1, 4, rows) * (rng.random(rows) < seen)
    texels = np.concatenate([count[:, None], count[:, None] * rng.integers(0, 65537, (rows, 3))], axis=1).astype(np.int64)
    return {"v": mesh["v"], "f": mesh["f"], "views": _dev(np.asarray(ref_volume.look_at_view(eye), np.float32)[None]),
            "face_idx": _dev(rng.integers(-1, F, (IMG, IMG)).astype(np.int32)), "texels": _dev(texels),
            "fallback": _dev(rng.uniform(0, 1, (F, 3)).astype(np.float32)), "background": _dev(rng.uniform(0, 1, 3).astype(np.float32))}


def test_ts_atlas_h():
    mesh_a, mesh_b = sphere_pair()  # F T = 5472 texels
    base_a, base_b = _check(atlas_call, _atlas_case(mesh_a, (3, 0, 0), 81, 0.9), _atlas_case(mesh_b, (0, 3, 0), 82, 0.2),
                            differ=("texel_idx", "face_totals", "state", "render"))
    assert {int(s) for s in base_a["state"].unique()} >= {2, 3} and {int(s) for s in base_b["state"].unique()} >= {1, 2, 3}
    small_a, small_b = one_face_pair()
    a, b = _atlas_case(small_a, (0, 0, 3), 83, 1.0), _atlas_case(small_b, (0, 0, 3), 84, 0.0)  # B: no texel was seen, and no pixel drawn
    b["face_idx"].fill_(-1)
    base_a, base_b = _check(atlas_call, a, b, differ=("texel_idx", "face_totals", "state"))
    assert not base_b["face_totals"].any() and (base_b["texel_idx"].view(torch.int32) == -1).all()
