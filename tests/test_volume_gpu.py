"""GPU tests of the TSDF volume and the marching tetrahedra against tests/ref_volume.py: the integrated state, the field and the extracted
soup bit for bit and in order, the capacity contract, purity, the closed surface through weld_mesh / mesh_topology, fuse_mesh end to end on
MeshRenderer depth, and the example's report."""
import functools
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import poison
import ref_volume as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DIMS, ORIGIN, H, TRUNC = (20, 18, 16), (-1.0, -0.9, -0.8), 0.1, 0.35
W_IMG, H_IMG = 24, 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cam(view, tan_fovx, tan_fovy, W, H):
    return SimpleNamespace(world_view_transform=_dev(np.asarray(view, np.float32)), tan_fovx=tan_fovx, tan_fovy=tan_fovy, image_width=W,
                           image_height=H, device="cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _views():
    """Three views of 24 x 20 over the 20 x 18 x 16 grid: one that sees all of it, one whose narrow frustum misses part of it, one whose
    eye sits inside the grid (samples at z <= 0).  Depth: random about the distance to the grid's centre, with 0, negative, NaN and inf
    entries; a random mask."""
    rng = np.random.default_rng(11)
    out = []
    for eye, tan in (((0.3, -0.2, -3.0), (0.5, 0.45)), ((2.5, 1.0, 0.4), (0.12, 0.1)), ((0.35, 0.2, -0.45), (0.9, 0.8))):
        view = ref.look_at_view(eye)
        dist = float(np.linalg.norm(eye))
        depth = (dist + rng.uniform(-0.9, 0.9, (H_IMG, W_IMG))).astype(np.float32)
        special = rng.integers(0, 12, (H_IMG, W_IMG))
        for code, value in ((0, 0.0), (1, -0.5), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -0.0)):
            depth[special == code] = value
        mask = (rng.integers(0, 4, (H_IMG, W_IMG)) != 0).astype(np.uint8)
        out.append((view, tan, depth, mask))
    return out


def test_the_views_cover_the_cases_the_kernel_branches_on():
    (p0, p1, p2), _ = ref.sample_positions(DIMS, ORIGIN, H)
    seen = []
    for view, (tx, ty), depth, mask in _views():
        M = view.astype(np.float64)
        v = [((p0 * M[0, c] + p1 * M[1, c]) + p2 * M[2, c]) + M[3, c] for c in range(3)]
        z = v[2]
        with np.errstate(all="ignore"):
            col = np.floor((v[0] / (z * np.float32(tx)) + 1.0) * (0.5 * W_IMG))
            row = np.floor((v[1] / (z * np.float32(ty)) + 1.0) * (0.5 * H_IMG))
        outside = (z > 0) & ((col < 0) | (col >= W_IMG) | (row < 0) | (row >= H_IMG))
        seen.append(((z <= 0).sum(), outside.sum()))
        for value in (0.0, np.inf, -np.inf):
            assert (depth == value).any()
        assert np.isnan(depth).any() and (depth < 0).any() and (mask == 0).any() and (mask != 0).any()
    assert seen[0] == (0, 0) and seen[1][1] > 1000 and seen[2][0] > 100, seen


# ---- integrate and field ------------------------------------------------------------------------------------------------------------------------
def _integrate_gpu(order, use_mask, carve):
    from diff_recon_hip import TSDFVolume
    vol = TSDFVolume(ORIGIN, H, DIMS, TRUNC, DEV)
    updated = torch.zeros(1, device=DEV, dtype=torch.int64)
    counts = []
    for k in order:
        view, (tx, ty), depth, mask = _views()[k]
        vol.integrate(_cam(view, tx, ty, W_IMG, H_IMG), _dev(depth), mask=_dev(mask) if use_mask else None, carve_uncovered=carve, updated=updated)
        counts.append(int(updated.item()))
    return vol, counts


@functools.lru_cache(maxsize=None)
def _integrate_ref(order, use_mask, carve):
    n = DIMS[0] * DIMS[1] * DIMS[2]
    s, w, counts, total = np.zeros(n, np.int64), np.zeros(n, np.int32), [], 0
    for k in order:
        view, (tx, ty), depth, mask = _views()[k]
        total += ref.integrate(s, w, DIMS, ORIGIN, H, TRUNC, view, tx, ty, W_IMG, H_IMG, depth, mask if use_mask else None,
                               ref.CARVE_UNCOVERED if carve else 0)
        counts.append(total)
    return s, w, counts


@pytest.mark.parametrize("carve", [False, True])
@pytest.mark.parametrize("use_mask", [False, True])
def test_integrate_matches_the_reference_bit_for_bit(use_mask, carve):
    vol, counts = _integrate_gpu((0, 1, 2), use_mask, carve)
    s, w, want = _integrate_ref((0, 1, 2), use_mask, carve)
    assert vol.sum.shape == vol.weight.shape == DIMS[::-1] and vol.sum.dtype == torch.int64 and vol.weight.dtype == torch.int32
    got_s, got_w = vol.sum.cpu().numpy().reshape(-1), vol.weight.cpu().numpy().reshape(-1)
    print("updated per view", want, "weights", np.bincount(w))
    assert counts == want
    assert np.array_equal(got_w, w), np.nonzero(got_w != w)[0][:10]
    assert np.array_equal(got_s, s), np.nonzero(got_s != s)[0][:10]
    assert want[0] > 0 and want[1] > want[0] and want[2] > want[1] and (w == 0).any() and (w == 3).any()  # every view adds; not everything is seen


def test_a_saturated_weight_is_left_alone():
    from diff_recon_hip import TSDFVolume
    vol = TSDFVolume(ORIGIN, H, DIMS, TRUNC, DEV)
    vol.weight.view(-1)[::3] = ref.INT32_MAX
    vol.sum.view(-1)[::3] = -7
    view, (tx, ty), depth, _ = _views()[0]
    updated = torch.zeros(1, device=DEV, dtype=torch.int64)
    vol.integrate(_cam(view, tx, ty, W_IMG, H_IMG), _dev(depth), carve_uncovered=True, updated=updated)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    w[::3], s[::3] = ref.INT32_MAX, -7
    want = ref.integrate(s, w, DIMS, ORIGIN, H, TRUNC, view, tx, ty, W_IMG, H_IMG, depth, None, ref.CARVE_UNCOVERED)
    assert int(updated.item()) == want and np.array_equal(vol.weight.cpu().numpy().reshape(-1), w) and np.array_equal(vol.sum.cpu().numpy().reshape(-1), s)


def test_view_order_does_not_matter_and_the_field_is_bit_equal():
    a, _ = _integrate_gpu((0, 1, 2), True, True)
    b, _ = _integrate_gpu((2, 0, 1), True, True)
    assert torch.equal(a.sum, b.sum) and torch.equal(a.weight, b.weight)
    s, w, _ = _integrate_ref((0, 1, 2), True, True)
    for min_weight in (1, 2, 3):
        got = b.field(min_weight).cpu().numpy().reshape(-1)
        want = ref.field(s, w, min_weight)
        assert np.array_equal(_bits(got), _bits(want)), min_weight
        assert np.array_equal(np.isnan(got), w < min_weight) and np.isnan(got).any() and not np.isnan(got).all()
    half = _integrate_gpu((0,), True, True)[0]  # volumes add: the state tensors are plain attributes
    rest = _integrate_gpu((1, 2), True, True)[0]
    half.sum += rest.sum
    half.weight += rest.weight
    assert torch.equal(half.sum, a.sum) and torch.equal(half.weight, a.weight)


# ---- extract ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(kind):
    """(field, dims, origin, h, iso)"""
    if kind == "sphere":
        return ref.sphere_field((12, 12, 12), (5.3, 5.6, 5.45), 3.7), (12, 12, 12), (0.0, 0.0, 0.0), 1.0, 0.0
    if kind == "torus":
        return ref.torus_field((12, 12, 12), (5.3, 5.6, 5.45), 3.4, 1.3), (12, 12, 12), (0.0, 0.0, 0.0), 1.0, 0.0
    if kind == "random":  # every (tetrahedron, case) pair, NaN and inf samples, an origin and a spacing that are no powers of two
        rng = np.random.default_rng(5)
        f = rng.normal(0.05, 1.0, 9 * 8 * 7).astype(np.float32)
        f[rng.integers(0, f.size, 40)] = np.nan
        f[rng.integers(0, f.size, 8)] = np.inf
        f[rng.integers(0, f.size, 8)] = -np.inf
        return f, (9, 8, 7), (0.1, -0.7, 3.3), 0.3, 0.05
    if kind == "blocks":  # more than one workgroup of cells, more than one tile of samples: 40 x 20 x 3 = 2400 samples
        return ref.sphere_field((40, 20, 3), (19.4, 9.7, 1.2), 7.3), (40, 20, 3), (-2.0, 1.0, 0.5), 0.25, 0.0
    if kind == "outside":
        return np.full(5 * 4 * 3, 2.5, np.float32), (5, 4, 3), (0.0, 0.0, 0.0), 1.0, 0.0
    if kind == "inside":
        return np.full(5 * 4 * 3, -2.5, np.float32), (5, 4, 3), (0.0, 0.0, 0.0), 1.0, 0.0
    if kind == "flat":  # one layer of samples: no cell at all
        return np.linspace(-1, 1, 30).astype(np.float32), (6, 5, 1), (0.0, 0.0, 0.0), 1.0, 0.0
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _extract_ref(kind):
    f, dims, origin, h, iso = _field(kind)
    return ref.extract(f, dims, origin, h, iso)


def _extract_gpu(kind):
    from diff_recon_hip import volume
    f, dims, origin, h, iso = _field(kind)
    v, faces, cells = volume.extract_isosurface(_dev(f.reshape(dims[::-1])), origin, h, iso, with_cells=True)
    assert v.dtype == torch.float32 and faces.dtype == cells.dtype == torch.int32 and v.shape[0] == 3 * faces.shape[0] == 3 * cells.shape[0]
    assert torch.equal(faces.reshape(-1), torch.arange(v.shape[0], device=DEV, dtype=torch.int32))
    return v.cpu().numpy().reshape(-1, 3, 3), cells.cpu().numpy()


@pytest.mark.parametrize("kind", ["sphere", "torus", "random", "blocks", "outside", "inside", "flat"])
def test_extract_matches_the_reference_bit_for_bit_and_in_order(kind):
    want_tri, want_cell = _extract_ref(kind)
    tri, cell = _extract_gpu(kind)
    print(kind, "triangles", len(want_tri))
    assert len(tri) == len(want_tri)  # total
    assert np.array_equal(cell, want_cell)
    diff = (_bits(tri) != _bits(want_tri)).reshape(len(tri), 9).any(axis=1)
    assert not diff.any(), (np.nonzero(diff)[0][:10], tri[diff][:2], want_tri[diff][:2])
    assert (len(tri) == 0) == (kind in ("outside", "inside", "flat"))
    if kind == "sphere":
        assert len(tri) == 1548
    if kind == "torus":
        assert len(tri) == 1372


def test_the_random_field_meets_every_tetrahedron_case_pair():
    f, dims, _, _, iso = _field("random")
    nx, ny, nz = dims
    seen = set()
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corner = [f[((k + (c >> 2 & 1)) * ny + j + (c >> 1 & 1)) * nx + i + (c & 1)] for c in range(8)]
                if np.isfinite(corner).all():
                    seen |= {(t, sum(1 << m for m in range(4) if corner[tet[m]] < iso)) for t, tet in enumerate(ref.TETS)}
    assert seen == {(t, m) for t in range(6) for m in range(16)}
    assert not np.isfinite(f).all()


def test_capacity_below_the_total_writes_only_the_prefix():
    from diff_recon_hip import volume
    lib = volume._lib
    f, dims, origin, h, iso = _field("sphere")
    want_tri, want_cell = _extract_ref("sphere")
    total_want = len(want_tri)
    fld = _dev(f)
    need = lib.tsv_extract_workspace_bytes(*dims)
    for capacity in (0, 1, 700, total_want, total_want + 5):
        with poison.PoisonedEmpty("float1") as pe:
            ws = poison.filled(need, torch.uint8, device=DEV)
            tri = poison.filled((total_want + 5, 9), torch.float32, device=DEV)
            cell = poison.filled(total_want + 5, torch.int32, device=DEV)
            total = poison.filled(1, torch.int64, device=DEV)
            rc = lib.tsv_extract(*dims, *origin, h, fld.data_ptr(), iso, capacity, tri.data_ptr() if capacity else None, cell.data_ptr(), total.data_ptr(),
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.tsv_last_error()
            torch.cuda.synchronize()
            pe.check_guards()
            assert int(total.item()) == total_want  # always the full count
            n = min(capacity, total_want)
            got, got_cell = tri.cpu().numpy(), cell.cpu().numpy()
            assert np.array_equal(_bits(got[:n]), _bits(want_tri.reshape(-1, 9)[:n])) and np.array_equal(got_cell[:n], want_cell[:n])
            assert (_bits(got[n:]) == 0x3F800000).all() and (got_cell[n:].view(np.uint32) == 0x3F800000).all()  # untouched: still the poison


def test_sphere_extraction_welds_into_one_closed_surface():
    from diff_recon_hip import extract_isosurface, mesh_topology, weld_mesh
    f, dims, origin, h, iso = _field("sphere")
    v, faces = extract_isosurface(_dev(f.reshape(dims[::-1])), origin, h, iso)
    w = weld_mesh(v, faces, eps=0.0)
    topo = mesh_topology(w.stats["num_vertices"], w.faces)
    print(w.stats, topo)
    assert w.stats["num_vertices"] == 776 and w.stats["num_faces"] == 1548 and topo["edges"] == 2322
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["pieces"] == 1 and topo["euler"] == 2


def test_field_and_extract_are_pure_and_repeatable():
    from diff_recon_hip import volume
    vol, _ = _integrate_gpu((0, 1, 2), False, True)

    def call(pattern):  # the field, the workspace, the total, the triangles and the cells come from torch.empty: all poisoned
        fld = vol.field(1)
        v, _, cells = volume.extract_isosurface(fld, vol.origin, vol.voxel_size, 0.0, with_cells=True)
        v2, _, cells2 = volume.extract_isosurface(fld, vol.origin, vol.voxel_size, 0.0, with_cells=True)  # again: nothing left behind matters
        assert v.shape[0] > 300
        return {"field": fld, "vertices": v, "cells": cells, "vertices_again": v2, "cells_again": cells2}

    base = poison.assert_pure(call)
    assert torch.equal(base["vertices"], base["vertices_again"]) and torch.equal(base["cells"], base["cells_again"])
    s, w, _ = _integrate_ref((0, 1, 2), False, True)
    want_tri, _ = ref.extract(ref.field(s, w), DIMS, ORIGIN, H)
    assert np.array_equal(base["vertices"].numpy().view(np.uint32), _bits(want_tri).reshape(-1))


def test_integrate_is_pure_on_a_cleared_state():
    def call(pattern):
        vol, counts = _integrate_gpu((2, 1), True, False)
        return {"sum": vol.sum, "weight": vol.weight, "updated": torch.tensor(counts)}

    poison.assert_pure(call)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def _latlong_sphere(nlon=24, nlat=12, r=0.6):
    v = [(0.0, 0.0, r)]
    for a in range(1, nlat):
        for b in range(nlon):
            th, ph = math.pi * a / nlat, 2 * math.pi * b / nlon
            v.append((r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)))
    v.append((0.0, 0.0, -r))
    south = len(v) - 1
    ring = lambda a, b: 1 + (a - 1) * nlon + b % nlon
    f = []
    for b in range(nlon):
        f.append((0, ring(1, b), ring(1, b + 1)))
        for a in range(1, nlat - 1):
            f += [(ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)), (ring(a, b), ring(a + 1, b + 1), ring(a, b + 1))]
        f.append((south, ring(nlat - 1, b + 1), ring(nlat - 1, b)))
    return np.array(v, np.float32), np.array(f, np.int32)


def test_fuse_mesh_of_a_sphere_equals_the_numpy_pipeline_and_is_closed():
    from diff_recon_hip import MeshRenderer, fuse_mesh, mesh_surface_distance, mesh_topology
    v, f = _latlong_sphere()
    assert len(f) == 2 * 24 * 11
    cams = [_cam(ref.look_at_view(eye), 0.45, 0.45, 48, 48) for eye in ref.AXIS_EYES]
    vd, fd = _dev(v), _dev(f)
    fused, vol = fuse_mesh(cams, vd, fd, 20, return_volume=True)
    assert vol.dims == (20, 20, 20) and abs(vol.trunc - 4 * vol.voxel_size) < 1e-12 and abs(vol.voxel_size - 1.2 / 11) < 1e-6
    # the numpy pipeline on the same rendered depth images
    n = 20 ** 3
    s, w = np.zeros(n, np.int64), np.zeros(n, np.int32)
    colour = torch.zeros((len(f), 3), device=DEV)
    for cam in cams:
        depth = MeshRenderer(cam).render(vertices=vd, faces=fd, faces_color=colour)["depth"].cpu().numpy()
        assert (depth == 0).any() and (depth > 2.3).any()
        ref.integrate(s, w, vol.dims, vol.origin, vol.voxel_size, vol.trunc, cam.world_view_transform.cpu().numpy(), 0.45, 0.45, 48, 48, depth,
                      flags=ref.CARVE_UNCOVERED)
    assert np.array_equal(vol.sum.cpu().numpy().reshape(-1), s) and np.array_equal(vol.weight.cpu().numpy().reshape(-1), w)
    want_tri, _ = ref.extract(ref.field(s, w), vol.dims, vol.origin, vol.voxel_size)
    soup_v, soup_f = vol.extract(weld=False)
    assert np.array_equal(_bits(soup_v.cpu().numpy().reshape(-1, 3, 3)), _bits(want_tri))
    got_tri = fused.vertices[fused.faces.to(torch.int64)].cpu().numpy()
    assert fused.stats["num_faces"] == len(want_tri) and np.array_equal(got_tri, want_tri)  # the weld dropped nothing and moved nothing
    want_topo = ref.topology(ref.weld_exact(want_tri)[1])
    topo = mesh_topology(fused.stats["num_vertices"], fused.faces)
    print("fused", fused.stats, topo, "numpy pipeline", want_topo)
    assert (topo["edges"], topo["boundary"], topo["nonmanifold"], topo["euler"]) == tuple(want_topo[k] for k in ("edges", "boundary", "nonmanifold", "euler"))
    assert topo["boundary"] == 0 and topo["nonmanifold"] == 0 and topo["pieces"] == 1 and topo["euler"] == 2
    d = mesh_surface_distance((fused.vertices, fused.faces), (vd, fd), 4000, seed=0)
    print({k: d[k] for k in ("accuracy", "completeness", "chamfer", "hausdorff")}, "voxel", vol.voxel_size)
    assert d["hausdorff"] < vol.voxel_size  # below one voxel, at the worst sample either way


# ---- example ------------------------------------------------------------------------------------------------------------------------------------
def test_example_reports_the_fused_mesh():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_synthetic
    cfg = dict(iters=20, triangles=2000)
    _, m, _ = train_synthetic.train("2D", log=None, **cfg)
    fused = train_synthetic.mesh_scores(m, "2D", extract=32, **cfg)["fused"]
    lines = train_synthetic.fused_report(fused)
    print("\n".join(lines))
    assert len(lines) == 3 and lines[0].startswith("fused mesh, resolution 32:") and "the soup:" in lines[0]
    assert lines[1].startswith("fused mesh against the soup:") and lines[2].startswith("fused mesh against the target:")
    for k in ("boundary", "pieces", "euler", "faces"):
        assert k in fused["topology"] and k in fused["soup"]
    assert 0 < fused["soup"]["faces"] <= m._vertex.shape[0] and fused["soup"]["boundary"] > 0  # a soup of independent triangles is mostly boundary
