"""GPU parity of the simple_knn drop-in (csrc/knn.hip through simple_knn -> ctypes -> C ABI) against the exact-search
oracle (oracle/ts_knn_oracle.py, scipy k-d tree in float64) on random clouds, and -- bit for bit, indices and distances, no
outlier budget -- against the numpy reference that restates the tie rule (tests/ref_knn.py) on inputs made of exact ties:
lattices around, across and far from the origin, box and group edges, zero extents, duplicates, a twinned mesh and rows with
NaN or infinite coordinates."""
import numpy as np
import pytest

import ref_knn as RK
from oracle import ts_knn_oracle as KO

pytestmark = pytest.mark.gpu


def _pts(n, seed, kind="uniform"):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, 3), dtype=np.float32) * np.array([10, 6, 3], np.float32)
    if kind == "clustered":  # most points in tight clusters, a few far away: long box lists, uneven radii
        c = rng.normal(size=(8, 3)).astype(np.float32) * 20
        p = c[rng.integers(0, 8, n)] + rng.normal(size=(n, 3)).astype(np.float32) * 0.05
        p[: n // 50] = rng.normal(size=(n // 50, 3)).astype(np.float32) * 100
        return p.astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("n,kind", [(9, "uniform"), (1000, "uniform"), (1025, "uniform"), (5000, "clustered"),
                                    (200_000, "uniform"), (100_000, "clustered")])
def test_mean_dist3_matches_exact_search(n, kind):
    import torch
    from simple_knn import distCUDA2
    p = _pts(n, n, kind)
    got = distCUDA2(torch.from_numpy(p).cuda()).cpu().numpy().astype(np.float64)
    want = KO.mean_dist3(p)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-12)


@pytest.mark.parametrize("n,g,kind", [(9, 3, "uniform"), (3000, 3, "uniform"), (3072, 1, "uniform"), (60_000, 3, "clustered"),
                                      (150_000, 3, "uniform"), (4096, 1024, "uniform")])
def test_nearest_other_matches_exact_search(n, g, kind):
    import torch
    from simple_knn import nearestNeighbor
    p = _pts(n, 7 * n + g, kind)
    got = nearestNeighbor(torch.from_numpy(p).cuda(), g)
    assert got.dtype == torch.uint32
    got = got.view(torch.int32).cpu().numpy().astype(np.int64)
    idx, d2 = KO.nearest_other(p, g)
    assert ((got // g) != (np.arange(n) // g)).all()
    same = got == idx
    # where the index differs the distances must tie to fp32 rounding (the search is exact, ties are broken by Morton order)
    dg = ((p[got].astype(np.float64) - p.astype(np.float64)) ** 2).sum(1)
    assert np.all(same | (np.abs(dg - d2) <= 1e-6 * np.maximum(d2, 1e-12)))
    assert same.mean() > 0.999
    if n <= 5000:  # ... and by Morton order means: exactly the reference's winner (its brute force is affordable up to a few thousand points)
        assert np.array_equal(got[~same], RK.nearest_other(p, g, exact=False)[0][~same])


def test_reference_demo_points():
    """The nine points of submodules/simple-knn/main.cu:53-61 (three clusters of three), results worked out by hand."""
    import torch
    from simple_knn import distCUDA2, nearestNeighbor
    p = np.array([[0, 0, .1], [.5, 0, 0], [0, 1, 0], [0, 3, .1], [.5, 3, 0], [0, 4, 0], [3, 0, .1], [3.5, 0, 0], [3, 1, 0]], np.float32)
    t = torch.from_numpy(p).cuda()
    d = distCUDA2(t).cpu().numpy()
    np.testing.assert_allclose(d, KO.mean_dist3(p), rtol=1e-6)
    nn = nearestNeighbor(t, 3).view(torch.int32).cpu().numpy()
    # nearest point of ANOTHER triple: cluster {0,1,2} <-> {3,4,5} along y, {6,7,8} reaches back to {0,1,2} along x
    idx, d2 = KO.nearest_other(p, 3)
    dg = ((p[nn].astype(np.float64) - p) ** 2).sum(1)
    np.testing.assert_allclose(dg, d2, rtol=1e-6)
    assert nn[2] == 3 and nn[3] == 2 and nn[6] == 1
    # point 0 is exactly 3 away from both point 3 (0, 3, .1) and point 6 (3, 0, .1): the reference keeps the first one met
    # in Morton order (strict `<`, simple_knn.cu:229).  With the origin-seeded box (0,0,0)-(3.5,4,.1) the leading
    # (z, y, x) bit triples are (1,1,0) for point 3 and (1,0,1) for point 6, so point 6 sorts first.
    assert nn[0] == 6


def test_small_inputs_and_errors():
    import torch
    from simple_knn import distCUDA2, nearestNeighbor
    assert distCUDA2(torch.zeros((0, 3), device="cuda")).shape == (0,)
    one = distCUDA2(torch.rand((1, 3), device="cuda"))
    assert torch.isinf(one).all()  # three missing neighbours: FLT_MAX * 3 overflows like the reference
    three = distCUDA2(torch.tensor([[0., 0, 0], [1, 0, 0], [0, 2, 0]], device="cuda")).cpu().numpy()
    np.testing.assert_allclose(three, KO.mean_dist3(np.array([[0., 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)), rtol=1e-6)
    dup = torch.tensor([[1., 1, 1]] * 5, device="cuda")  # duplicates are neighbours at distance 0
    assert (distCUDA2(dup) == 0).all()
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros((4, 2), device="cuda"))
    with pytest.raises(RuntimeError):
        nearestNeighbor(torch.zeros((4, 3), device="cuda"), 3)
    with pytest.raises(RuntimeError):
        nearestNeighbor(torch.zeros((4, 3), device="cuda"), 0)
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros((4, 3)))


# ---- exact cases: every coordinate a small integer times a power of two, so fp32 equality is the criterion (tests/ref_knn.py) ------------------
def _run(p, g):
    import torch
    from simple_knn import distCUDA2, nearestNeighbor
    t = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    nn = nearestNeighbor(t, g)
    assert nn.dtype == torch.uint32
    return nn.view(torch.int32).cpu().numpy().astype(np.int64), distCUDA2(t).cpu().numpy()


def _assert_exact(p, r, g, tie_share=None):
    """Indices equal and the fp32 bit patterns of the mean distances equal, on every row; a non-finite row answers itself and +inf."""
    nn, md = _run(p, g)
    finite = np.isfinite(p).all(1)
    if tie_share is not None:  # the input is not vacuous: that many of its points have more than one candidate at the minimal distance
        assert (r["ties"][finite] >= 2).mean() >= tie_share
    bad = np.nonzero(~finite)[0]
    assert np.array_equal(nn[bad], bad) and np.array_equal(md[bad].view(np.uint32), np.full(len(bad), 0x7F800000, np.uint32))
    wrong = np.nonzero(nn != r["nearest"])[0]
    assert len(wrong) == 0, (len(wrong), wrong[:5], nn[wrong[:5]], r["nearest"][wrong[:5]])
    want = r["mean3"]  # the three nearest ignore the groups
    wrong = np.nonzero(md.view(np.uint32) != want.view(np.uint32))[0]
    assert len(wrong) == 0, (len(wrong), wrong[:5], md[wrong[:5]], want[wrong[:5]])


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("scale", [2.0 ** -20, 1.0, 2.0 ** 20])
@pytest.mark.parametrize("shift", [0.0, -6.5, -20.0, 1000.0])
def test_lattice_ties_go_to_the_first_in_morton_order(shift, scale, g):
    """The shuffled 14^3 lattice (2742 points, three boxes): every point has a tie.  shift 0: the origin is a corner of the box; -6.5: inside;
    -20: every coordinate negative, the origin seed enlarges the box; +1000: far from the origin, a coarse grid of many equal codes, ties fall
    to index order."""
    p, r = RK.solve("lattice", g, shift=shift, scale=scale)
    _assert_exact(p, r, g, tie_share=0.5)


@pytest.mark.parametrize("n,g", [(1023, 1), (1024, 1), (1025, 1), (2048, 1), (2049, 1), (1023, 3), (1026, 3), (2049, 3), (2048, 1024), (3072, 1024),
                                 (1500, 1500)])
def test_box_and_group_edges(n, g):
    """One box less one, exactly one, one more, two, two and one; groups as large as a box; one group only (no candidate: nearest[i] = i)."""
    p, r = RK.solve("edge", g, n=n)
    if n == g:
        assert np.array_equal(r["nearest"], np.arange(n))
    _assert_exact(p, r, g, tie_share=None if n == g else 0.5)


@pytest.mark.parametrize("name,g", [("plane0", 1), ("plane0", 4), ("plane5", 1), ("plane5", 4), ("line", 1), ("line", 3)])
def test_zero_extents(name, g):
    """A plane through the origin (z extent 0: 0 / 0 in the quantisation), a plane at z = 5 (every z on the box's face), a line (two zero extents)."""
    p, r = RK.solve(name, g)
    _assert_exact(p, r, g, tie_share=0.5)


@pytest.mark.parametrize("name,g", [("copies", 1), ("copies", 3), ("doubled", 1), ("doubled", 3)])
def test_duplicates(name, g):
    """1100 copies of one point among 1000 lattice points: the mean distance of a copy is 0 and its nearest is the first copy in (code, index)
    order outside its group.  The lattice twice over: the twin is the one nearest, the three nearest are 0, 1, 1."""
    p, r = RK.solve(name, g)
    if name == "copies":
        copy = (p == np.array([3, 4, 5], np.float32)).all(1)
        assert copy.sum() >= 1100 and (r["mean3"][copy] == 0).all() and (r["ties"][copy] >= 1097).all()
    _assert_exact(p, r, g, tie_share=0.5 if name == "copies" else None)


def test_twinned_mesh_vertices():
    """What the trainer's nearest-vertex regulariser sees: a triangle soup over a shared-vertex grid with its back-face twins, group = 3."""
    p, r = RK.solve("twinned", 3)
    assert r["ties"].max() == 11 and (r["d2"] == 0).all()
    _assert_exact(p, r, 3, tie_share=0.5)


@pytest.mark.parametrize("name,g", [("nan", 1), ("nan", 3), ("inf", 1), ("inf", 3)])
def test_non_finite_rows_take_no_part(name, g):
    """5 % of the rows with a NaN coordinate; one row with x = +inf and one with y = -inf (two axes of the Morton grid degenerate).  The finite
    rows equal the reference, in which a non-finite row is nobody's candidate; a non-finite row gets its own index and +inf."""
    p, r = RK.solve(name, g)
    assert not np.isfinite(p).all()
    _assert_exact(p, r, g, tie_share=0.5)
