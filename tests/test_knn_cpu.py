"""The bit-exact reference of the nearest-neighbour helpers (tests/ref_knn.py) checked without a GPU: the hand-worked demo points, the
float64 k-d tree oracle where no tie exists, the exactness of every shared input, and the rows that take no part."""
import numpy as np
import pytest

import ref_knn as RK
from oracle import ts_knn_oracle as KO

DEMO = np.array([[0, 0, .1], [.5, 0, 0], [0, 1, 0], [0, 3, .1], [.5, 3, 0], [0, 4, 0], [3, 0, .1], [3.5, 0, 0], [3, 1, 0]], np.float32)


def test_demo_points_tie_goes_to_the_first_in_morton_order():
    """tests/test_knn_gpu.py::test_reference_demo_points works the codes out by hand: point 0 is exactly 3 away from points 3 and 6, and with the
    origin-seeded box (0,0,0)-(3.5,4,.1) point 6 sorts first."""
    r = RK.search(DEMO, 3, exact=False)  # .1 and .5 are no dyadic rationals: the tie of point 0 is exact all the same (3^2 either way)
    assert r["ties"][0] == 2 and r["nearest"][0] == 6
    assert r["pos"][6] < r["pos"][3]
    assert r["nearest"][2] == 3 and r["nearest"][3] == 2 and r["nearest"][6] == 1
    lo, hi = RK.bounding_box(DEMO)
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, np.array([3.5, 4, .1], np.float32))


def _spread(v):
    """Bit b of v to bit 3 b, one bit at a time."""
    return sum(((int(v) >> b) & 1) << (3 * b) for b in range(10))


def test_morton_codes_by_hand():
    # box (0,0,0)-(4,4,4): t = (v / 4) * 1023 is exact in float32: 0, 255.75, 511.5, 767.25, 1023 -> 0, 255, 511, 767, 1023
    cell = {0: 0, 1: 255, 2: 511, 3: 767, 4: 1023}
    p = np.array([[0, 0, 0], [4, 4, 4], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 2, 1], [2, 4, 3]], np.float32)
    want = [_spread(cell[x]) | (_spread(cell[y]) << 1) | (_spread(cell[z]) << 2) for x, y, z in p.astype(int).tolist()]
    assert RK.morton_codes(p).tolist() == want and want[1] == (1 << 30) - 1
    assert np.array_equal(RK.morton_order(p), np.argsort(np.argsort(want, kind="stable"), kind="stable"))
    # the same cloud in the negative octant has the box (-4, 0): -k sits in the cell of 4 - k, the origin gets all ones
    mirrored = [_spread(cell[4 - x]) | (_spread(cell[4 - y]) << 1) | (_spread(cell[4 - z]) << 2) for x, y, z in p.astype(int).tolist()]
    assert RK.morton_codes(-p).tolist() == mirrored and mirrored[0] == (1 << 30) - 1
    # the origin seed: moved off the origin to 8 ... 12 the box stays (0, 12) and only the upper third of the grid is used
    # ((8 + k) / 12) * 1023 = 682, 767.25, 852.5, 937.75, 1023
    far = {0: 682, 1: 767, 2: 852, 3: 937, 4: 1023}
    assert RK.morton_codes(p + np.float32(8)).tolist() == [_spread(far[x]) | (_spread(far[y]) << 1) | (_spread(far[z]) << 2)
                                                           for x, y, z in p.astype(int).tolist()]
    # zero extent: 0 / 0 = NaN -> cell 0 on that axis
    flat = np.array([[0, 0, 0], [4, 0, 0], [2, 0, 0]], np.float32)
    assert RK.morton_codes(flat).tolist() == [0, _spread(1023), _spread(511)]
    # NaN is ignored by the box and quantised to 0; an infinite coordinate sends its whole axis to cell 0 (finite / inf = 0, inf / inf = NaN)
    bad = np.array([[0, 0, 0], [4, 4, 4], [np.nan, 4, 0], [np.inf, 0, 4], [2, 2, 2]], np.float32)
    lo, hi = RK.bounding_box(bad)
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, np.array([np.inf, 4, 4], np.float32))
    assert RK.morton_codes(bad).tolist() == [0, (_spread(1023) << 1) | (_spread(1023) << 2), _spread(1023) << 1, _spread(1023) << 2,
                                             (_spread(511) << 1) | (_spread(511) << 2)]
    # equal codes keep index order
    same = np.array([[1, 1, 1]] * 4 + [[0, 0, 0]], np.float32)
    assert RK.morton_order(same).tolist() == [1, 2, 3, 4, 0]


@pytest.mark.parametrize("n,g", [(9, 3), (700, 1), (1500, 3), (2048, 1024), (64, 64)])
def test_reference_equals_the_kd_tree_oracle_without_ties(n, g):
    rng = np.random.default_rng(n)
    p = rng.random((n, 3), dtype=np.float32) * np.array([10, 6, 3], np.float32) - np.array([3, 0, 1], np.float32)
    r = RK.search(p, g, exact=False)
    if n == g:  # no candidate anywhere: the documented nearest[i] = i
        assert np.array_equal(r["nearest"], np.arange(n)) and np.isinf(r["d2"]).all() and (r["ties"] == 0).all()
    else:
        assert (r["ties"] == 1).all()
        idx, d2 = KO.nearest_other(p, g)
        assert np.array_equal(r["nearest"], idx)
        np.testing.assert_allclose(r["d2"], d2, rtol=1e-12)
    np.testing.assert_allclose(r["mean3"].astype(np.float64), KO.mean_dist3(p), rtol=4 * 2.0 ** -24)  # three float32 roundings and the division


def test_fewer_than_four_points_count_missing_neighbours_as_flt_max():
    p = np.array([[0., 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    for n in (1, 2):
        got = RK.mean_dist3(p[:n])
        assert got.shape == (n,) and (got == np.inf).all()  # FLT_MAX * 3 overflows like the reference
    # three points: two real neighbours and one FLT_MAX
    want = [(np.float32(1) + np.float32(4) + RK.FLT_MAX) / np.float32(3), (np.float32(1) + np.float32(5) + RK.FLT_MAX) / np.float32(3),
            (np.float32(4) + np.float32(5) + RK.FLT_MAX) / np.float32(3)]
    assert RK.mean_dist3(p).tolist() == [float(w) for w in want]
    np.testing.assert_allclose(RK.mean_dist3(p).astype(np.float64), KO.mean_dist3(p), rtol=1e-6)
    assert RK.nearest_other(p[:1], 1)[0].tolist() == [0]
    assert RK.search(np.zeros((0, 3), np.float32))["nearest"].shape == (0,)


@pytest.mark.parametrize("name", sorted(RK.INPUTS))
def test_every_shared_input_is_exact_in_float32(name):
    """search(exact=True) asserts that each finite squared distance is a float32 number; so does every scale and shift of the lattice."""
    g = 1 if name in ("plane0", "plane5", "edge") else 3
    p, r = RK.solve(name, g)
    assert len(p) > 2 * RK.BOX and len(p) % g == 0
    finite = np.isfinite(p).all(1)
    if name == "doubled":  # the one nearest candidate is the twin (unless it shares the group); this input's ties are among the three nearest: 0, 1, 1
        assert (r["d2"] == 0).mean() > 0.99 and (r["mean3"] == np.float32(2) / np.float32(3)).mean() > 0.9
    else:  # the inputs are there for their ties
        assert (r["ties"][finite] >= 2).mean() >= 0.5, (name, float((r["ties"][finite] >= 2).mean()))
    assert np.array_equal(r["nearest"][~finite], np.nonzero(~finite)[0]) and np.isinf(r["mean3"][~finite]).all()
    assert np.isfinite(r["mean3"][finite]).all() and finite[r["nearest"][finite]].all()


@pytest.mark.parametrize("shift", [0.0, -6.5, -20.0, 1000.0])
@pytest.mark.parametrize("scale", [2.0 ** -20, 1.0, 2.0 ** 20])
def test_moved_and_scaled_lattices_are_exact_and_full_of_ties(shift, scale):
    p, r = RK.solve("lattice", 3, shift=shift, scale=scale)
    assert len(p) == 2742 and (r["ties"] >= 2).mean() >= 0.5
    base = RK.solve("lattice", 3, shift=shift, scale=1.0)[1]
    assert np.array_equal(r["nearest"], base["nearest"])  # a power of two scales every fp32 operation of the front half exactly


def test_the_tie_rule_is_not_the_smallest_index():
    """The lattice separates 'first in Morton order' from 'smallest index': most winners differ."""
    p, r = RK.solve("lattice", 3)
    n = len(p)
    grp = np.arange(n) // 3
    p64 = p.astype(np.float64)
    differ = 0
    for i in range(0, n, 7):
        d2 = ((p64 - p64[i]) ** 2).sum(1)
        d2[grp == grp[i]] = np.inf
        differ += int(np.argmin(d2) != r["nearest"][i])  # argmin: the smallest index at the minimum
        assert d2[r["nearest"][i]] == d2.min() == r["d2"][i]
    assert differ > 0.5 * len(range(0, n, 7))


@pytest.mark.parametrize("name,g", [("nan", 1), ("nan", 3), ("inf", 3)])
def test_non_finite_rows_take_no_part(name, g):
    """The finite rows answer as the finite subset alone does, indices mapped back, PROVIDED both are ordered by the same codes: the non-finite
    rows leave the bounding box alone when they hold NaN (fminf / fmaxf ignore it), so there the subset can be searched on its own.  An infinite
    coordinate changes the grid, so there only the distances and the candidate sets are compared."""
    p, r = RK.solve(name, g)
    finite = np.isfinite(p).all(1)
    keep = np.nonzero(finite)[0]
    assert 0 < (~finite).sum() < len(p)
    assert np.array_equal(r["nearest"][~finite], np.nonzero(~finite)[0])
    assert np.isinf(r["mean3"][~finite]).all() and (r["mean3"][~finite] > 0).all()
    # the subset with each point's ORIGINAL group: search it with explicit groups by brute force
    q = p[keep].astype(np.float64)
    grp = keep // g
    pos = RK.morton_order(p)[keep]
    if name == "nan":
        assert np.array_equal(np.argsort(pos), np.argsort(RK.morton_order(p[keep]), kind="stable"))  # the same order with and without the NaN rows
    for a in range(0, len(keep), 5):
        d2 = ((q - q[a]) ** 2).sum(1)
        other = np.delete(d2, a)
        b3 = np.sort(other)[:3].astype(np.float32)
        assert r["mean3"][keep[a]] == ((b3[0] + b3[1]) + b3[2]) / np.float32(3)
        d2[grp == grp[a]] = np.inf
        tie = np.nonzero(d2 == d2.min())[0]
        assert r["nearest"][keep[a]] == keep[tie[np.argmin(pos[tie])]]
        assert r["ties"][keep[a]] == len(tie)
