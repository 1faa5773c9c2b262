"""GPU test of the four queries on the triangle index, three of them on the one walk of csrc/ts_bvh_walk.h: tests/golden/bvh_walk.npz, recorded on the GPU
before the walks were single-sourced (tests/golden/make_golden_bvh_walk.py), replayed bit for bit.

Every output is an integer or correctly rounded under -ffp-contract=off, so it is compared for equality, the (wave, leaf) visit counts and the
winding number's term counts included: those pin the order and the pruning of the walk, which no face result would notice.  The one
exception is wq of a query that evaluated faces: only atan2 may differ between toolchains, by a few ulp, which moves a quantised face term
by at most one unit (tests/test_mesh_winding_gpu.py), so |wq - golden| <= terms[:, 0] there."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_bvh_walk", os.path.join(GOLDEN, "make_golden_bvh_walk.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


GEN = _generator()  # defines CASES and the functions; reads no file and imports no torch until a function is called


@pytest.fixture(scope="module")
def record():
    return GEN.load()


def _bits(a):
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def test_the_record_holds_the_cases_it_is_meant_to(record):
    RECORD = record
    assert list(RECORD) == [c[0] for c in GEN.CASES]
    assert {len(r["f"]) for r in RECORD.values()} == {1, 8, 9, 65, 521} and {len(r["o"]) for r in RECORD.values()} == {1, 64, 65, 257, 321}
    assert os.path.getsize(os.path.join(GOLDEN, "bvh_walk.npz")) < 200 * 1024
    quarter, none, allbad = RECORD["quarter521_q65"], RECORD["none9_q64"], RECORD["soup65_allbad_q65"]
    assert int(quarter["keep"].sum()) * 4 <= len(quarter["keep"]) + 3 and not none["keep"].any()
    assert not np.isfinite(allbad["o"]).all(axis=1).any() and not any(int(allbad[k][0]) for k in allbad if k.endswith("_visits"))
    big = RECORD["soup521_q321"]
    bad = ~np.isfinite(big["o"]).all(axis=1)
    assert 0.05 < bad.mean() < 0.2 and np.isnan(big["tl"]).any() and (big["d"] == 0).all(axis=1).any() and (~np.isfinite(big["d"])).any()
    assert (big["rc0_face"] >= 0).sum() > 200 and big["w2_terms"][:, 1].max() > 0  # rays that hit, nodes that were accepted


@pytest.mark.parametrize("case", [c[0] for c in GEN.CASES])
def test_the_four_queries_answer_what_they_answered_before(record, case):
    want = record[case]
    got = GEN.run(want["v"], want["f"], want["keep"], want["o"], want["d"], want["tl"])
    outputs = [k for k in want if k not in ("v", "f", "keep", "o", "d", "tl")]
    assert sorted(got) == sorted(outputs) and len(outputs) == 26
    for k in outputs:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if k.endswith("_wq"):
            faces = np.maximum(want[k.replace("_wq", "_terms")][:, 0], 0)  # 0 faces evaluated (or a bad point): bit for bit
            assert (np.abs(got[k] - want[k]) <= faces).all(), (case, k, np.nonzero(np.abs(got[k] - want[k]) > faces)[0][:10])
        else:
            same = _bits(got[k]) == _bits(want[k])
            assert same.all(), (case, k, np.nonzero(~same.reshape(len(same), -1).all(axis=1))[0][:10], got[k][~same][:5], want[k][~same][:5])
