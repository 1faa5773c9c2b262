"""Records what the four queries on the triangle index answer, as tests/golden/bvh_walk.npz (needs the GPU) and
tests/golden/bvh_walk_bytes.json (host code, no GPU):

    python triangle-splatting_amd/build.py && python tests/golden/make_golden_bvh_walk.py [--out DIR] [--bytes-only]

Both records were taken from the commit before the walks of the index were single-sourced (csrc/ts_bvh_walk.h).
tests/test_bvh_walk_gpu.py replays bvh_walk.npz and holds every later build to it bit for bit, the (wave, leaf) visit counts and the
winding number's term counts included: those pin the ORDER and the PRUNING of the walk, which neither the face results nor a float64
reference would notice.  tests/test_bvh_walk_cpu.py holds the four workspace size queries to bvh_walk_bytes.json.  Run it again only when
a walk or a workspace is meant to change.

Shapes: the smallest at which the walk can go wrong.  F in {1, 8, 9, 65, 521} (521 faces: 66 leaves, 9, 2, 1 nodes, a ragged last group on
every level; 1 and 8: the root is a leaf), from ref_mesh_distance.heavy_tailed_soup and ref_mesh_surface.grid_mesh (exact ties on shared
edges and vertices); a mesh whose keep mask drops three faces in four (the trailing leaves and inner nodes are empty boxes); a mesh with
no eligible face; Q in {1, 64, 65, 257, 321} (257: one lane in a second workgroup); about one query in ten non-finite, for rays a few zero
or non-finite directions and NaN limits as well; one call whose queries are all non-finite, so that every wave skips the walk.

Stored: every array is the concatenation over CASES (names in `cases`) along its first axis; counts[c] = (V, F, Q) of case c gives the
rows that are its own (load() below cuts them out again), a *_visits array has one row per case.  Inputs: v, f, keep (all ones where
has_keep[c] is 0: that case passes None), o (the points and the ray origins), d, tl.  Outputs:
  closest     cl_face, cl_dist2, cl_point, cl_visits
  ray_cast    rcK_face, rcK_t, rcK_bary, rcK_side, rcK_visits   K = 0: cull_back False, no limit;  K = 1: cull_back True, t_limit = tl
  crossings   xK_hits, xK_winding2, xK_touches, xK_visits       K = 0: per-ray directions d, t_limit = tl;  K = 1: SHARED direction, no limit
  winding     wB_wq, wB_terms                                   B = 2: beta 2;  B = inf: the exact sum
"""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PACKAGE = os.path.join(ROOT, "triangle-splatting_amd")
for _p in (PACKAGE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SHARED_DIRECTION = (0.7548777, 0.5698403, 0.3247180)
# (name, generator, F, keep rule, Q, all queries bad)
CASES = (
    ("soup1_q1", "soup", 1, None, 1, False), ("grid1_q1", "grid", 1, None, 1, False),
    ("soup8_q1", "soup", 8, None, 1, False), ("grid8_q1", "grid", 8, None, 1, False),
    ("soup9_q1", "soup", 9, None, 1, False), ("grid9_q64", "grid", 9, None, 64, False),
    ("soup65_q65", "soup", 65, None, 65, False), ("grid65_q1", "grid", 65, None, 1, False),
    ("soup521_q321", "soup", 521, None, 321, False), ("grid521_q257", "grid", 521, None, 257, False),
    ("quarter521_q65", "grid", 521, "quarter", 65, False), ("none9_q64", "soup", 9, "none", 64, False),
    ("soup65_allbad_q65", "soup", 65, None, 65, True),
)
# the four workspace size queries -> their library below diff_recon_hip
QUERIES = {"tsb_closest_workspace_bytes": "libts_bvh.so", "tsr_cast_workspace_bytes": "libts_ray.so",
           "tsi_crossings_workspace_bytes": "libts_inside.so", "tsn_winding_workspace_bytes": "libts_winding.so"}
SMALL_BELOW = 2500000  # TS_RS_SMALL_BELOW of csrc/ts2d_common.h
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, SMALL_BELOW - 1, SMALL_BELOW, SMALL_BELOW + 1, 5000000, 2 ** 31 - 1025)


def measure_bytes(package=PACKAGE):
    out = {"sizes": list(SIZES), "queries": {}}
    for name, lib in QUERIES.items():
        query = getattr(ctypes.CDLL(os.path.join(package, "diff_recon_hip", lib)), name)
        query.restype, query.argtypes = ctypes.c_size_t, [ctypes.c_int32]
        out["queries"][name] = [query(n) for n in SIZES]
    return out


def inputs(case):
    """The inputs of one case, from its own seed: v, f, keep (or None), o (Q, 3), d (Q, 3), tl (Q,), all numpy."""
    import ref_mesh_distance as refd
    import ref_mesh_surface as refs
    name, kind, F, rule, Q, allbad = case
    seed = 1000 * F + Q
    if kind == "soup":
        v, f = refd.heavy_tailed_soup(F, seed=F)
    else:
        v, f = refs.grid_mesh(max(1, int(np.ceil(np.sqrt(F / 2)))), seed=F)
        f = f[:F]
    assert len(f) == F
    keep = None
    if rule == "quarter":
        keep = (np.arange(F) % 4 == 1).astype(np.uint8)
    elif rule == "none":
        keep = np.zeros(F, np.uint8)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    o = mid + rng.uniform(-2.0, 2.0, (Q, 3)) * half
    near = np.arange(Q) % 4 == 3  # every fourth query lies close to a vertex
    o[near] = v[rng.integers(0, len(v), int(near.sum()))] + rng.normal(size=(int(near.sum()), 3)) * 1e-2 * half
    corners = v[f[rng.integers(0, F, Q)]].astype(np.float64)  # every ray aims at a point of a face
    at = (corners * rng.dirichlet((1.0, 1.0, 1.0), Q)[:, :, None]).sum(axis=1)
    d = (at - o) * rng.uniform(0.5, 2.0, (Q, 1))  # t counts in units of |d|
    o, d = o.astype(np.float32), d.astype(np.float32)
    plumb = np.arange(Q) % 5 == 2  # straight down onto a vertex, x and y exact: a tie between the faces around it
    o[plumb] = v[rng.integers(0, len(v), int(plumb.sum()))] + np.array([0, 0, 1], np.float32)
    d[plumb] = (0, 0, -1)
    tl = (np.linalg.norm(at - o, axis=1) / np.maximum(np.linalg.norm(d, axis=1), 1e-30) * rng.uniform(0.2, 3.0, Q)).astype(np.float32)
    tl[rng.random(Q) < 0.1] = np.inf
    bad = rng.random(Q) < 0.1
    if allbad:
        bad[:] = True
    o[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    if not allbad:
        pick = rng.random(Q)
        d[pick < 0.03] = 0.0
        odd = (pick >= 0.03) & (pick < 0.06)
        d[odd, rng.integers(0, 3, int(odd.sum()))] = rng.choice(np.array([np.nan, np.inf], np.float32), int(odd.sum()))
        tl[(pick >= 0.06) & (pick < 0.09)] = np.nan
    return v, f, keep, o, d, tl


def run(v, f, keep, o, d, tl, device="cuda"):
    """Every output of the four queries on one case's inputs, through the Python API, as {key: numpy array}."""
    import torch
    from diff_recon_hip import MeshBVH, generalized_winding_number

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)

    def counter():
        return torch.zeros((1,), device=device, dtype=torch.int64)

    out = {}
    bvh = MeshBVH(dev(v), dev(f), dev(keep))
    o_, d_, tl_ = dev(o), dev(d), dev(tl)
    n = counter()
    face, dist2, point = bvh.closest(o_, leaf_visits=n)
    out.update(cl_face=face, cl_dist2=dist2, cl_point=point, cl_visits=n)
    for k, (cull, limit) in enumerate(((False, None), (True, tl_))):
        n = counter()
        h = bvh.ray_cast(o_, d_, t_limit=limit, cull_back=cull, leaf_visits=n)
        out.update({f"rc{k}_face": h.face, f"rc{k}_t": h.t, f"rc{k}_bary": h.bary, f"rc{k}_side": h.side, f"rc{k}_visits": n})
    for k, (dirs, limit) in enumerate(((d_, tl_), (torch.tensor(SHARED_DIRECTION, device=device, dtype=torch.float32), None))):
        n = counter()
        x = bvh.ray_crossings(o_, dirs, t_limit=limit, leaf_visits=n)
        out.update({f"x{k}_hits": x.hits, f"x{k}_winding2": x.winding2, f"x{k}_touches": x.touches, f"x{k}_visits": n})
    for tag, beta in (("2", 2.0), ("inf", float("inf"))):
        _, wq, terms = generalized_winding_number(o_, bvh, beta=beta, return_terms=True)
        out.update({f"w{tag}_wq": wq, f"w{tag}_terms": terms})
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def load(path=os.path.join(HERE, "bvh_walk.npz")):
    """{case name: {key: its rows}} of a record written below; keep is None where the case passed none."""
    z = np.load(path)
    ends = np.cumsum(z["counts"], axis=0)
    starts = ends - z["counts"]
    column = {"v": 0, "f": 1, "keep": 1}  # of counts: the rows of v are counted by V, those of f and keep by F, every other array's by Q
    out = {}
    for c, name in enumerate(z["cases"]):
        one = {}
        for k in z.files:
            if k in ("cases", "counts", "has_keep"):
                continue
            col = column.get(k, 2)
            first, last = (c, c + 1) if k.endswith("_visits") else (starts[c, col], ends[c, col])
            one[k] = z[k][first:last]
        if not z["has_keep"][c]:
            one["keep"] = None
        out[str(name)] = one
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE, help="the directory the two records are written to")
    ap.add_argument("--bytes-only", action="store_true", help="bvh_walk_bytes.json alone: no GPU needed")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if not a.bytes_only:
        import torch  # noqa: F401  (before measure_bytes loads a library of ours: the process is to hold one HIP runtime, torch's)
    path = os.path.join(a.out, "bvh_walk_bytes.json")
    with open(path, "w") as fh:
        text = json.dumps(measure_bytes(), indent=1)
        fh.write(re.sub(r"\[\s+([\d,\s]+?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text) + "\n")  # a row of numbers on one line
    print("bvh_walk_bytes.json:", os.path.getsize(path), "bytes")
    if not a.bytes_only:
        parts = []
        for case in CASES:
            v, f, keep, o, d, tl = inputs(case)
            got = run(v, f, keep, o, d, tl)
            parts.append(dict(got, v=v, f=f, keep=np.ones(len(f), np.uint8) if keep is None else keep, o=o, d=d, tl=tl,
                              has_keep=np.array([keep is not None], np.uint8), counts=np.array([[len(v), len(f), len(o)]], np.int32)))
            print(case[0], {k: int(x[0]) for k, x in got.items() if k.endswith("_visits")}, "faces hit", int((got["rc0_face"] >= 0).sum()),
                  "terms", got["w2_terms"].clip(0).sum(axis=0).tolist())
        path = os.path.join(a.out, "bvh_walk.npz")
        np.savez_compressed(path, cases=np.array([c[0] for c in CASES]), **{k: np.concatenate([p[k] for p in parts]) for k in parts[0]})
        print("bvh_walk.npz:", os.path.getsize(path), "bytes")
