"""What a round of quadric-error edge contractions costs on an MI355X beside a round of half-edge collapses of the same mesh, and what placing
the survivors does to the shape -- beside decimate_mesh and vertex clustering at the same face count.

    python tools/bench_mesh_contract.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_contract.json]

Meshes (those of tools/bench_mesh_decimate.py):
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces
    soup          the triangles of synthetic.scene(--soup, ...), welded with weld_mesh(eps = 1e-3 of the scene's extent)

Time.  On each, in alternating blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest
block as the spread:

    contract_round  one contract_round with a budget of a quarter of the faces: the front, one decision per eligible edge -- two quadrics, the
                    solve and the rings of both ends where both are free -- the three sorts of the ranking, the selection, the face map,
                    the vertices, quadrics and blend that follow, one host read
    decimate_round  one decimate_round with the same budget on the same quadrics: a capability of the parent commit, timed in the same process
with ratio_decimate = contract_round / decimate_round; and, in blocks of one call each,

    contract_tenth  contract_mesh to a tenth of the faces and
    decimate_tenth  decimate_mesh to the same, compaction included: time, rounds, whether the target was reached.

Quality, on every mesh whose contraction collapsed anything: for the result of contract_tenth, of decimate_tenth and of simplify_mesh at the
cell size whose face count comes closest to contract_tenth's (bisection over the cell size), mesh_surface_distance to the input (accuracy,
completeness, Chamfer, Hausdorff; 100000 samples each way) and triangle_quality at the minimum, the 1st percentile and the median with the
number of needles (quality below 0.1).

Public wrappers throughout: allocation of outputs and workspaces and the read-backs included.  No figure here is a pass / fail condition.
Writes the JSON and prints it as one line."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="*", default=[100_000, 1_000_000], help="face counts of the remeshed sphere")
    ap.add_argument("--soup", type=int, default=100_000, help="triangles of the synthetic scene")
    ap.add_argument("--blocks", type=int, default=7, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=3, help="calls per block")
    ap.add_argument("--whole-blocks", type=int, default=3, help="blocks of one call for the contract_mesh / decimate_mesh parts")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=100_000, help="surface samples each way of the quality comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_contract.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_contract.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import (contract_mesh, contract_round, decimate_mesh, decimate_round, extract_isosurface, mesh_surface_distance, remesh,
                                simplify_mesh, triangle_quality, vertex_quadrics, weld_mesh)

    def block(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    def summary(v):
        return {"ms": round(statistics.median(v), 4), "min_block_ms": round(min(v), 4), "max_block_ms": round(max(v), 4)}

    def timed(parts, blocks, iters, warmup):
        for _ in range(warmup):
            for fn in parts.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in parts}
        for _ in range(blocks):
            for k, fn in parts.items():
                times[k].append(block(fn, iters))
        out = {k: summary(v) for k, v in times.items()}
        print(", ".join(f"{k} {v['ms']:.3f} ms" for k, v in out.items()), file=sys.stderr, flush=True)
        return out

    def shape(v, f):
        q = triangle_quality(v, f)
        q = q[~q.isnan()]
        if not q.numel():
            return None
        return {"faces": int(f.shape[0]), "min": float(q.min()), "p01": float(q.quantile(0.01)) if q.numel() <= 16_000_000 else None,
                "median": float(q.median()), "needles": int((q < 0.1).sum())}

    def distance(v, f, v0, f0):
        d = mesh_surface_distance((v, f), (v0, f0), args.samples, seed=0)
        return {k: float(d[k]) for k in ("accuracy", "completeness", "chamfer", "hausdorff")}

    def whole(m):
        return {"rounds": m.stats["rounds"], "reached": m.reached, "target_faces": m.stats["target_faces"], "faces": m.stats["num_faces"],
                "vertices": m.stats["num_vertices"], "collapsed": m.stats["collapsed"],
                "largest_cost": max((r["max_cost_collapsed"] for r in m.stats["per_round"]), default=None)}

    def clustered(v, f, want):
        """simplify_mesh at the cell size whose face count comes closest to `want`: bisection, the face count falls as the cell grows."""
        extent = float((v.max(dim=0).values - v.min(dim=0).values).max())
        lo, hi, best = extent / 4096.0, extent / 2.0, None
        for _ in range(24):
            cell = math.sqrt(lo * hi)
            s = simplify_mesh(v, f, cell)
            n = int(s.faces.shape[0])
            if best is None or abs(n - want) < abs(int(best[1].faces.shape[0]) - want):
                best = (cell, s)
            if n > want:
                lo = cell
            else:
                hi = cell
        return best

    def scored(m, v, f):
        return dict(shape(m.vertices, m.faces) or {"faces": 0}, vertices=int(m.vertices.shape[0]),
                    **(distance(m.vertices, m.faces, v, f) if m.faces.shape[0] else {}))

    def measure(v, f):
        F = int(f.shape[0])
        q = vertex_quadrics(v, f)
        t = timed({"contract_round": lambda: contract_round(v, f, q, F // 4), "decimate_round": lambda: decimate_round(v, f, q, F // 4)},
                  args.blocks, args.iters, args.warmup)
        t["contract_round"].update(budget=F // 4, stats=contract_round(v, f, q, F // 4).stats)
        t["decimate_round"].update(budget=F // 4, stats=decimate_round(v, f, q, F // 4).stats)
        t["ratio_decimate"] = round(t["contract_round"]["ms"] / t["decimate_round"]["ms"], 3)
        t.update(timed({"contract_tenth": lambda: contract_mesh(v, f, ratio=0.1), "decimate_tenth": lambda: decimate_mesh(v, f, ratio=0.1)},
                       args.whole_blocks, 1, 1))
        placed, kept = contract_mesh(v, f, ratio=0.1), decimate_mesh(v, f, ratio=0.1)
        t["contract_tenth"].update(whole(placed))
        t["decimate_tenth"].update(whole(kept))
        quality = None
        if placed.stats["collapsed"]:
            cell, s = clustered(v, f, int(placed.faces.shape[0]))
            quality = {"input": shape(v, f), "contracted": scored(placed, v, f), "decimated": scored(kept, v, f),
                       "clustered": dict(scored(s, v, f), cell=cell)}
        return t, quality

    g = torch.arange(48, device=dev, dtype=torch.float32) / 47.0
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    base = weld_mesh(*extract_isosurface((((x - 0.49) ** 2 + (y - 0.51) ** 2 + (z - 0.5) ** 2).sqrt() - 0.4).contiguous(), (0.0, 0.0, 0.0), 1.0 / 47.0), eps=0.0)
    probe = remesh((base.vertices, base.faces), 64)
    per_res2 = probe.faces.shape[0] / 64.0 ** 2
    meshes, shapes = {}, {}
    for N in args.faces:
        res = max(16, int(round(math.sqrt(N / per_res2))))
        m = remesh((base.vertices, base.faces), res)
        parts, quality = measure(m.vertices, m.faces)
        meshes[f"remesh_{N}"] = {"workload": f"remesh of a sphere at resolution {res}: {int(m.faces.shape[0])} faces, {int(m.vertices.shape[0])} vertices",
                                 "parts": parts}
        shapes[f"remesh_{N}"] = quality
        del m
        torch.cuda.empty_cache()

    tri = torch.from_numpy(np.ascontiguousarray(synthetic.scene(args.soup, 256, 192, 2, seed=0, edge_px=10.0)["vertex"])).to(dev)
    sv, sf = tri.reshape(-1, 3).contiguous(), torch.arange(3 * tri.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    extent = float((sv.max(dim=0).values - sv.min(dim=0).values).max())
    w = weld_mesh(sv, sf, eps=1e-3 * extent)
    parts, quality = measure(w.vertices, w.faces)
    meshes["soup"] = {"workload": f"synthetic.scene({args.soup}) welded with eps = 1e-3 of its extent: {int(w.faces.shape[0])} faces, "
                                  f"{int(w.vertices.shape[0])} vertices", "parts": parts}
    shapes["soup"] = quality

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of the two rounds after {args.warmup} warm-up calls each, "
                  f"{args.whole_blocks} alternating blocks of one call of contract_mesh and decimate_mesh after one warm-up call, device events around "
                  "each block; ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces and the "
                  "read-backs included); stats from calls of their own; budget of the round = a quarter of the faces; max_normal_deg = 30, no "
                  "max_cost, no max_edge, carried quadrics, regularization = 1e-3, reach = 1; quality: "
                  f"{args.samples} surface samples each way against the input, simplify_mesh at the cell size (bisection, 24 steps) whose face "
                  "count comes closest to the contracted mesh's",
        "meshes": meshes,
        "quality": shapes,
        "not_measured": "meshes above 1 M faces; the kernels alone without allocation and read-back; classify_kernel alone, its share of the round "
                        "and its achieved bandwidth; other values of regularization and reach; keep masks, pins, max_cost and max_edge; "
                        "memoryless quadrics; attribute blending; vertices of high valence",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
