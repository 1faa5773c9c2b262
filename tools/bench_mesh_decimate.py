"""What a round of quadric-error collapses and a whole decimate_mesh cost on an MI355X, beside a round of length-ordered collapses and the
edge table of the same mesh, and what the decimation does to the shape -- beside vertex clustering at the same face count.

    python tools/bench_mesh_decimate.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_decimate.json]

Meshes (those of tools/bench_mesh_collapse.py):
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces
    soup          the triangles of synthetic.scene(--soup, ...), welded with weld_mesh(eps = 1e-3 of the scene's extent)

On each, in alternating blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest block as the
spread:

    quadrics        vertex_quadrics: the corner records, their sort, one ring walk per vertex
    decimate_round  one decimate_round with a budget of a quarter of the faces: the front, the classification of BOTH directions of every
                    eligible edge, the three sorts of the ranking, the selection, the face map, the quadric merge, one host read
    collapse_round  one collapse_edges round with min_edge = the 20th percentile of the edge lengths, and
    edges           mesh_edges with lengths: capabilities of the parent commit on the same front, timed in the same process
with ratio_collapse = decimate_round / collapse_round and ratio_edges = decimate_round / edges; and, in blocks of one call each,

    decimate_half   decimate_mesh to half the faces and
    decimate_tenth  to a tenth, compaction included: time, rounds, whether the target was reached, and per round the share of the candidates
                    in budget that won (the width of the independent set)

Quality, on every mesh whose decimation collapsed anything: for the result of decimate_tenth (decimate_half where the tenth was not reached)
and for simplify_mesh at the cell size whose face count comes closest (bisection over the cell size), mesh_surface_distance to the input
(accuracy, completeness, Chamfer, Hausdorff; 100000 samples each way) and triangle_quality at the minimum, the 1st percentile and the median.

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
    ap.add_argument("--whole-blocks", type=int, default=3, help="blocks of one call for the decimate_mesh parts")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=100_000, help="surface samples each way of the quality comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_decimate.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import (collapse_edges, decimate_mesh, decimate_round, extract_isosurface, mesh_edges, mesh_surface_distance, remesh,
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

    def percentile(v, f, q):
        lengths = mesh_edges(int(v.shape[0]), f, vertices=v).length
        return float(lengths[torch.isfinite(lengths)].quantile(q)) if lengths.numel() <= 16_000_000 else float(lengths[torch.isfinite(lengths)][::4].quantile(q))

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
                "won_of_in_budget": [round(r["collapsed"] / r["in_budget"], 4) for r in m.stats["per_round"]],
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

    def measure(v, f):
        V, F = int(v.shape[0]), int(f.shape[0])
        short = percentile(v, f, 0.2)
        q = vertex_quadrics(v, f)
        t = timed({"quadrics": lambda: vertex_quadrics(v, f), "decimate_round": lambda: decimate_round(v, f, q, F // 4),
                   "collapse_round": lambda: collapse_edges(v, f, min_edge=short), "edges": lambda: mesh_edges(V, f, vertices=v)},
                  args.blocks, args.iters, args.warmup)
        t["decimate_round"].update(budget=F // 4, stats=decimate_round(v, f, q, F // 4).stats)
        t["collapse_round"].update(min_edge=short, stats=collapse_edges(v, f, min_edge=short).stats)
        t["ratio_collapse"] = round(t["decimate_round"]["ms"] / t["collapse_round"]["ms"], 3)
        t["ratio_edges"] = round(t["decimate_round"]["ms"] / t["edges"]["ms"], 3)
        t.update(timed({"decimate_half": lambda: decimate_mesh(v, f, ratio=0.5), "decimate_tenth": lambda: decimate_mesh(v, f, ratio=0.1)},
                       args.whole_blocks, 1, 1))
        half, tenth = decimate_mesh(v, f, ratio=0.5), decimate_mesh(v, f, ratio=0.1)
        t["decimate_half"].update(whole(half))
        t["decimate_tenth"].update(whole(tenth))
        quality = None
        pick = tenth if tenth.reached else half
        if pick.stats["collapsed"]:
            cell, s = clustered(v, f, int(pick.faces.shape[0]))
            quality = {"input": shape(v, f), "of": "decimate_tenth" if tenth.reached else "decimate_half",
                       "decimated": dict(shape(pick.vertices, pick.faces), vertices=int(pick.vertices.shape[0]), **distance(pick.vertices, pick.faces, v, f)),
                       "clustered": dict(shape(s.vertices, s.faces) or {"faces": 0}, vertices=int(s.vertices.shape[0]), cell=cell,
                                         **(distance(s.vertices, s.faces, v, f) if s.faces.shape[0] else {}))}
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
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every round-sized part after {args.warmup} warm-up calls each, "
                  f"{args.whole_blocks} alternating blocks of one call of the decimate_mesh parts after one warm-up call, device events around each block; "
                  "ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces and the read-backs "
                  "included); stats from calls of their own; budget of the round = a quarter of the faces; max_normal_deg = 30, no max_cost, no "
                  f"max_edge, carried quadrics; quality: {args.samples} surface samples each way against the input, simplify_mesh at the cell "
                  "size (bisection, 24 steps) whose face count comes closest to the decimated mesh's",
        "meshes": meshes,
        "quality": shapes,
        "not_measured": "meshes above 1 M faces; the kernels alone without allocation and read-back; the share of the six sorts, of the ring walks and "
                        "of the merge; a radix select of the budget line in place of the three ranking sorts; keep masks, pins, max_cost and "
                        "max_edge; memoryless quadrics; vertices of high valence; achieved bandwidth per kernel",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
