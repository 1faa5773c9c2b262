"""What a round of edge collapses and a whole collapse_short_edges cost on an MI355X, beside the edge table and a round of edge flips of the
same mesh, and what the collapses do to the shape of the faces.

    python tools/bench_mesh_collapse.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_collapse.json]

Meshes (those of tools/bench_mesh_flip.py):
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces
    soup          the triangles of synthetic.scene(--soup, ...), welded with weld_mesh(eps = 1e-3 of the scene's extent)

On each, with min_edge = the 20th percentile of the mesh's finite edge lengths, in alternating blocks of back-to-back calls between device
events, median over the blocks with the fastest and slowest block as the spread:

    collapse_round  one collapse_edges round: the sort-by-edge front, the sort of the corners, vertex classes, the classification with its
                    ring walks, the two selection gathers, the winners, the gather of the faces, one host read
    collapse_all    collapse_short_edges to convergence (at most 64 rounds) with its compaction: its rounds (reported) with the last one
                    that collapses nothing
    edges           mesh_edges with lengths, and
    flip_round      one flip_edges round: capabilities of the parent commit on the same front, timed in the same process
with ratio_flip = collapse_round / flip_round and ratio_edges = collapse_round / edges.

Quality: diff_recon_hip.triangle_quality (4 sqrt(3) area / sum of squared edges) at the minimum, the 1st percentile and the median, and the
needles (quality below 0.1), before and after, on
    split         split_long_edges of the welded soup to half its median edge length (input (a) of DESIGN 16u): delaunay_flips alone, then
                  collapse_short_edges at a quarter of that median with delaunay_flips behind it
    remesh_N      the first remeshed sphere: collapse_short_edges at the 20th percentile, delaunay_flips behind it, and isotropic_remesh at
                  the median edge length

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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_collapse.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_collapse.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import (collapse_edges, collapse_short_edges, delaunay_flips, extract_isosurface, flip_edges, isotropic_remesh, mesh_edges,
                                remesh, split_long_edges, triangle_quality, weld_mesh)

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

    def timed(parts):
        for _ in range(args.warmup):
            for fn in parts.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in parts}
        for _ in range(args.blocks):
            for k, fn in parts.items():
                times[k].append(block(fn, args.iters))
        out = {k: summary(v) for k, v in times.items()}
        print(", ".join(f"{k} {v['ms']:.3f} ms" for k, v in out.items()), file=sys.stderr, flush=True)
        return out

    def percentile(v, f, q):
        lengths = mesh_edges(int(v.shape[0]), f, vertices=v).length
        return float(lengths[torch.isfinite(lengths)].quantile(q)) if lengths.numel() <= 16_000_000 else float(lengths[torch.isfinite(lengths)][::4].quantile(q))

    def measure(v, f):
        V = int(v.shape[0])
        short = percentile(v, f, 0.2)
        t = timed({"collapse_round": lambda: collapse_edges(v, f, min_edge=short), "collapse_all": lambda: collapse_short_edges(v, f, min_edge=short),
                   "edges": lambda: mesh_edges(V, f, vertices=v), "flip_round": lambda: flip_edges(v, f)})
        t["min_edge"] = short
        t["collapse_round"].update(stats=collapse_edges(v, f, min_edge=short).stats)
        many = collapse_short_edges(v, f, min_edge=short)
        t["collapse_all"].update(rounds=many.stats["rounds"], calls=many.stats["rounds"] + int(many.converged), converged=many.converged,
                                 collapsed=many.stats["collapsed"], guarded=many.stats["guarded"], vertices=many.stats["num_vertices"],
                                 faces=many.stats["num_faces"], per_round=[r["collapsed"] for r in many.stats["per_round"]])
        t["ratio_flip"] = round(t["collapse_round"]["ms"] / t["flip_round"]["ms"], 3)
        t["ratio_edges"] = round(t["collapse_round"]["ms"] / t["edges"]["ms"], 3)
        return t

    def shape(v, f):
        q = triangle_quality(v, f)
        q = q[~q.isnan()]
        if not q.numel():
            return None
        return {"faces": int(f.shape[0]), "min": float(q.min()), "p01": float(q.quantile(0.01)) if q.numel() <= 16_000_000 else None,
                "median": float(q.median()), "needles": int((q < 0.1).sum())}

    def quality(v, f, min_edge):
        flips_alone = delaunay_flips(v, f)
        c = collapse_short_edges(v, f, min_edge=min_edge)
        d = delaunay_flips(c.vertices, c.faces)
        return {"min_edge": min_edge, "before": shape(v, f), "flips_alone": shape(v, flips_alone.faces),
                "collapsed": dict(shape(c.vertices, c.faces), rounds=c.stats["rounds"], converged=c.converged, collapses=c.stats["collapsed"],
                                  guarded=c.stats["guarded"], guarded_by={k[8:]: n for k, n in c.stats.items() if k.startswith("guarded_")}),
                "collapsed_then_flipped": dict(shape(c.vertices, d.faces), rounds=d.stats["rounds"], flipped=d.stats["flipped"])}

    # a sphere's level set, then remesh at the resolution that gives about N faces: the face count of a level set grows with resolution^2
    g = torch.arange(48, device=dev, dtype=torch.float32) / 47.0
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    base = weld_mesh(*extract_isosurface((((x - 0.49) ** 2 + (y - 0.51) ** 2 + (z - 0.5) ** 2).sqrt() - 0.4).contiguous(), (0.0, 0.0, 0.0), 1.0 / 47.0), eps=0.0)
    probe = remesh((base.vertices, base.faces), 64)
    per_res2 = probe.faces.shape[0] / 64.0 ** 2
    meshes, shapes = {}, {}
    for N in args.faces:
        res = max(16, int(round(math.sqrt(N / per_res2))))
        m = remesh((base.vertices, base.faces), res)
        meshes[f"remesh_{N}"] = {"workload": f"remesh of a sphere at resolution {res}: {int(m.faces.shape[0])} faces, {int(m.vertices.shape[0])} vertices",
                                 "parts": measure(m.vertices, m.faces)}
        if not shapes:
            shapes[f"remesh_{N}"] = dict(quality(m.vertices, m.faces, percentile(m.vertices, m.faces, 0.2)), workload=meshes[f"remesh_{N}"]["workload"])
            target = percentile(m.vertices, m.faces, 0.5)
            r = isotropic_remesh(m.vertices, m.faces, target, iterations=3)
            shapes[f"remesh_{N}"]["isotropic_remesh"] = dict(shape(r.vertices, r.faces), target_edge=target, vertices=int(r.vertices.shape[0]),
                                                             edge_length_before=r.stats["before"]["edge_length"], edge_length_after=r.stats["after"]["edge_length"],
                                                             iterations=r.stats["iterations"], closing=r.stats["closing"])
        del m
        torch.cuda.empty_cache()

    tri = torch.from_numpy(np.ascontiguousarray(synthetic.scene(args.soup, 256, 192, 2, seed=0, edge_px=10.0)["vertex"])).to(dev)
    sv, sf = tri.reshape(-1, 3).contiguous(), torch.arange(3 * tri.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    extent = float((sv.max(dim=0).values - sv.min(dim=0).values).max())
    w = weld_mesh(sv, sf, eps=1e-3 * extent)
    meshes["soup"] = {"workload": f"synthetic.scene({args.soup}) welded with eps = 1e-3 of its extent: {int(w.faces.shape[0])} faces, "
                                  f"{int(w.vertices.shape[0])} vertices", "parts": measure(w.vertices, w.faces)}

    median = percentile(w.vertices, w.faces, 0.5)
    fine = split_long_edges(w.vertices, w.faces, max_edge=0.5 * median)
    shapes["split"] = dict(quality(fine.vertices, fine.faces, 0.25 * median),
                           workload=f"split_long_edges of the welded soup to {0.5 * median:.4g}, half its median edge; collapse below {0.25 * median:.4g}")

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part after {args.warmup} warm-up calls each, device events "
                  "around each block; ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces and the "
                  "read-backs included); stats from calls of their own; min_edge = the 20th percentile of the finite edge lengths; ratio_flip = "
                  "collapse_round / flip_round, ratio_edges = collapse_round / edges",
        "meshes": meshes,
        "quality": shapes,
        "not_measured": "meshes above 1 M faces; the kernels alone without allocation and read-back; the share of the three sorts, of the ring walks "
                        "and of the binary searches; keep masks, pins and the vertex-limit mode; vertices of high valence; achieved bandwidth per kernel",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
