"""What a round of edge flips and a whole delaunay_flips cost on an MI355X, beside the edge table and the edge split of the same mesh, and
what the flips do to the shape of the faces.

    python tools/bench_mesh_flip.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_flip.json]

Meshes (those of tools/bench_mesh_subdivide.py):
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces
    soup          the triangles of synthetic.scene(--soup, ...), welded with weld_mesh(eps = 1e-3 of the scene's extent)

On each, in alternating blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest block as
the spread:

    flip_round    one flip_edges round: the sort-by-edge front, the per-edge classification, the selection, the two sorts of the winners'
                  new edges, the gather of the faces, one host read
    delaunay      delaunay_flips to convergence (at most 64 rounds): its rounds (reported) with the last one that flips nothing
    edges         mesh_edges with lengths, and
    split_all     one split_edges round over all edges: capabilities of the parent commit on the same front, timed in the same process
with ratio_split = flip_round / split_all and ratio_edges = flip_round / edges.

Quality: diff_recon_hip.triangle_quality (4 sqrt(3) area / sum of squared edges) at the minimum, the 1st percentile and the median, before
and after delaunay_flips, with the rounds and the non-Delaunay edges left guarded, on
    split         split_long_edges of the welded soup to half its median edge length
    cap           a flat grid with a slot of --slot cells cut out and closed again by fill_holes: a centroid fan over a long thin loop

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
    ap.add_argument("--slot", type=int, default=60, help="cells of the slot cut out of the flat grid")
    ap.add_argument("--blocks", type=int, default=7, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=3, help="calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_flip.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_flip.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import (delaunay_flips, extract_isosurface, fill_holes, flip_edges, mesh_edges, remesh, split_edges, split_long_edges,
                                triangle_quality, weld_mesh)

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

    def measure(v, f):
        V = int(v.shape[0])
        t = timed({"flip_round": lambda: flip_edges(v, f), "delaunay": lambda: delaunay_flips(v, f),
                   "edges": lambda: mesh_edges(V, f, vertices=v), "split_all": lambda: split_edges(v, f)})
        t["flip_round"].update(stats=flip_edges(v, f).stats)
        many = delaunay_flips(v, f)
        t["delaunay"].update(rounds=many.stats["rounds"], calls=many.stats["rounds"] + int(many.converged), converged=many.converged,
                             flipped=many.stats["flipped"], guarded=many.stats["guarded"])
        t["ratio_split"] = round(t["flip_round"]["ms"] / t["split_all"]["ms"], 3)
        t["ratio_edges"] = round(t["flip_round"]["ms"] / t["edges"]["ms"], 3)
        return t

    def shape(q):
        q = q[~q.isnan()]
        return {"min": float(q.min()), "p01": float(q.quantile(0.01)), "median": float(q.median())} if q.numel() else None

    def quality(v, f, slots=None):
        out = delaunay_flips(v, f)
        r = {"faces": int(f.shape[0]), "rounds": out.stats["rounds"], "converged": out.converged, "flipped": out.stats["flipped"],
             "guarded": out.stats["guarded"], "slots_rewritten": int(out.face_flipped.sum()),
             "before": shape(triangle_quality(v, f)), "after": shape(triangle_quality(v, out.faces))}
        if slots is not None:  # the slots of interest, and those a flip touched beside them
            where = slots | out.face_flipped
            r["slots"] = {"faces": int(where.sum()), "before": shape(triangle_quality(v, f)[where]), "after": shape(triangle_quality(v, out.faces)[where])}
        return r

    # a sphere's level set, then remesh at the resolution that gives about N faces: the face count of a level set grows with resolution^2
    g = torch.arange(48, device=dev, dtype=torch.float32) / 47.0
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    base = weld_mesh(*extract_isosurface((((x - 0.49) ** 2 + (y - 0.51) ** 2 + (z - 0.5) ** 2).sqrt() - 0.4).contiguous(), (0.0, 0.0, 0.0), 1.0 / 47.0), eps=0.0)
    probe = remesh((base.vertices, base.faces), 64)
    per_res2 = probe.faces.shape[0] / 64.0 ** 2
    meshes = {}
    for N in args.faces:
        res = max(16, int(round(math.sqrt(N / per_res2))))
        m = remesh((base.vertices, base.faces), res)
        meshes[f"remesh_{N}"] = {"workload": f"remesh of a sphere at resolution {res}: {int(m.faces.shape[0])} faces, {int(m.vertices.shape[0])} vertices",
                                 "parts": measure(m.vertices, m.faces)}
        del m
        torch.cuda.empty_cache()

    tri = torch.from_numpy(np.ascontiguousarray(synthetic.scene(args.soup, 256, 192, 2, seed=0, edge_px=10.0)["vertex"])).to(dev)
    sv, sf = tri.reshape(-1, 3).contiguous(), torch.arange(3 * tri.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    extent = float((sv.max(dim=0).values - sv.min(dim=0).values).max())
    w = weld_mesh(sv, sf, eps=1e-3 * extent)
    meshes["soup"] = {"workload": f"synthetic.scene({args.soup}) welded with eps = 1e-3 of its extent: {int(w.faces.shape[0])} faces, "
                                  f"{int(w.vertices.shape[0])} vertices", "parts": measure(w.vertices, w.faces)}

    lengths = mesh_edges(int(w.vertices.shape[0]), w.faces, vertices=w.vertices).length
    half = 0.5 * float(lengths[torch.isfinite(lengths)].median())
    fine = split_long_edges(w.vertices, w.faces, max_edge=half)
    shapes = {"split": dict(quality(fine.vertices, fine.faces), workload=f"split_long_edges of the welded soup to {half:.4g}, half its median edge")}

    n, slot = args.slot + 20, args.slot  # an (n x 21)-cell flat grid without the cells of row 10 from column 10 on for `slot` cells
    jj, ii = torch.meshgrid(torch.arange(n + 1), torch.arange(22), indexing="xy")
    gv = torch.stack([jj.reshape(-1), ii.reshape(-1), torch.zeros(22 * (n + 1), dtype=torch.int64)], 1).to(dev, torch.float32)
    a = (torch.arange(21)[:, None] * (n + 1) + torch.arange(n)[None, :])
    hole = torch.zeros((21, n), dtype=torch.bool)
    hole[10, 10:10 + slot] = True
    a = a[~hole]
    gf = torch.cat([torch.stack([a, a + 1, a + n + 2], 1), torch.stack([a, a + n + 2, a + n + 1], 1)]).to(dev, torch.int32)
    filled = fill_holes(gv, gf, max_loop_edges=2 * slot + 2)
    shapes["cap"] = dict(quality(filled.vertices, filled.faces, filled.face_loop >= 0),
                         workload=f"a flat {n} x 21 grid with a slot of {slot} x 1 cells closed by fill_holes: a fan of {int((filled.face_loop >= 0).sum())} faces")

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part after {args.warmup} warm-up calls each, device events "
                  "around each block; ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces and the "
                  "read-backs included); stats from calls of their own; ratio_split = flip_round / split_all, ratio_edges = flip_round / edges",
        "meshes": meshes,
        "quality": shapes,
        "not_measured": "meshes above 1 M faces; the kernels alone without allocation and read-back; the share of the sorts and of the binary "
                        "search; keep masks; achieved bandwidth per kernel",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
