"""What the edge table and the edge split cost on an MI355X, beside the one-ring adjacency of the same mesh.

    python tools/bench_mesh_subdivide.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_subdivide.json]

Meshes:
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces: a clean
                  closed surface of nearly uniform edges
    soup          the triangles of synthetic.scene(--soup, ...) (what train_synthetic.py trains against), welded with weld_mesh(eps = 1e-3
                  of the scene's extent): boundary and non-manifold edges, edges of very different lengths

On each, in alternating blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest block as
the spread:

    edges         mesh_edges with lengths: two sorts of the 3 F half-edge records, one scan, the per-edge pass, one host read
    split_all     one split_edges round over all edges: the same front, the scan of the marks, the scatter, the scan of the piece counts,
                  the emission of 4 F faces, one host read and the joins of the wrapper
    split_long    split_long_edges to half the median edge length: its rounds (reported) with the last one that marks nothing
    adjacency     vertex_adjacency of the same mesh: two sorts over the 6 F directed records -- a capability of the parent commit, timed in
                  the same process for scale
with ratio_edges = edges / adjacency and ratio_split = split_all / adjacency.

Public wrappers throughout: allocation of outputs and workspaces and the read-backs included.  No time here is a pass / fail condition.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_subdivide.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_subdivide.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import extract_isosurface, mesh_edges, remesh, split_edges, split_long_edges, vertex_adjacency, weld_mesh

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
        table = mesh_edges(V, f, vertices=v)
        finite = table.length[torch.isfinite(table.length)]
        half = 0.5 * float(finite.median())
        t = timed({"edges": lambda: mesh_edges(V, f, vertices=v), "split_all": lambda: split_edges(v, f),
                   "split_long": lambda: split_long_edges(v, f, max_edge=half), "adjacency": lambda: vertex_adjacency(V, f)})
        t["edges"].update(stats=table.stats, median_edge=2.0 * half, longest_edge=float(finite.max()))
        one = split_edges(v, f)
        t["split_all"].update(stats={k: one.stats[k] for k in ("edges", "marked", "out_faces", "faces_split")})
        many = split_long_edges(v, f, max_edge=half)
        t["split_long"].update(max_edge=half, rounds=many.stats["rounds"], calls=many.stats["rounds"] + int(many.stats["converged"]),
                               converged=many.stats["converged"], faces=int(many.faces.shape[0]), vertices=int(many.vertices.shape[0]))
        t["adjacency"].update(stats=vertex_adjacency(V, f).stats)
        t["ratio_edges"] = round(t["edges"]["ms"] / t["adjacency"]["ms"], 3)
        t["ratio_split"] = round(t["split_all"]["ms"] / t["adjacency"]["ms"], 3)
        return t

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

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part after {args.warmup} warm-up calls each, device events "
                  "around each block; ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces, the "
                  "read-backs and the joins of the wrappers included); stats from calls of their own; ratio_edges = edges / adjacency, "
                  "ratio_split = split_all / adjacency",
        "meshes": meshes,
        "not_measured": "meshes above 1 M faces; the kernels alone without allocation, read-back and the wrapper's joins; the share of the two sorts; "
                        "the per-vertex limit mode; attributes; achieved bandwidth per kernel",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
