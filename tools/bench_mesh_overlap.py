"""What the triangle-overlap query costs on an MI355X, beside the closest-point query on the same index.

    python tools/bench_mesh_overlap.py [--faces 100000 1000000 --soup 100000 --blocks 7 --iters 3 --out profiles/mesh_overlap.json]

Meshes:
    remesh_N      diff_recon_hip.remesh of a sphere's level set at the resolution that gives about N faces, for every N of --faces: a clean
                  closed surface, few candidates beyond neighbours
    soup          the triangles of synthetic.scene(--soup, ...) (what train_synthetic.py trains against), welded with weld_mesh(eps = 1e-3
                  of the scene's extent): crossings almost everywhere
    cross         remesh_N of the first N against a copy of itself shifted by half a voxel, MeshBVH.overlap(other)

On each, in alternating blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest block as
the spread:

    overlap       MeshBVH.overlap(): the first call, the second where the list overflowed max(1024, F // 8), and the sort
    counts        the same query with capacity 0 and no list: what intersecting_face_mask and self_intersection_report run
    closest       MeshBVH.closest of the mesh's own face centroids: the same index, the same walk, Q = F -- a capability of the parent
                  commit, timed in the same process for scale
with, from a call of its own each, the stats of the query and the (wave, leaf) visits of `counts` and of `closest`, and
ratio = counts / closest, list_ratio = overlap / closest.

Public wrappers throughout: allocation of outputs and workspaces and the read-back of the stats included; the index is built once,
outside.  No time here is a pass / fail condition.  Writes the JSON and prints it as one line."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_overlap.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_overlap.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import extract_isosurface, remesh, weld_mesh
    from diff_recon_hip.mesh_overlap import STATS_KEYS, _query, overlap
    from diff_recon_hip.mesh_surface import MeshBVH

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

    def measure(a, b=None):
        """The three parts on the index `a` (against `b` in cross mode), then counters from calls of their own."""
        centroids = a.vertices[a.faces.long()].mean(dim=1).contiguous()
        t = timed({"overlap": lambda: overlap(a, b), "counts": lambda: _query(a, b, 0, None), "closest": lambda: (b or a).closest(centroids)})
        visits = torch.zeros(1, device=dev, dtype=torch.int64)
        _, _, st, _, _ = _query(a, b, 0, visits)
        t["counts"].update(leaf_visits=int(visits.item()), stats=dict(zip(STATS_KEYS, st)))
        visits.zero_()
        (b or a).closest(centroids, leaf_visits=visits)
        t["closest"].update(leaf_visits=int(visits.item()), queries=int(centroids.shape[0]))
        res = overlap(a, b)
        t["overlap"].update(pairs=int(res.pairs.shape[0]), calls=2 if res.pairs.shape[0] > max(1024, a.num_faces // 8) else 1)
        t["ratio"] = round(t["counts"]["ms"] / t["closest"]["ms"], 3)
        t["list_ratio"] = round(t["overlap"]["ms"] / t["closest"]["ms"], 3)
        return t

    # a sphere's level set, then remesh at the resolution that gives about N faces: the face count of a level set grows with resolution^2
    g = torch.arange(48, device=dev, dtype=torch.float32) / 47.0
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    base = weld_mesh(*extract_isosurface((((x - 0.49) ** 2 + (y - 0.51) ** 2 + (z - 0.5) ** 2).sqrt() - 0.4).contiguous(), (0.0, 0.0, 0.0), 1.0 / 47.0), eps=0.0)
    probe = remesh((base.vertices, base.faces), 64)
    per_res2 = probe.faces.shape[0] / 64.0 ** 2
    meshes, first = {}, None
    for N in args.faces:
        res = max(16, int(round(math.sqrt(N / per_res2))))
        m = remesh((base.vertices, base.faces), res)
        bvh = MeshBVH(m.vertices, m.faces)
        meshes[f"remesh_{N}"] = {"workload": f"remesh of a sphere at resolution {res}: {int(m.faces.shape[0])} faces, {int(m.vertices.shape[0])} vertices",
                                 "parts": measure(bvh)}
        if first is None:
            first = (bvh, m, float(m.stats["voxel_size"]))
        else:
            del bvh, m
        torch.cuda.empty_cache()

    tri = torch.from_numpy(np.ascontiguousarray(synthetic.scene(args.soup, 256, 192, 2, seed=0, edge_px=10.0)["vertex"])).to(dev)
    sv, sf = tri.reshape(-1, 3).contiguous(), torch.arange(3 * tri.shape[0], device=dev, dtype=torch.int32).reshape(-1, 3)
    extent = float((sv.max(dim=0).values - sv.min(dim=0).values).max())
    w = weld_mesh(sv, sf, eps=1e-3 * extent)
    meshes["soup"] = {"workload": f"synthetic.scene({args.soup}) welded with eps = 1e-3 of its extent: {int(w.faces.shape[0])} faces, "
                                  f"{int(w.vertices.shape[0])} vertices", "parts": measure(MeshBVH(w.vertices, w.faces))}
    if first is not None:
        bvh, m, h = first
        other = MeshBVH(m.vertices + torch.tensor([0.5 * h, 0.0, 0.0], device=dev), m.faces)
        meshes["cross"] = {"workload": f"remesh_{args.faces[0]} against a copy of itself shifted by half a voxel along x", "parts": measure(bvh, other)}

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part after {args.warmup} warm-up calls each, device events "
                  "around each block; ms = median block, min / max block = the spread; public wrappers (allocation of outputs and workspaces and the "
                  "read-back of the stats included; the index is built once, outside); stats, pairs and leaf visits from calls of their own; "
                  "ratio = counts / closest, list_ratio = overlap / closest",
        "meshes": meshes,
        "not_measured": "meshes above 1 M faces; the kernel alone without the clears and the read-back; fp64 pipe utilisation; other shifts of the cross check",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
