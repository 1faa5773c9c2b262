"""Times the vertex weld (diff_recon_hip.mesh_weld over csrc/mesh_weld.hip) part by part on the soup of a synthetic scene, next to
simple_knn.nearestNeighbor on the same points -- the search that shares the weld's front half (Morton codes, radix sort, gathered points,
1024-point boxes; csrc/ts_knn_front.h) and so the honest yardstick for the label pass:

    python tools/bench_mesh_weld.py [--triangles 1000000 --targets 1.02 3 6 --blocks 10 --iters 10 --warmup 5 --out profiles/mesh_weld.json]

Scene: synthetic.scene(mode="frustum") with P triangles, V = 3 P un-shared vertices, F = P front faces.  For every target the tool first finds,
by doubling and bisection on the device, an eps whose mean cluster size V / V' is about the target (random triangles share no vertices, so the
clusters come from chance proximity; near 6 single linkage is close to percolating), then times with device events, in alternating blocks
after a warm-up, each through its public wrapper (workspace allocation from torch's caching allocator included):

    labels        weld_labels                      the radius search and the union-find
    compact       compact_labels, both positions   numbering and welded positions (includes the read-back of V')
    remap         remap_faces                      face remap and keep mask
    census        edge_census                      two 3 F-element radix sorts and the run-length pass, on the remapped faces under the keep mask
    nearest       simple_knn.nearestNeighbor(points, 3)

and reads the search's (workgroup, box) visits from the library's counter in a run of its own.  Writes, and prints as one JSON line, the
median block time of every part with the slowest and fastest block.  Needs a HIP device; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--targets", type=float, nargs="+", default=[1.02, 3.0, 6.0], help="mean cluster sizes V / V' to find an eps for")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=10, help="calls per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_weld.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_weld.py needs a HIP device (the weld has no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import synthetic
    from diff_recon_hip import mesh_weld
    from simple_knn import nearestNeighbor

    P = args.triangles
    s = synthetic.scene(P, 1920, 1080, 0, seed=42, mode="frustum", with_grads=False)
    vertices = torch.from_numpy(np.ascontiguousarray(s["vertex"].reshape(-1, 3))).to(dev)
    V = vertices.shape[0]
    faces = torch.arange(V, device=dev, dtype=torch.int32).reshape(P, 3)
    own = torch.arange(V, device=dev, dtype=torch.int32)
    extent = (vertices.max(0).values - vertices.min(0).values).tolist()

    def mean_cluster(eps):
        label = mesh_weld.weld_labels(vertices, eps)
        return V / int((label == own).sum().item())

    def find_eps(target):
        """An eps with mean cluster size within 3 % of the target: doubling from far below the mean spacing, then bisection."""
        lo = 0.0
        hi = 0.02 * (extent[0] * extent[1] * extent[2] / V) ** (1.0 / 3.0)
        while mean_cluster(hi) < target:
            lo, hi = hi, 2.0 * hi
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            m = mean_cluster(mid)
            if abs(m - target) <= 0.03 * target:
                return mid
            lo, hi = (mid, hi) if m < target else (lo, mid)
        return 0.5 * (lo + hi)

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

    def measure(target):
        eps = find_eps(target)
        print(f"target {target:g}: eps {eps:.6g}", file=sys.stderr, flush=True)
        label = mesh_weld.weld_labels(vertices, eps)
        remap, welded, n = mesh_weld.compact_labels(label, vertices, "first")
        new_faces, keep = mesh_weld.remap_faces(V, faces, remap)
        parts = {
            "labels": lambda: mesh_weld.weld_labels(vertices, eps),
            "compact_first": lambda: mesh_weld.compact_labels(label, vertices, "first"),
            "compact_mean": lambda: mesh_weld.compact_labels(label, vertices, "mean"),
            "remap": lambda: mesh_weld.remap_faces(V, faces, remap),
            "census": lambda: mesh_weld.edge_census(V, new_faces, keep),
            "nearest": lambda: nearestNeighbor(vertices, 3),
        }
        for _ in range(args.warmup):
            for fn in parts.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in parts}
        for _ in range(args.blocks):
            for k, fn in parts.items():
                times[k].append(block(fn, args.iters))
        print(f"target {target:g}: " + ", ".join(f"{k} {statistics.median(v):.3f} ms" for k, v in times.items()), file=sys.stderr, flush=True)
        visits = torch.zeros(1, device=dev, dtype=torch.int64)
        mesh_weld.weld_labels(vertices, eps, visits)
        torch.cuda.synchronize()
        nboxes = (V + 1023) // 1024
        counts = mesh_weld.edge_census(V, new_faces, keep).tolist()
        sizes = torch.bincount(remap.to(torch.int64), minlength=n)
        out = {k: summary(v) for k, v in times.items()}
        out.update({
            "target_mean_cluster": target, "eps": eps, "vertices_out": n, "mean_cluster": round(V / n, 4), "largest_cluster": int(sizes.max().item()),
            "vertices_in_clusters_of_2_or_more": int(sizes[sizes > 1].sum().item()), "faces_kept": int(keep.sum().item()),
            "edges_boundary_manifold_nonmanifold": counts, "box_visits": int(visits.item()), "boxes": nboxes,
            "box_visits_per_workgroup": round(int(visits.item()) / nboxes, 2),
            "pair_tests_upper_bound": int(visits.item()) * 1024 * 1024,
            "labels_over_nearest": round(out["labels"]["ms"] / out["nearest"]["ms"], 3),
        })
        return out

    result = {
        "workload": f"synthetic.scene(P={P}, 1920x1080, mode=frustum, seed 42): V = {V} un-shared vertices, F = {P} front faces; extent "
                    f"{extent[0]:.0f} x {extent[1]:.0f} x {extent[2]:.0f}",
        "method": f"per eps: {args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around "
                  "each block; public wrappers (allocation of outputs and workspace included; compact also reads V' back); box visits from the library's "
                  "counter in a call of its own",
        "runs": [measure(t) for t in args.targets],
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
