"""Times the parts of diff_recon_hip.mesh_manifold (csrc/mesh_manifold.hip) on the meshes a fusion produces, a first measurement:

    python tools/bench_mesh_manifold.py [--grid 256 --large 512 --cell 2 --blocks 10 --iters 20 --warmup 3 --out profiles/mesh_manifold.json]

The mesh is the welded level set of tools/bench_volume.py's sphere volume (tools/bench_mesh_simplify.py's: one analytic depth view fused with
carving into a --grid^3 volume, extracted, welded with eps = 0) after simplify_mesh in cells of --cell voxels on the volume's grid, so that
there is something to split: pinched cells leave edges that three faces use and vertices where two sheets touch; --large N repeats
everything at N^3.  The parts:

    vertex_fans        vertex_fans: the records, the two sorts and the two gathers, the links, the flatten, the vertex pass; reads its six
                       counts back
    split_nonmanifold  split_nonmanifold(fans=...): labels and keepers, the prefix sum, sources, faces, and the gathers and concatenations
                       behind the input's vertices; reads its totals back
    adjacency          vertex_adjacency on the same mesh: the same two sorts over twice the records, in the same blocks
    weld               weld_mesh(eps=0) on the same mesh: the neighbouring operator, in the same blocks
    copy_<part>        dst.copy_(src) of half of the part's model bytes (so that read + written = the model bytes): the streaming yardstick of
                       that part, in the same blocks

Timed with device events, in alternating blocks after a warm-up, like tools/bench_mesh_holes.py; public wrappers, so the allocation of
outputs and workspaces and the wrappers' host reads are included.  model_bytes is the least each part must move (inputs read once, outputs
written once), not a counter reading: the sort passes are what lies between vertex_fans and its copy.
Writes, and prints as one JSON line, the median block time of every part.
Needs a HIP device; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")]
import torch


def measure(G, args, dev):
    from bench_mesh_simplify import fused_sphere
    from diff_recon_hip import mesh_manifold as M
    from diff_recon_hip import mesh_simplify as Q
    from diff_recon_hip import mesh_smooth as S
    from diff_recon_hip.mesh_weld import mesh_topology, weld_mesh
    mesh, origin, h = fused_sphere(G, args.view, dev)
    fused = (mesh.vertices.shape[0], mesh.faces.shape[0])
    small = Q.simplify_mesh(mesh.vertices, mesh.faces, args.cell * h, origin)
    del mesh
    torch.cuda.empty_cache()
    v, f = small.vertices, small.faces
    V, F = v.shape[0], f.shape[0]
    fans = M.vertex_fans(V, f)
    out = M.split_nonmanifold(v, f, fans=fans)
    new = fans.stats["new_vertices"]
    before, after = mesh_topology(V, f), mesh_topology(out.vertices.shape[0], out.faces)
    nbytes = 12 * V + 12 * F
    model = {  # bytes each part has to move at the least
        "vertex_fans": 12 * F + 12 * F + 4 * V,                               # faces in; corner_fan and vertex_fans out
        "split_nonmanifold": 12 * F + 12 * F + 12 * F + 8 * new + 2 * 12 * V,  # faces and corner_fan in; faces and the two lists out; the vertices copied
        "adjacency": 12 * F + 4 * (V + 1) + 2 * 4 * 6 * F + V,
    }
    model["weld"] = 2 * nbytes  # the mesh in, the mesh out
    calls = {
        "vertex_fans": lambda: M.vertex_fans(V, f),
        "split_nonmanifold": lambda: M.split_nonmanifold(v, f, fans=fans),
        "adjacency": lambda: S.vertex_adjacency(V, f),
    }
    parts = {}
    for name, fn in calls.items():
        half = model[name] // 2
        src, dst = torch.empty((half,), device=dev, dtype=torch.uint8).fill_(1), torch.empty((half,), device=dev, dtype=torch.uint8)
        parts[name] = fn
        parts["copy_" + name] = (lambda s, d: lambda: d.copy_(s))(src, dst)
        model["copy_" + name] = 2 * half
    parts["weld"] = lambda: weld_mesh(v, f, eps=0.0)

    def block(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    for _ in range(args.warmup):
        for fn in parts.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in parts}
    for _ in range(args.blocks):
        for k, fn in parts.items():
            times[k].append(block(fn, args.iters))
    res = {k: {"ms": round(statistics.median(t), 4), "min_block_ms": round(min(t), 4), "max_block_ms": round(max(t), 4)} for k, t in times.items()}
    print(f"{G}^3: " + ", ".join(f"{k} {t['ms']:.3f} ms" for k, t in res.items()), file=sys.stderr, flush=True)
    for k, t in res.items():
        t["model_bytes"] = model[k]
        t["model_GB_per_s"] = round(model[k] / (t["ms"] * 1e-3) / 1e9, 1)
    for k in calls:
        res[k]["over_copy"] = round(res[k]["ms"] / res["copy_" + k]["ms"], 2)
        res[k]["over_adjacency"] = round(res[k]["ms"] / res["adjacency"]["ms"], 3)
        res[k]["over_weld"] = round(res[k]["ms"] / res["weld"]["ms"], 3)
    return {
        "workload": f"the welded level set of a {G}^3 volume over [-1, 1]^3 (one {args.view} x {args.view} analytic depth view of a sphere of radius "
                    f"0.6, carving on; {fused[0]} vertices, {fused[1]} faces) after simplify_mesh in cells of {args.cell:g} voxels: {V} vertices, "
                    f"{F} faces, {nbytes} bytes",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspaces and the wrappers' host reads included); model_bytes is the least "
                  "each part must move, not a counter reading; copy_<part> copies half of them, so that it reads and writes as many",
        "vertices": V, "faces": F, "voxel": h, "cell_voxels": args.cell, "parts": res, "simplify_stats": small.stats, "fan_stats": fans.stats,
        "split_stats": out.stats, "topology_before": before, "topology_after": after, "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume the mesh is extracted from")
    ap.add_argument("--large", type=int, default=0, help="measure the mesh of a second volume of this many samples a side (0: none)")
    ap.add_argument("--view", type=int, default=800, help="the fused depth image is --view x --view pixels")
    ap.add_argument("--cell", type=float, default=2.0, help="simplify_mesh clusters in cells of this many voxels before anything is timed")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_manifold.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_manifold.py needs a HIP device (the vertex-fan kernels have no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    result = measure(args.grid, args, dev)
    if args.large:
        torch.cuda.empty_cache()
        result["large"] = measure(args.large, args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
