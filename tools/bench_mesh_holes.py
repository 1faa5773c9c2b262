"""Times the parts of diff_recon_hip.mesh_holes (csrc/mesh_holes.hip) on the meshes a fusion produces, a first measurement:

    python tools/bench_mesh_holes.py [--grid 256 --large 512 --blocks 10 --iters 20 --warmup 3 --out profiles/mesh_holes.json]

The mesh is the welded level set of tools/bench_volume.py's sphere volume (tools/bench_mesh_simplify.py's: one analytic depth view fused with
carving into a --grid^3 volume, extracted, welded with eps = 0): an open surface whose boundary is one long outer loop plus whatever small
ones; --large N repeats everything at N^3.  The parts:

    boundary_loops  boundary_loops(adjacency=...): the search per half-edge, the census, the two doubling passes, the ranking, the scatter; reads
                    its four counts back
    fill_holes      fill_holes(max_loop_edges=64, loops=...): status, numbering, sums and faces, and the concatenation behind the input's
                    vertices and faces; reads its three totals and the status histogram back
    adjacency       vertex_adjacency on the same mesh: what boundary_loops needs first, in the same blocks
    weld            weld_mesh(eps=0) on the same mesh: the neighbouring operator, in the same blocks
    copy_<part>     dst.copy_(src) of half of the part's model bytes (so that read + written = the model bytes): the streaming yardstick of
                    that part, in the same blocks

Timed with device events, in alternating blocks after a warm-up, like tools/bench_mesh_smooth.py; public wrappers, so the allocation of
outputs and workspaces and the wrappers' host reads are included.  model_bytes is the least each part must move (inputs read once, outputs
written once), not a counter reading: the doubling rounds over all 3 F half-edges are what lies between boundary_loops and its copy.
Writes, and prints as one JSON line, the median block time of every part.
Needs a HIP device; there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")]
import torch


def measure(G, args, dev):
    from bench_mesh_simplify import fused_sphere
    from diff_recon_hip import mesh_holes as H
    from diff_recon_hip import mesh_smooth as S
    from diff_recon_hip.mesh_weld import weld_mesh
    mesh, _, h = fused_sphere(G, args.view, dev)
    torch.cuda.empty_cache()
    v, f = mesh.vertices, mesh.faces
    V, F = v.shape[0], f.shape[0]
    adj = S.vertex_adjacency(V, f)
    E = adj.stats["entries"]
    loops = H.boundary_loops(V, f, adjacency=adj)
    L, M = loops.stats["loops"], loops.stats["loop_half_edges"]
    filled = H.fill_holes(v, f, args.max_loop_edges, loops=loops)
    nbytes = 12 * V + 12 * F
    model = {  # bytes each part has to move at the least
        "boundary_loops": 12 * F + 4 * (V + 1) + 8 * E + 12 * F + 4 * (F + 1) + 12 * F,  # faces and table in; the three outputs to their capacity
        "fill_holes": 4 * (L + 1) + 4 * M + L + 12 * L + 16 * M + 2 * nbytes,  # the loops in; status, vertices, faces, face loops out; the mesh copied
        "adjacency": 12 * F + 4 * (V + 1) + 2 * 4 * 6 * F + V,
    }
    model["weld"] = 2 * nbytes  # the mesh in, the mesh out
    calls = {
        "boundary_loops": lambda: H.boundary_loops(V, f, adjacency=adj),
        "fill_holes": lambda: H.fill_holes(v, f, args.max_loop_edges, loops=loops),
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
    out = {k: {"ms": round(statistics.median(t), 4), "min_block_ms": round(min(t), 4), "max_block_ms": round(max(t), 4)} for k, t in times.items()}
    print(f"{G}^3: " + ", ".join(f"{k} {t['ms']:.3f} ms" for k, t in out.items()), file=sys.stderr, flush=True)
    for k, t in out.items():
        t["model_bytes"] = model[k]
        t["model_GB_per_s"] = round(model[k] / (t["ms"] * 1e-3) / 1e9, 1)
    for k in calls:
        out[k]["over_copy"] = round(out[k]["ms"] / out["copy_" + k]["ms"], 2)
        out[k]["over_weld"] = round(out[k]["ms"] / out["weld"]["ms"], 3)
    rounds = max(1, math.ceil(math.log2(max(min(3 * F, V + 1), 2))))
    return {
        "workload": f"the welded level set of a {G}^3 volume over [-1, 1]^3 (one {args.view} x {args.view} analytic depth view of a sphere of radius "
                    f"0.6, carving on): {V} vertices, {F} faces, {E} adjacency entries of which {adj.stats['boundary']} boundary, {nbytes} bytes",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspaces and the wrappers' host reads included); model_bytes is the least "
                  "each part must move, not a counter reading; copy_<part> copies half of them, so that it reads and writes as many",
        "vertices": V, "faces": F, "entries": E, "voxel": h, "max_loop_edges": args.max_loop_edges, "doubling_rounds_per_pass": rounds, "parts": out,
        "adjacency_stats": adj.stats, "loop_stats": loops.stats, "fill_stats": filled.stats, "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume the mesh is extracted from")
    ap.add_argument("--large", type=int, default=0, help="measure the mesh of a second volume of this many samples a side (0: none)")
    ap.add_argument("--view", type=int, default=800, help="the fused depth image is --view x --view pixels")
    ap.add_argument("--max-loop-edges", type=int, default=64, help="fill_holes closes the loops of at most this many edges")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_holes.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_holes.py needs a HIP device (the hole-filling kernels have no CPU fallback)")
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
