"""Times diff_recon_hip.mesh_orient (csrc/mesh_orient.hip) on the meshes a fusion produces, a first measurement:

    python tools/bench_mesh_orient.py [--grid 256 --large 512 --cell 2 --blocks 10 --iters 20 --warmup 3 --out profiles/mesh_orient.json]

The mesh is tools/bench_mesh_manifold.py's: the welded level set of tools/bench_volume.py's sphere volume after simplify_mesh in cells of
--cell voxels and split_nonmanifold, so that every shared edge links; half of its faces are then reversed by a seeded mask, so that there is
something to orient.  --large N repeats everything at N^3.  The parts:

    orient_anchor, orient_majority, orient_volume   orient_faces in each mode: the records, the two sorts and the two gathers, the links, the
                                                    flatten, for volume the maximum and the term pass, the decision, the recount; reads its
                                                    ten counts back
    vertex_fans        vertex_fans on the same mesh: the same two sorts of 3 F records, the yardstick (its code is not this library's)
    adjacency          vertex_adjacency on the same mesh: the same two sorts over twice the records

Timed with device events, in alternating blocks after a warm-up, like tools/bench_mesh_manifold.py; public wrappers, so the allocation of
outputs and workspaces and the wrappers' host reads are included.
Writes, and prints as one JSON line, the median block time of every part and every mode's ratio to vertex_fans.
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
    from diff_recon_hip import mesh_orient as O
    from diff_recon_hip import mesh_simplify as Q
    from diff_recon_hip import mesh_smooth as S
    mesh, origin, h = fused_sphere(G, args.view, dev)
    small = Q.simplify_mesh(mesh.vertices, mesh.faces, args.cell * h, origin)
    del mesh
    torch.cuda.empty_cache()
    split = M.split_nonmanifold(small.vertices, small.faces)
    v, clean = split.vertices, split.faces
    V, F = v.shape[0], clean.shape[0]
    mask = torch.rand((F,), device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed)) < 0.5
    f = torch.where(mask[:, None], clean[:, [0, 2, 1]], clean).contiguous()
    stats = {mode: O.orient_faces(v, f, outward=mode).stats for mode in O.OUTWARD}
    oriented = O.orient_faces(v, f, outward="volume")
    parts = {"orient_" + mode: (lambda m: lambda: O.orient_faces(v, f, outward=m))(mode) for mode in O.OUTWARD}
    parts["vertex_fans"] = lambda: M.vertex_fans(V, f)
    parts["adjacency"] = lambda: S.vertex_adjacency(V, f)

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
    for k in parts:
        res[k]["over_vertex_fans"] = round(res[k]["ms"] / res["vertex_fans"]["ms"], 3)
        res[k]["over_adjacency"] = round(res[k]["ms"] / res["adjacency"]["ms"], 3)
    return {
        "workload": f"the welded level set of a {G}^3 volume over [-1, 1]^3 (one {args.view} x {args.view} analytic depth view of a sphere of radius "
                    f"0.6, carving on) after simplify_mesh in cells of {args.cell:g} voxels and split_nonmanifold: {V} vertices, {F} faces; "
                    f"{int(mask.sum())} faces reversed by a mask seeded with {args.seed}",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspaces and the wrappers' host reads included)",
        "vertices": V, "faces": F, "cell_voxels": args.cell, "parts": res, "orient_stats": stats,
        "same_direction_edges_after": M.vertex_fans(V, oriented.faces).stats["same_direction_edges"],
        "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume the mesh is extracted from")
    ap.add_argument("--large", type=int, default=0, help="measure the mesh of a second volume of this many samples a side (0: none)")
    ap.add_argument("--view", type=int, default=800, help="the fused depth image is --view x --view pixels")
    ap.add_argument("--cell", type=float, default=2.0, help="simplify_mesh clusters in cells of this many voxels before anything is timed")
    ap.add_argument("--seed", type=int, default=1, help="the seed of the mask that reverses half of the faces")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_orient.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_orient.py needs a HIP device (the face-orientation kernels have no CPU fallback)")
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
