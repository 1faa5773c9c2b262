"""Times the steps of diff_recon_hip.simplify_mesh (csrc/mesh_simplify.hip) on the meshes a fusion produces, a first measurement:

    python tools/bench_mesh_simplify.py [--grid 256 --large 512 --cells 2 4 --blocks 10 --iters 20 --warmup 3 --out profiles/mesh_simplify.json]

The mesh is the welded level set of tools/bench_volume.py's sphere volume (one analytic depth view fused with carving into a --grid^3
volume, extracted, welded with eps = 0); --large N repeats everything at N^3.  For every cell size of --cells (in voxels):

    labels       cluster_labels: cell keys, two stable 32-bit sorts of (word, index), the run heads
    compact      compact_labels(label, vertices, "first"): the numbering; reads V' back
    place        place_clusters: member sort, face incidence sort over 3 F slots, one thread per cluster (quadric placement)
    remap        remap_faces
    unique       unique_faces: three stable sorts over F, the neighbour compare and the reversed-triple lookup
    copy         dst.copy_(src) of the mesh's bytes (12 V + 12 F): the streaming yardstick, in the same blocks
    weld         weld_mesh(eps=0) on the same mesh: the neighbouring operator, in the same blocks

Timed with device events, in alternating blocks after a warm-up, like tools/bench_volume.py; public wrappers, so the allocation of outputs
and workspaces is included.  model_bytes is the least each part must move (inputs read once, outputs written once), not a counter reading:
the sorts' passes are what lies between a part and the copy.  Writes, and prints as one JSON line, the median block time of every part.
Needs a HIP device; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")]
import torch


def fused_sphere(G, view, dev):
    """The welded level set of bench_volume's volume: (WeldedMesh, origin, voxel size)."""
    from bench_volume import sphere_view
    from diff_recon_hip import volume as V
    h = 2.0 / (G - 1)  # the cube [-1, 1]^3
    vol = V.TSDFVolume((-1.0, -1.0, -1.0), h, (G, G, G), 4.0 * h, dev)
    cam, depth = sphere_view(view, 0.6, 3.0, 0.45, dev)
    vol.integrate(cam, depth, carve_uncovered=True)
    return vol.extract(), vol.origin, h


def measure(G, args, dev):
    from diff_recon_hip import mesh_simplify as S
    from diff_recon_hip.mesh_weld import compact_labels, remap_faces, weld_mesh
    mesh, origin, h = fused_sphere(G, args.view, dev)
    torch.cuda.empty_cache()
    v, f = mesh.vertices, mesh.faces
    V, F = v.shape[0], f.shape[0]
    nbytes = 12 * V + 12 * F
    src, dst = torch.empty((nbytes,), device=dev, dtype=torch.uint8).fill_(1), torch.empty((nbytes,), device=dev, dtype=torch.uint8)

    def block(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    cells = {}
    for K in args.cells:
        cell = K * h
        label = S.cluster_labels(v, origin, cell)
        remap, _, n = compact_labels(label, v, "first")
        new_faces, keep_remap = remap_faces(V, f, remap)
        s = S.simplify_mesh(v, f, cell, origin)
        parts = {
            "labels": lambda: S.cluster_labels(v, origin, cell),
            "compact": lambda: compact_labels(label, v, "first"),
            "place": lambda: S.place_clusters(v, f, remap, origin, cell),
            "remap": lambda: remap_faces(V, f, remap),
            "unique": lambda: S.unique_faces(n, new_faces, keep_remap),
            "copy": lambda: dst.copy_(src),
            "weld": lambda: weld_mesh(v, f, eps=0.0),
        }
        for _ in range(args.warmup):
            for fn in parts.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in parts}
        for _ in range(args.blocks):
            for k, fn in parts.items():
                times[k].append(block(fn, args.iters))
        out = {k: {"ms": round(statistics.median(t), 4), "min_block_ms": round(min(t), 4), "max_block_ms": round(max(t), 4)} for k, t in times.items()}
        print(f"{G}^3, cell {K} voxels: " + ", ".join(f"{k} {t['ms']:.3f} ms" for k, t in out.items()), file=sys.stderr, flush=True)
        model = {  # bytes each part has to move at the least
            "labels": 12 * V + 4 * V,                        # positions in, labels out
            "compact": 4 * V + 4 * V + 12 * V,               # labels in, remap out, all V rows of the positions written
            "place": 12 * V + 4 * V + 12 * F + 12 * V + 4 * V,  # positions, remap and faces in; V rows of positions and member counts out
            "remap": 4 * V + 12 * F + 12 * F + F,            # remap and faces in, faces and keep out
            "unique": 12 * F + F + F,                        # faces and keep in, keep out
            "copy": 2 * nbytes,
            "weld": 2 * nbytes,                              # the mesh in, the mesh out
        }
        copy_rate = model["copy"] / (out["copy"]["ms"] * 1e-3) / 1e9
        for k, t in out.items():
            t["model_bytes"] = model[k]
            t["model_GB_per_s"] = round(model[k] / (t["ms"] * 1e-3) / 1e9, 1)
            t["of_copy_rate"] = round(t["model_GB_per_s"] / copy_rate, 4)
        chain = sum(out[k]["ms"] for k in ("labels", "compact", "place", "remap", "unique"))
        cells[str(K)] = {"cell_voxels": K, "parts": out, "chain_ms": round(chain, 4), "chain_over_copy": round(chain / out["copy"]["ms"], 1),
                         "chain_over_weld": round(chain / out["weld"]["ms"], 3), "stats": s.stats}
    return {
        "workload": f"the welded level set of a {G}^3 volume over [-1, 1]^3 (one {args.view} x {args.view} analytic depth view of a sphere of radius "
                    f"0.6, carving on): {V} vertices, {F} faces, {nbytes} bytes; grid origin = the volume's",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspaces included; compact reads V' back); model_bytes is the least each "
                  "part must move, not a counter reading",
        "vertices": V, "faces": F, "cells": cells, "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume the mesh is extracted from")
    ap.add_argument("--large", type=int, default=0, help="measure the mesh of a second volume of this many samples a side (0: none)")
    ap.add_argument("--view", type=int, default=800, help="the fused depth image is --view x --view pixels")
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="cell sizes in voxels")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify.py needs a HIP device (the simplification kernels have no CPU fallback)")
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
