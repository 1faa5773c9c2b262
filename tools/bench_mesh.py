"""Times the opaque mesh renderer (diff_recon_hip.MeshRenderer) next to what a user had to use before to look at a mesh: the 3D splat
rasterizer's forward with rich_info=False and SH degree 0 on the same triangles, called the way `bench.py --forward-only --rasterizer 3D`
calls it.  One process, alternating blocks, device events, after a warm-up:

    python tools/bench_mesh.py [--triangles 1000000 --width 1920 --height 1080 --edge-px 6 --blocks 10 --iters 20 --out profiles/mesh_render.json]

Writes (and prints as one JSON line): both times per call (median over the blocks) with their spread (min / max block), the mesh render's
per-kernel times (the library's event hooks, a run of its own: the hooks serialise the launches), and how many (wavefront, face) pairs the
depth test walked against four times the pairs in the tile lists -- what the early stop saved.  Needs a HIP device; there is no fallback."""
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--edge-px", type=float, default=6.0)
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per renderer")
    ap.add_argument("--iters", type=int, default=20, help="calls per block (blocks x iters >= 200 for a quotable figure)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a HIP device (neither renderer has a CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import synthetic
    from diff_recon_hip import MeshRenderer
    from diff_triangle_rasterization_2D import TriangleRasterizationSettings, _C, center2D_sink
    from diff_triangle_rasterization_3D import TriangleRasterizer

    P, W, H = args.triangles, args.width, args.height
    s = synthetic.scene(P, W, H, 0, seed=42, edge_px=args.edge_px, with_grads=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    class Cam:
        device = dev
        image_width, image_height, tan_fovx, tan_fovy = W, H, s["tanfovx"], s["tanfovy"]
        world_view_transform = t(s["viewmatrix"])
    mesh = MeshRenderer(Cam())
    vertices = t(s["vertex"].reshape(-1, 3))
    faces = torch.arange(3 * P, device=dev, dtype=torch.int32).reshape(P, 3)  # twins off: F = P, no invalid faces
    colors = t(np.random.default_rng(42).random((P, 3), dtype=np.float32))

    rs = TriangleRasterizationSettings(
        image_width=W, image_height=H, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
        campos=t(s["campos"]), sh_degree=0, gamma=1.0, scale_modifier=1.0, background_depth=5000.0, background=t(s["background"]),
        back_culling=False, rich_info=False, debug=False)
    raster = TriangleRasterizer(rs)
    vertex, shs, opacity = t(s["vertex"]), t(s["shs"]), t(s["opacity"])

    def run_mesh():
        return mesh.render(vertices, faces, colors)

    def run_splat():
        with torch.no_grad():
            return raster(vertex, center2D_sink(P, dev), opacity, shs=shs)

    def block(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    for _ in range(args.warmup):
        run_mesh()
        run_splat()
    torch.cuda.synchronize()
    times = {"mesh": [], "splat3d": []}
    for _ in range(args.blocks):
        times["mesh"].append(block(run_mesh, args.iters))
        times["splat3d"].append(block(run_splat, args.iters))

    def summary(v):
        return {"ms": round(statistics.median(v), 4), "min_block_ms": round(min(v), 4), "max_block_ms": round(max(v), 4)}

    # per-kernel times: the library's event hooks around every launch, in a run of their own
    _C.profile_reset(); _C.profile_only(""); _C.profile_enable(True)
    for _ in range(args.iters):
        run_mesh()
    torch.cuda.synchronize()
    kernels = {n: round(ms / max(c, 1), 4) for n, ms, c in _C.profile_read()}
    _C.profile_reset()
    for _ in range(args.iters):
        run_splat()
    torch.cuda.synchronize()
    splat_kernels = {n: round(ms / max(c, 1), 4) for n, ms, c in _C.profile_read()}
    _C.profile_enable(False); _C.profile_reset()

    mesh.wave_visits = torch.zeros(1, device=dev, dtype=torch.int64)
    out = run_mesh()
    torch.cuda.synchronize()
    visits, pairs = int(mesh.wave_visits.item()), mesh.last_num_rendered
    mesh.wave_visits = None
    m, sp = summary(times["mesh"]), summary(times["splat3d"])
    result = {
        "workload": f"S(P={P}, {W}x{H}, edge {args.edge_px:g} px, seed 42), F = P faces (no twins, no invalid faces)",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls per renderer after {args.warmup} warm-up calls each, device events around each block",
        "mesh_render": m, "splat3d_forward_rich_info_false_sh0": sp,
        "mesh_not_slower": m["ms"] <= sp["ms"] or m["min_block_ms"] <= sp["max_block_ms"],
        "mesh_kernels_avg_ms": kernels, "splat3d_kernels_avg_ms": splat_kernels,
        "tile_face_pairs_in_lists": pairs, "wave_face_pairs_in_lists": 4 * pairs, "wave_face_pairs_visited": visits,
        "visited_share": round(visits / max(4 * pairs, 1), 4),
        "covered_share": round(float(out["mask"].mean().item()), 4),
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
