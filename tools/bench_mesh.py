"""Times the opaque mesh renderer (diff_recon_hip.MeshRenderer) next to what a user had to use before to look at a mesh: the 3D splat
rasterizer's forward with rich_info=False and SH degree 0 on the same triangles, called the way `bench.py --forward-only --rasterizer 3D`
calls it.  One process, alternating blocks, device events, after a warm-up:

    python tools/bench_mesh.py [--triangles 1000000 --width 1920 --height 1080 --edge-px 6 --blocks 10 --iters 20 --out profiles/mesh_render.json]

Writes (and prints as one JSON line): both times per call (median over the blocks) with their spread (min / max block), the mesh render's
per-kernel times (the library's event hooks, a run of its own: the hooks serialise the launches), and how many (wavefront, face) pairs the
depth test walked against four times the pairs in the tile lists -- what the early stop saved.  Needs a HIP device; there is no fallback.

    python tools/bench_mesh.py --census [--coarse-edge-px 60 --out profiles/mesh_census.json]

times the per-face census (diff_recon_hip.MeshCensus.add over csrc/mesh_census.hip) instead: alternating blocks of `render` and
`render + census add` with the same block and warm-up counts, the census alone on a fixed face_idx image, the kernel's own time from the
library's event hooks, and the run statistics that decide its atomic traffic (runs = maximal equal-index stretches inside a wavefront's 64
pixels; one row update of four 64-bit adds per run).  The same on a coarse mesh of the same coverage (--coarse-edge-px), where runs are long."""
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
    ap.add_argument("--out", default=None, help="default: profiles/mesh_render.json, with --census profiles/mesh_census.json")
    ap.add_argument("--census", action="store_true", help="time MeshCensus.add next to the render it follows instead (see above)")
    ap.add_argument("--coarse-edge-px", type=float, default=60.0, help="--census: mean edge of the second, coarse mesh (0: skip it)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mesh_census.json" if args.census else "mesh_render.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a HIP device (neither renderer has a CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.census:
        return census_main(args, dev)
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


def census_main(args, dev):
    import synthetic
    from diff_recon_hip import MeshCensus, MeshRenderer
    from diff_triangle_rasterization_2D import _C
    W, H = args.width, args.height
    target = torch.from_numpy(np.random.default_rng(43).random((3, H, W), dtype=np.float32)).to(dev)

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

    def measure(P, edge_px):
        s = synthetic.scene(P, W, H, 0, seed=42, edge_px=edge_px, with_grads=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

        class Cam:
            device = dev
            image_width, image_height, tan_fovx, tan_fovy = W, H, s["tanfovx"], s["tanfovy"]
            world_view_transform = t(s["viewmatrix"])
        mesh = MeshRenderer(Cam())
        vertices = t(s["vertex"].reshape(-1, 3))
        faces = torch.arange(3 * P, device=dev, dtype=torch.int32).reshape(P, 3)
        colors = t(np.random.default_rng(42).random((P, 3), dtype=np.float32))
        census = MeshCensus(P, dev)

        def run_render():
            return mesh.render(vertices, faces, colors)

        def run_both():
            census.add(mesh.render(vertices, faces, colors)["face_idx"], target)

        fixed = run_render()["face_idx"]

        def run_census():
            census.add(fixed, target)

        def run_count():
            census.add(fixed)

        for _ in range(args.warmup):
            run_render()
            run_both()
            run_count()
        torch.cuda.synchronize()
        times = {"render": [], "both": [], "census": [], "count": []}
        for _ in range(args.blocks):
            times["render"].append(block(run_render, args.iters))
            times["both"].append(block(run_both, args.iters))
            times["census"].append(block(run_census, args.iters))
            times["count"].append(block(run_count, args.iters))
        _C.profile_reset(); _C.profile_only("mesh_census"); _C.profile_enable(True)
        for _ in range(args.iters):
            run_census()
        torch.cuda.synchronize()
        kernel = {n: round(ms / max(c, 1), 4) for n, ms, c in _C.profile_read()}
        _C.profile_enable(False); _C.profile_only(""); _C.profile_reset()
        # what the kernel adds: runs inside 64-pixel wavefronts of the linear sweep
        flat = fixed.flatten()
        head = torch.ones_like(flat, dtype=torch.bool)
        head[1:] = flat[1:] != flat[:-1]
        head[::64] = True
        runs = int((head & (flat >= 0)).sum().item())
        counted = int((flat >= 0).sum().item())
        per_wave = torch.nn.functional.pad(head & (flat >= 0), (0, -flat.numel() % 64)).view(-1, 64).sum(1)
        wave_atomics = int(((4 * per_wave + 63) // 64).sum().item())  # computed from the image, not a counter: four lanes per run, 64 lanes per instruction
        # the accumulator is an exact function of the calls: the last column-0 sum must be (calls so far) x (counted pixels)
        calls = args.warmup * 2 + args.blocks * args.iters * 3 + args.iters
        assert int(census.acc[:, 0].sum().item()) == calls * counted, "census lost or gained pixels"
        r, bo, ce, co = (summary(times[k]) for k in ("render", "both", "census", "count"))
        diff = [b - a for a, b in zip(times["render"], times["both"])]
        return {
            "workload": f"S(P={P}, {W}x{H}, edge {edge_px:g} px, seed 42), F = P faces, random target",
            "render": r, "render_plus_census_add": bo, "census_add_after_render_ms": summary(diff),
            "census_add_alone_back_to_back": ce, "census_add_without_target_back_to_back": co, "mesh_census_kernel_avg_ms": kernel.get("mesh_census"),
            "counted_pixels": counted, "runs": runs, "mean_run_px": round(counted / max(runs, 1), 3), "faces_with_pixels": int((census.acc[:, 0] > 0).sum().item()),
            "atomic_wave_instructions_computed": wave_atomics, "atomic_lane_adds_upper_bound": 4 * runs, "atomic_bytes_upper_bound": 32 * runs,
            "read_bytes": 16 * W * H, "census_not_slower_than_render": summary(diff)["ms"] <= r["ms"],
        }

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} calls each of render / render + census add / census add alone / count only, after "
                  f"{args.warmup} warm-up calls, device events around each block; census_add_after_render = per-block difference of the first two",
        "headline": measure(args.triangles, args.edge_px),
        "device": torch.cuda.get_device_name(dev),
    }
    if args.coarse_edge_px > 0:
        coarse_P = max(int(round(args.triangles * (args.edge_px / args.coarse_edge_px) ** 2)), 1)  # the same total area
        result["coarse"] = measure(coarse_P, args.coarse_edge_px)
    h = result["headline"]
    k = h["mesh_census_kernel_avg_ms"] or h["census_add_alone_back_to_back"]["ms"]
    result["headline_kernel_rates"] = {"read_GB_per_s": round(h["read_bytes"] / k / 1e6, 1), "atomic_row_updates_per_us": round(h["runs"] / k / 1e3, 1),
                                       "atomic_GB_per_s_upper_bound": round(h["atomic_bytes_upper_bound"] / k / 1e6, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
