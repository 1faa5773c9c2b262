"""Times the geometric mesh scores (diff_recon_hip.mesh_distance over csrc/mesh_distance.hip) part by part, next to
simple_knn.nearestNeighbor(points, 1) on as many points -- the search of one set against itself that shares the front half (Morton codes,
radix sort, gathered points, 1024-point boxes; csrc/ts_knn_front.h) and the candidate loop, and so the honest yardstick for the cross search:

    python tools/bench_mesh_distance.py [--points 1000000 --faces 1000000 --blocks 10 --iters 5 --warmup 3 --out profiles/mesh_distance.json]

Timed with device events, in alternating blocks after a warm-up, each through its public wrapper (workspace allocation from torch's caching
allocator included):

    cross_volume     nearest_points, Q = R = --points, both sets uniform in one volume
    cross_surface    nearest_points between two --points-sample surface sets of nearby meshes (a bumpy height field and the same field
                     displaced by a fraction of its cell)
    sample           sample_mesh_surface, --points samples of a height-field mesh of about --faces faces (includes the face areas and the
                     blocking read of the total area)
    nearest_other    simple_knn.nearestNeighbor(points, 1) on the volume's query set: the yardstick

and reads each search's (workgroup, ref box) visits from the library's counter in a run of its own.  Writes, and prints as one JSON line,
the median block time of every part with the slowest and fastest block, the visits and the ratios to the yardstick.  Needs a HIP device;
there is no fallback.

    python tools/bench_mesh_distance.py --surface [--points 1000000 --faces 1000000 ... --out profiles/mesh_surface.json]

times the point-to-SURFACE query instead (diff_recon_hip.mesh_surface over csrc/mesh_bvh.hip), the same way:

    build            MeshBVH of the second height field (about --faces faces)
    closest          MeshBVH.closest of --points surface samples of the first field against it
    cross_surface    nearest_points between those samples and as many of the second field: the point-to-point search, as context

and reads the (wave, leaf) visits of the query from the library's counter in a run of its own.

    python tools/bench_mesh_distance.py --rays [--faces 1000000 --view 800 ... --out profiles/mesh_ray.json]

times the first-hit ray query (diff_recon_hip.mesh_ray over csrc/mesh_ray.hip) on a soup of --faces small triangles in the unit cube:

    camera_rays      ray_cast of the --view x --view pixel-centre rays of a camera that looks at the cube
    random_rays      ray_cast of as many rays with random origins in the cube, each aimed at a random face
    closest          MeshBVH.closest of those origins against the same index: the point query at the same Q and F, as context

and records rays per second, the hit share and the (wave, leaf) visits of both casts."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]
import torch


def height_field(n, amplitude, phase, dev):
    """(vertices, faces) of an n x n grid over the unit square, z = amplitude * sin * cos bumps: 2 (n - 1)^2 faces."""
    g = torch.linspace(0.0, 1.0, n, device=dev)
    x, y = torch.meshgrid(g, g, indexing="ij")
    z = amplitude * torch.sin(12.0 * x + phase) * torch.cos(9.0 * y - phase)
    vertices = torch.stack([x, y, z], dim=-1).reshape(-1, 3).contiguous()
    i = (torch.arange(n - 1, device=dev)[:, None] * n + torch.arange(n - 1, device=dev)[None, :]).reshape(-1)
    faces = torch.cat([torch.stack([i, i + n, i + n + 1], dim=1), torch.stack([i, i + n + 1, i + 1], dim=1)]).to(torch.int32).contiguous()
    return vertices, faces


class LookAt:
    """The duck-typed camera of MeshRenderer and camera_rays: W x H pixels, looks from `eye` at `target`."""

    def __init__(self, W, H, eye, target, tan_fov, dev):
        eye, target = torch.tensor(eye, dtype=torch.float64), torch.tensor(target, dtype=torch.float64)
        fwd = (target - eye) / (target - eye).norm()
        right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), fwd)
        right = right / right.norm()
        view = torch.eye(4, dtype=torch.float64)
        view[:3, :3] = torch.stack([right, torch.linalg.cross(fwd, right), fwd], dim=1)
        view[3, :3] = -eye @ view[:3, :3]
        self.device, self.image_width, self.image_height, self.tan_fovx, self.tan_fovy = dev, W, H, tan_fov, tan_fov * H / W
        self.world_view_transform = view.to(torch.float32).to(dev)


def bench_rays(args, dev, block, summary):
    from diff_recon_hip.mesh_ray import camera_rays, ray_cast
    from diff_recon_hip.mesh_surface import MeshBVH
    F, side = args.faces, args.view
    g = torch.Generator(device=dev).manual_seed(42)
    tri = torch.rand((F, 1, 3), device=dev, generator=g) + (torch.rand((F, 3, 3), device=dev, generator=g) - 0.5) * 0.01
    vertices, faces = tri.reshape(-1, 3).contiguous(), torch.arange(3 * F, device=dev, dtype=torch.int32).reshape(F, 3)
    bvh = MeshBVH(vertices, faces)
    cam_o, cam_d = camera_rays(LookAt(side, side, (0.3, 0.2, -2.0), (0.5, 0.5, 0.5), 0.3, dev))
    Q = cam_o.shape[0]
    rnd_o = torch.rand((Q, 3), device=dev, generator=g)
    rnd_d = tri[torch.randint(0, F, (Q,), device=dev, generator=g)].mean(dim=1) - rnd_o
    parts = {
        "camera_rays": lambda: ray_cast(bvh, cam_o, cam_d),
        "random_rays": lambda: ray_cast(bvh, rnd_o, rnd_d),
        "closest": lambda: bvh.closest(rnd_o),
    }
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
    waves, leaves = (Q + 63) // 64, (F + 7) // 8
    for name, (o, d) in (("camera_rays", (cam_o, cam_d)), ("random_rays", (rnd_o, rnd_d))):
        visits = torch.zeros(1, device=dev, dtype=torch.int64)
        hits = ray_cast(bvh, o, d, leaf_visits=visits)
        torch.cuda.synchronize()
        out[name].update({"rays_per_second": round(Q / (out[name]["ms"] * 1e-3)), "leaf_visits": int(visits.item()),
                          "leaf_visits_per_wave": round(int(visits.item()) / waves, 2), "leaves": leaves,
                          "hit_share": round(float((hits.face >= 0).double().mean().item()), 4),
                          "over_closest": round(out[name]["ms"] / out["closest"]["ms"], 3)})
    visits = torch.zeros(1, device=dev, dtype=torch.int64)
    bvh.closest(rnd_o, visits)
    torch.cuda.synchronize()
    out["closest"].update({"leaf_visits": int(visits.item()), "leaf_visits_per_wave": round(int(visits.item()) / waves, 2)})
    return {
        "workload": f"a soup of {F} triangles of edge about 0.01 spread over the unit cube; camera_rays: the {side} x {side} = {Q} pixel-centre rays of a "
                    f"view of the cube from (0.3, 0.2, -2), tan(fov / 2) = 0.3; random_rays: {Q} rays from uniform origins in the cube, each aimed at "
                    f"the centroid of a random face; closest: MeshBVH.closest of those origins (context: the point query at the same Q and F)",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around "
                  "each block; public wrappers (allocation of outputs and workspaces included; the index is built once, outside); leaf visits and "
                  "hit share from a call of its own",
        "parts": out,
        "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--faces", type=int, default=1_000_000)
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=5, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--surface", action="store_true", help="time the point-to-surface query (MeshBVH) instead")
    ap.add_argument("--rays", action="store_true", help="time the first-hit ray query (ray_cast) instead")
    ap.add_argument("--view", type=int, default=800, help="with --rays: the camera view is --view x --view pixels")
    ap.add_argument("--out", default=None, help="default: profiles/mesh_distance.json, with --surface profiles/mesh_surface.json, with --rays profiles/mesh_ray.json")
    args = ap.parse_args()
    if args.surface and args.rays:
        ap.error("--surface and --rays are two measurements: run them one after the other")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mesh_ray.json" if args.rays else "mesh_surface.json" if args.surface else "mesh_distance.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_distance.py needs a HIP device (the mesh scores have no CPU fallback)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def block(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    def summary(v):
        return {"ms": round(statistics.median(v), 4), "min_block_ms": round(min(v), 4), "max_block_ms": round(max(v), 4)}

    if args.rays:
        result = bench_rays(args, dev, block, summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return

    from diff_recon_hip.mesh_distance import nearest_points, sample_mesh_surface
    from simple_knn import nearestNeighbor

    P = args.points
    g = torch.Generator(device=dev).manual_seed(42)
    vol_q = torch.rand((P, 3), device=dev, generator=g) * 100
    vol_r = torch.rand((P, 3), device=dev, generator=g) * 100
    n = int(round((args.faces / 2) ** 0.5)) + 1
    mesh_a, mesh_b = height_field(n, 0.05, 0.0, dev), height_field(n, 0.05, 0.02, dev)
    F = mesh_a[1].shape[0]
    surf_q, surf_r = sample_mesh_surface(*mesh_a, P, seed=0).points, sample_mesh_surface(*mesh_b, P, seed=1).points

    if args.surface:
        from diff_recon_hip.mesh_surface import MeshBVH
        bvh = MeshBVH(*mesh_b)
        parts = {
            "build": lambda: MeshBVH(*mesh_b),
            "closest": lambda: bvh.closest(surf_q),
            "cross_surface": lambda: nearest_points(surf_q, surf_r),
        }
    else:
        parts = {
            "cross_volume": lambda: nearest_points(vol_q, vol_r),
            "cross_surface": lambda: nearest_points(surf_q, surf_r),
            "sample": lambda: sample_mesh_surface(*mesh_a, P, seed=0),
            "nearest_other": lambda: nearestNeighbor(vol_q, 1),
        }
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

    if args.surface:
        visits = torch.zeros(1, device=dev, dtype=torch.int64)
        _, d2, _ = bvh.closest(surf_q, visits)
        torch.cuda.synchronize()
        waves, leaves = (P + 63) // 64, (F + 7) // 8
        out["closest"].update({"leaf_visits": int(visits.item()), "leaf_visits_per_wave": round(int(visits.item()) / waves, 2), "leaves": leaves,
                               "mean_distance": float(d2.sqrt().mean().item()),
                               "over_cross_surface": round(out["closest"]["ms"] / out["cross_surface"]["ms"], 3)})
        result = {
            "workload": f"{P} surface samples of an {n} x {n} height field against the {F} faces of the same field a phase of 0.02 apart; "
                        f"cross_surface: the same samples against {P} samples of the second field (nearest_points)",
            "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around "
                      "each block; public wrappers (allocation of the index, outputs and workspaces included); leaf visits from the library's "
                      "counter in a call of its own",
            "parts": out,
            "device": torch.cuda.get_device_name(dev),
        }
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return

    nboxes = (P + 1023) // 1024
    for name, (q, r) in (("cross_volume", (vol_q, vol_r)), ("cross_surface", (surf_q, surf_r))):
        visits = torch.zeros(1, device=dev, dtype=torch.int64)
        _, d2 = nearest_points(q, r, visits)
        torch.cuda.synchronize()
        out[name].update({"box_visits": int(visits.item()), "box_visits_per_workgroup": round(int(visits.item()) / nboxes, 2),
                          "distance_evaluations_upper_bound": int(visits.item()) * 1024 * 1024,
                          "mean_distance": float(d2.to(torch.float64).sqrt().mean().item()),
                          "over_nearest_other": round(out[name]["ms"] / out["nearest_other"]["ms"], 3)})
    result = {
        "workload": f"cross_volume: Q = R = {P} points uniform in a 100^3 cube; cross_surface: {P} surface samples each of two {n} x {n} height fields "
                    f"({F} faces) a phase of 0.02 apart; sample: {P} samples of one of them; nearest_other: simple_knn.nearestNeighbor on the cube's "
                    f"{P} queries, batch_size 1; {nboxes} boxes per set",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspace included; sample also computes the face areas and reads their sum "
                  "back); box visits from the library's counter in a call of its own",
        "parts": out,
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
