"""What counting ALL hits of a ray costs on an MI355X beside the first hit, and what a signed distance and a distance volume of a mesh cost.

    python tools/bench_mesh_inside.py [--faces 1000000 --view 800 --points 1000000 --grids 64 128 256 --blocks 10 --iters 5
                                       --out profiles/mesh_inside.json]

Rays: tools/bench_mesh_distance.py --rays' workload, a soup of --faces triangles of edge about 0.01 spread over the unit cube, the
--view x --view pixel-centre rays of its camera and as many random rays aimed at face centroids; the index is built once.  In alternating
blocks of back-to-back calls between device events, median over the blocks with the fastest and slowest block as the spread:

    cast_camera / cast_random / cast_shared            ray_cast (tsr_cast, the parent's first-hit walk) on the three sets of rays
    crossings_camera / crossings_random                ray_crossings with a direction per ray, the same rays
    crossings_shared                                   ray_crossings from the random origins along INSIDE_DIRECTIONS[0], the shared form;
                                                       cast_shared casts the same rays with the direction repeated per ray
with the (wave, leaf) visits of both walks from a call of its own.  The all-hit walk cannot prune on a nearest hit: it is supposed to cost more.

Points: bench_mesh_distance.py's mesh, a height field of about --faces faces over the unit square (an OPEN mesh: the sign means little, the
cost is that of any mesh of its size), --points points uniform in its box: `closest` (MeshBVH.closest alone), `signed_distance` (closest, one
crossings call per direction needed, the sign kernel) and `contains_points`.  Grids: mesh_to_sdf of the same mesh at --grids samples
along each axis of a cube around it, one call per block.

Public wrappers throughout: allocation of outputs and workspaces included.  Writes the JSON and prints it as one line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=1_000_000)
    ap.add_argument("--view", type=int, default=800, help="the camera view is --view x --view pixels; as many random rays")
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--grids", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=5, help="calls per block (the grids: one)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_inside.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_inside.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    from bench_mesh_distance import LookAt, height_field
    from diff_recon_hip.mesh_inside import INSIDE_DIRECTIONS, contains_points, mesh_to_sdf, ray_crossings, signed_distance
    from diff_recon_hip.mesh_ray import camera_rays, ray_cast
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

    def timed(parts, iters):
        for _ in range(args.warmup):
            for fn in parts.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in parts}
        for _ in range(args.blocks):
            for k, fn in parts.items():
                times[k].append(block(fn, iters))
        out = {k: summary(v) for k, v in times.items()}
        print(", ".join(f"{k} {v['ms']:.3f} ms" for k, v in out.items()), file=sys.stderr, flush=True)
        return out

    # ---- rays -----------------------------------------------------------------------------------------------------------------------------
    F, side = args.faces, args.view
    g = torch.Generator(device=dev).manual_seed(42)
    tri = torch.rand((F, 1, 3), device=dev, generator=g) + (torch.rand((F, 3, 3), device=dev, generator=g) - 0.5) * 0.01
    vertices, faces = tri.reshape(-1, 3).contiguous(), torch.arange(3 * F, device=dev, dtype=torch.int32).reshape(F, 3)
    bvh = MeshBVH(vertices, faces)
    cam_o, cam_d = camera_rays(LookAt(side, side, (0.3, 0.2, -2.0), (0.5, 0.5, 0.5), 0.3, dev))
    Q = cam_o.shape[0]
    rnd_o = torch.rand((Q, 3), device=dev, generator=g)
    rnd_d = tri[torch.randint(0, F, (Q,), device=dev, generator=g)].mean(dim=1) - rnd_o
    one = torch.tensor(INSIDE_DIRECTIONS[0], device=dev, dtype=torch.float32)
    one_d = one.expand(Q, 3).contiguous()
    sets = {"camera": (cam_o, cam_d, cam_d), "random": (rnd_o, rnd_d, rnd_d), "shared": (rnd_o, one_d, one)}
    parts = {}
    for name, (o, d_cast, d_cross) in sets.items():
        parts["cast_" + name] = lambda o=o, d=d_cast: ray_cast(bvh, o, d)
        parts["crossings_" + name] = lambda o=o, d=d_cross: ray_crossings(bvh, o, d)
    rays = timed(parts, args.iters)
    waves, leaves = (Q + 63) // 64, (F + 7) // 8
    for name, (o, d_cast, d_cross) in sets.items():
        v_cast, v_cross = torch.zeros(1, device=dev, dtype=torch.int64), torch.zeros(1, device=dev, dtype=torch.int64)
        first = ray_cast(bvh, o, d_cast, leaf_visits=v_cast)
        c = ray_crossings(bvh, o, d_cross, leaf_visits=v_cross)
        torch.cuda.synchronize()
        assert torch.equal(c.hits == 0, first.face < 0), "the two walks disagree on who hits nothing"
        rays["cast_" + name].update(leaf_visits=int(v_cast.item()), leaf_visits_per_wave=round(int(v_cast.item()) / waves, 2),
                                    rays_per_second=round(Q / (rays["cast_" + name]["ms"] * 1e-3)))
        rays["crossings_" + name].update(leaf_visits=int(v_cross.item()), leaf_visits_per_wave=round(int(v_cross.item()) / waves, 2),
                                         rays_per_second=round(Q / (rays["crossings_" + name]["ms"] * 1e-3)),
                                         over_cast=round(rays["crossings_" + name]["ms"] / rays["cast_" + name]["ms"], 3),
                                         hit_share=round(float((c.hits > 0).double().mean().item()), 4),
                                         mean_hits=round(float(c.hits.double().mean().item()), 3),
                                         unclean=int(((c.touches != 0) | ((c.winding2 & 1) != 0)).sum().item()))
    del bvh, tri, vertices, faces, parts
    torch.cuda.empty_cache()

    # ---- points and grids on the height field ---------------------------------------------------------------------------------------------
    n = int(round((F / 2) ** 0.5)) + 1
    hv, hf = height_field(n, 0.05, 0.0, dev)
    hb = MeshBVH(hv, hf)
    P = args.points
    pts = torch.rand((P, 3), device=dev, generator=g) * torch.tensor([1.0, 1.0, 0.2], device=dev) - torch.tensor([0.0, 0.0, 0.1], device=dev)
    points = timed({"closest": lambda: hb.closest(pts), "signed_distance": lambda: signed_distance(pts, hb),
                    "contains_points": lambda: contains_points(pts, hb)}, args.iters)
    sdf, _, decided = signed_distance(pts, hb)
    points["signed_distance"].update(ns_per_point=round(points["signed_distance"]["ms"] * 1e6 / P, 2), undecided=int((~decided).sum().item()),
                                     negative_share=round(float((sdf < 0).double().mean().item()), 4),
                                     over_closest=round(points["signed_distance"]["ms"] / points["closest"]["ms"], 3))
    grids = {}
    for res in args.grids:
        h = 1.2 / (res - 1)
        origin = (-0.1, -0.1, -0.6)
        t = timed({f"mesh_to_sdf_{res}": lambda: mesh_to_sdf(hb, origin, h, (res, res, res))}, 1)[f"mesh_to_sdf_{res}"]
        field = mesh_to_sdf(hb, origin, h, (res, res, res))
        t.update(samples=res ** 3, ns_per_sample=round(t["ms"] * 1e6 / res ** 3, 2), undecided=int(torch.isnan(field).sum().item()))
        grids[str(res)] = t
        del field
        torch.cuda.empty_cache()

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part (the grids: one call) after {args.warmup} warm-up "
                  "calls each, device events around each block; ms = median block, min / max block = the spread; public wrappers (allocation of "
                  "outputs and workspaces included; the index is built once, outside); leaf visits and shares from a call of its own",
        "rays": {"workload": f"a soup of {F} triangles of edge about 0.01 spread over the unit cube; camera: the {side} x {side} = {Q} pixel-centre rays of "
                             f"a view of the cube from (0.3, 0.2, -2), tan(fov / 2) = 0.3; random: {Q} rays from uniform origins in the cube, each aimed "
                             f"at the centroid of a random face; shared: the same origins along INSIDE_DIRECTIONS[0]; {leaves} leaves, {waves} waves",
                 "parts": rays},
        "points": {"workload": f"a height field of {hf.shape[0]} faces over the unit square (open), {P} points uniform in [0, 1]^2 x [-0.1, 0.1]",
                   "parts": points},
        "grids": {"workload": f"mesh_to_sdf of the same height field on res^3 samples over [-0.1, 1.1]^2 x [-0.6, 0.6]", "parts": grids},
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
