"""What the generalised winding number costs on an MI355X, what its far field saves and what it gives up, beside the ray counts of mesh_inside.py.

    python tools/bench_mesh_winding.py [--faces 1000000 --points 1000000 --exact-points 4096 --betas 1.5 2 3 --grids 64 128 --blocks 7 --iters 3
                                        --out profiles/mesh_winding.json]

Meshes: tools/bench_mesh_distance.py --rays' soup, --faces triangles of edge about 0.01 spread over the unit cube, and tools/bench_mesh_inside.py's
height field of about --faces faces over the unit square (an OPEN mesh: what the feature is for).  On each, --points points uniform in the
mesh's box; the index and the node moments are built once.  In alternating blocks of back-to-back calls between device events, median over
the blocks with the fastest and slowest block as the spread:

    gwn_beta_B                          generalized_winding_number at each of --betas
    gwn_exact                           the same with beta = inf on the first --exact-points points (every face for every point)
    moments                             winding_moments on a fresh index (the build of the index itself is outside)
with, from a call of its own per beta, the mean faces evaluated and nodes accepted per point and the largest |w_beta - w_exact| over the
--exact-points points.

Grids, on the height field, at --grids samples along each axis of the cube of bench_mesh_inside.py: contains_points and the distance volume
with both methods -- mesh_to_sdf (rays) beside mesh_to_sdf_winding.  The rays rows are the yardstick: they are what the parent commit runs.

Public wrappers throughout: allocation of outputs and workspaces included.  No time here is a pass / fail condition.  Writes the JSON and
prints it as one line."""
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
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--exact-points", type=int, default=4096, help="the exact form (beta = inf) runs on this many points")
    ap.add_argument("--betas", type=float, nargs="*", default=[1.5, 2.0, 3.0])
    ap.add_argument("--grids", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--blocks", type=int, default=7, help="alternating blocks per part")
    ap.add_argument("--iters", type=int, default=3, help="calls per block (the exact form and the grids: one)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_winding.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    from bench_mesh_distance import height_field
    from diff_recon_hip.mesh_inside import _grid_points, contains_points, mesh_to_sdf
    from diff_recon_hip.mesh_surface import MeshBVH
    from diff_recon_hip.mesh_winding import (UNITS_PER_TURN, contains_points_winding, generalized_winding_number, mesh_to_sdf_winding,
                                             winding_moments)

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

    F, P, E = args.faces, args.points, min(args.exact_points, args.points)
    g = torch.Generator(device=dev).manual_seed(42)
    tri = torch.rand((F, 1, 3), device=dev, generator=g) + (torch.rand((F, 3, 3), device=dev, generator=g) - 0.5) * 0.01
    soup = (tri.reshape(-1, 3).contiguous(), torch.arange(3 * F, device=dev, dtype=torch.int32).reshape(F, 3))
    soup_pts = torch.rand((P, 3), device=dev, generator=g)
    n = int(round((F / 2) ** 0.5)) + 1
    field = height_field(n, 0.05, 0.0, dev)
    field_pts = torch.rand((P, 3), device=dev, generator=g) * torch.tensor([1.0, 1.0, 0.2], device=dev) - torch.tensor([0.0, 0.0, 0.1], device=dev)

    def name_of(beta):
        return f"gwn_beta_{beta:g}"

    meshes = {}
    for name, (v, f), pts, where in (("soup", soup, soup_pts, "uniform in the unit cube"),
                                     ("height_field", field, field_pts, "uniform in [0, 1]^2 x [-0.1, 0.1]")):
        bvh = MeshBVH(v, f)
        winding_moments(bvh)
        parts = {name_of(b): (lambda b=b: generalized_winding_number(pts, bvh, beta=b)) for b in args.betas}
        t = timed(parts, args.iters)
        t.update(timed({"gwn_exact": lambda: generalized_winding_number(pts[:E], bvh, beta=float("inf"))}, 1))
        fresh = [MeshBVH(v, f) for _ in range(args.warmup + args.blocks)]  # an index each: the moments are cached on it
        it = iter(fresh)
        for _ in range(args.warmup):
            winding_moments(next(it))
        torch.cuda.synchronize()
        t["moments"] = summary([block(lambda: winding_moments(next(it)), 1) for _ in range(args.blocks)])
        del fresh
        _, exact = generalized_winding_number(pts[:E], bvh, beta=float("inf"))
        for b in args.betas:
            _, wq, terms = generalized_winding_number(pts, bvh, beta=b, return_terms=True)
            torch.cuda.synchronize()
            t[name_of(b)].update(ns_per_point=round(t[name_of(b)]["ms"] * 1e6 / P, 2),
                                 mean_faces_evaluated=round(float(terms[:, 0].double().mean().item()), 2),
                                 mean_nodes_accepted=round(float(terms[:, 1].double().mean().item()), 2),
                                 max_abs_w_minus_exact=float((wq[:E] - exact).abs().max().item()) / UNITS_PER_TURN,
                                 inside_share=round(float((wq >= UNITS_PER_TURN // 2).double().mean().item()), 4),
                                 decides_like_exact_share=round(float(((wq[:E] >= UNITS_PER_TURN // 2) == (exact >= UNITS_PER_TURN // 2)).double().mean().item()), 6))
        t["gwn_exact"].update(points=E, us_per_point=round(t["gwn_exact"]["ms"] * 1e3 / E, 2), faces_evaluated=int(f.shape[0]))
        meshes[name] = {"workload": f"{int(f.shape[0])} faces, {P} points {where}", "parts": t}
        if name == "soup":
            del bvh
            torch.cuda.empty_cache()

    grids = {}
    for res in args.grids:
        h = 1.2 / (res - 1)
        origin = (-0.1, -0.1, -0.6)
        gp =_grid_points(origin, h, (res, res, res), dev)
        t = timed({"contains_points_rays": lambda: contains_points(gp, bvh), "contains_points_winding": lambda: contains_points_winding(gp, bvh),
                   "mesh_to_sdf_rays": lambda: mesh_to_sdf(bvh, origin, h, (res, res, res)),
                   "mesh_to_sdf_winding": lambda: mesh_to_sdf_winding(bvh, origin, h, (res, res, res))}, 1)
        by_rays, by_winding = mesh_to_sdf(bvh, origin, h, (res, res, res)), mesh_to_sdf_winding(bvh, origin, h, (res, res, res))
        t["mesh_to_sdf_rays"].update(undecided=int(torch.isnan(by_rays).sum().item()), negative=int((by_rays < 0).sum().item()))
        t["mesh_to_sdf_winding"].update(undecided=int(torch.isnan(by_winding).sum().item()), negative=int((by_winding < 0).sum().item()),
                                        over_rays=round(t["mesh_to_sdf_winding"]["ms"] / t["mesh_to_sdf_rays"]["ms"], 3))
        t["contains_points_winding"].update(over_rays=round(t["contains_points_winding"]["ms"] / t["contains_points_rays"]["ms"], 3))
        for v_ in t.values():
            v_.update(samples=res ** 3, ns_per_sample=round(v_["ms"] * 1e6 / res ** 3, 2))
        grids[str(res)] = t
        del by_rays, by_winding, gp
        torch.cuda.empty_cache()

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of every part (gwn_exact, moments and the grids: one call) after "
                  f"{args.warmup} warm-up calls each, device events around each block; ms = median block, min / max block = the spread; public wrappers "
                  "(allocation of outputs and workspaces included; the index and the node moments are built once, outside; `moments` builds them on a "
                  "fresh index per block); term counts, errors and shares from a call of its own; beta defaults to 2 on the grids",
        "meshes": meshes,
        "grids": {"workload": "the height field on res^3 samples over [-0.1, 1.1]^2 x [-0.6, 0.6]; the rays rows are the parent's path", "parts": grids},
        "not_measured": "other beta on the grids; meshes above 1 M faces; the kernel alone without the Morton sort of the points; fp64 pipe utilisation",
        "device": torch.cuda.get_device_name(dev),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
