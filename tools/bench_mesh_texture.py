"""What a texture bake costs per view on an MI355X, beside what the per-face bake and the vertex-colour draw cost for the same pixels.

    python tools/bench_mesh_texture.py [--triangles 1000000 --width 1920 --height 1080 --edge-px 6 --coarse-edge-px 60 --res 1 4 16
                                        --blocks 10 --iters 200 --out profiles/mesh_texture.json]

The scene is tools/bench_mesh.py's: S(P, W x H, edge px, seed 42) drawn by MeshRenderer once; its face_idx image is the input of everything
timed here.  A second, coarse mesh of the same total area (--coarse-edge-px, 0 to skip) is the case a texture is for: few faces, many pixels
each.  Per mesh and per R (texels per face edge), alternating blocks of back-to-back calls between device events, median over the blocks with
the fastest and slowest block as the spread:

    texel_index          tsa_texel_index alone (texel_idx only; atlas_idx and bary NULL), outputs preallocated
    census_add_texels    ts2d_mesh_census_add on texel_idx with a target, F T rows -- with the run length of its key image inside 64-pixel waves
    index_then_add       the two launches back to back: one view of a bake
    resolve, face_totals tsa_resolve (with rgb8) and tsa_face_totals, once per bake
and, in the same blocks, what the parent pays for the same pixels:
    interpolate          tsc_interpolate alone (C = 3, no bary): the same barycentrics, three attribute gathers instead of the index arithmetic
    census_add_faces     ts2d_mesh_census_add on face_idx, F rows: bake_face_colors' accumulation

Writes the JSON (and prints it as one line).  Nothing here is a kernel time from a profiler: launch overhead is hidden behind the previous
kernel only where the kernel is longer than a launch; the shortest figures are launch-bound and say so ("launch_bound": median below 0.01 ms).
Every call of a block reads the same images (8 MB of keys, 25 MB of target), so the per-view figures are cache-warm: in a bake the key
image of a view has just been written, the target comes from memory."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "triangle-splatting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--edge-px", type=float, default=6.0)
    ap.add_argument("--coarse-edge-px", type=float, default=60.0, help="mean edge of the second, coarse mesh of the same total area (0: skip it)")
    ap.add_argument("--res", type=int, nargs="+", default=[1, 4, 16], help="texels per face edge")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per timed call")
    ap.add_argument("--iters", type=int, default=200, help="calls per block: a window of 4 ms and more for calls of 0.02 ms")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_texture.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_texture.py measures on a HIP device; none is visible (there is no CPU fallback and no CPU figure)")
    dev = torch.device("cuda:0")
    import synthetic
    from diff_recon_hip import MeshCensus, MeshRenderer, TextureAtlas, color_volume, mesh_texture as mt
    from diff_triangle_rasterization_2D import _C as native
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
        m = statistics.median(v)
        return {"ms": round(m, 4), "min_block_ms": round(min(v), 4), "max_block_ms": round(max(v), 4), "launch_bound": m < 0.01}

    def run_lengths(key):
        """Runs of equal keys inside 64-pixel waves of the linear sweep, over the counted pixels: what the census kernel combines."""
        flat = key.flatten()
        head = torch.ones_like(flat, dtype=torch.bool)
        head[1:] = flat[1:] != flat[:-1]
        head[::64] = True
        counted = int((flat >= 0).sum().item())
        runs = int((head & (flat >= 0)).sum().item())
        return {"counted_pixels": counted, "runs": runs, "mean_run_px": round(counted / max(runs, 1), 3)}

    def measure(P, edge_px):
        s = synthetic.scene(P, W, H, 0, seed=42, edge_px=edge_px, with_grads=False)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

        class Cam:
            device = dev
            image_width, image_height, tan_fovx, tan_fovy = W, H, s["tanfovx"], s["tanfovy"]
            world_view_transform = t(s["viewmatrix"])
        cam = Cam()
        tx, ty = float(cam.tan_fovx), float(cam.tan_fovy)
        vertices = t(s["vertex"].reshape(-1, 3))
        faces = torch.arange(3 * P, device=dev, dtype=torch.int32).reshape(P, 3)
        face_idx = MeshRenderer(cam).render(vertices, faces, torch.zeros((P, 3), device=dev))["face_idx"]
        view, stream = cam.world_view_transform.contiguous(), native.stream()
        attributes, background = torch.rand((3 * P, 3), device=dev), torch.zeros(3, device=dev)
        interpolated = torch.empty((3, H, W), device=dev)
        face_census = MeshCensus(P, dev)

        def run_interpolate():
            color_volume._check(color_volume._lib.tsc_interpolate(view.data_ptr(), tx, ty, W, H, 3 * P, vertices.data_ptr(), P,
                                                                  faces.data_ptr(), face_idx.data_ptr(), 3, attributes.data_ptr(), background.data_ptr(),
                                                                  interpolated.data_ptr(), None, stream), "interpolate")

        def run_face_census():
            face_census.add(face_idx, target)

        out = {"workload": f"S(P={P}, {W}x{H}, edge {edge_px:g} px, seed 42), F = P faces, random target", "face_idx": run_lengths(face_idx), "res": {}}
        for R in args.res:
            atlas = TextureAtlas(P, R, dev)
            lay = atlas.layout
            texel = torch.empty((H, W), device=dev, dtype=torch.int32)
            totals = torch.empty((P, 4), device=dev, dtype=torch.int64)
            image = torch.empty((3, lay.height, lay.width), device=dev)
            state = torch.empty((lay.height, lay.width), device=dev, dtype=torch.uint8)
            rgb8 = torch.empty((lay.height, lay.width, 3), device=dev, dtype=torch.uint8)
            fill = (C.c_float * 3)(0.5, 0.5, 0.5)

            def run_index():
                mt._check(mt._lib.tsa_texel_index(view.data_ptr(), tx, ty, W, H, 3 * P, vertices.data_ptr(), P, faces.data_ptr(),
                                                  face_idx.data_ptr(), R, lay.cells_per_row, texel.data_ptr(), None, None, stream), "texel_index")

            def run_add():
                atlas.census.add(texel, target)

            def run_both():
                run_index()
                run_add()

            def run_totals():
                mt._check(mt._lib.tsa_face_totals(P, R, atlas.texels.data_ptr(), totals.data_ptr(), stream), "face_totals")

            def run_resolve():
                mt._check(mt._lib.tsa_resolve(P, R, lay.cells_per_row, lay.cells_per_col, atlas.texels.data_ptr(), totals.data_ptr(), 1, None, fill,
                                              image.data_ptr(), state.data_ptr(), rgb8.data_ptr(), stream), "resolve")

            calls = {"texel_index": run_index, "census_add_texels": run_add, "index_then_add": run_both, "interpolate": run_interpolate,
                     "census_add_faces": run_face_census, "face_totals": run_totals, "resolve": run_resolve}
            run_index()
            for _ in range(args.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(args.blocks):
                for k, fn in calls.items():
                    times[k].append(block(fn, args.iters))
            row = {k: summary(v) for k, v in times.items()}
            row.update(texels=P * lay.texels_per_face, accumulator_bytes=32 * P * lay.texels_per_face, atlas=[lay.width, lay.height],
                       texel_idx=run_lengths(texel), texels_observed=int((atlas.texels[:, 0] > 0).sum().item()),
                       two_launch_sum_ms=round(row["texel_index"]["ms"] + row["census_add_texels"]["ms"], 4),
                       parent_per_face_bake_ms=row["census_add_faces"]["ms"])
            # the accumulator is an exact function of the calls: every add counts every drawn pixel once
            adds = args.warmup * 2 + args.blocks * args.iters * 2
            assert int(atlas.texels[:, 0].sum().item()) == adds * row["texel_idx"]["counted_pixels"], "the atlas lost or gained pixels"
            out["res"][str(R)] = row
            del atlas, image, state, rgb8, totals
            torch.cuda.empty_cache()
        return out

    result = {
        "method": f"{args.blocks} alternating blocks x {args.iters} back-to-back calls of each entry after {args.warmup} warm-up rounds, device events "
                  "around each block; ms = median block, min / max block = the spread; launch_bound marks medians below 0.01 ms",
        "headline": measure(args.triangles, args.edge_px),
        "device": torch.cuda.get_device_name(dev),
    }
    if args.coarse_edge_px > 0:
        coarse_P = max(int(round(args.triangles * (args.edge_px / args.coarse_edge_px) ** 2)), 1)  # the same total area
        result["coarse"] = measure(coarse_P, args.coarse_edge_px)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
