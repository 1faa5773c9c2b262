"""Times the four kernels of diff_recon_hip.color_volume (csrc/color_volume.hip) at the size a reconstruction uses, a first measurement:

    python tools/bench_color_volume.py [--grid 256 --large 512 --view 800 --blocks 10 --iters 20 --warmup 3 --out profiles/color_volume.json]

    color_integrate   tsc_integrate (through the C ABI) of one --view x --view depth and colour image of a sphere into a --grid^3 volume
    tsdf_integrate    TSDFVolume.integrate of the same view without carving: the distance kernel beside it, a yardstick
    copy              dst.copy_(src) of 28 bytes per sample, the colour state: the streaming yardstick, measured in the same blocks
    color_field       ColorTSDFVolume.color_field of that volume
    sample            sample_grid of the colour field at the welded vertices of the extracted surface
    interpolate       interpolate_vertex_attributes of the extracted mesh's vertex colours over MeshRenderer's face_idx at 1920 x 1080

The protocol is tools/bench_volume.py's: device events around alternating blocks after a warm-up, public wrappers (allocation of outputs
included), every part reported with the least bytes it must move and the rate that gives, and as a fraction of the copy rate.  The colour
state of a 256^3 volume (448 MiB) is past the 256 MiB Infinity Cache already; --large N repeats the measurement at N^3 under the key "large".
Writes, and prints as one JSON line, the median block time of every part with the slowest and fastest block.
Needs a HIP device; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd"), os.path.join(ROOT, "tools")]
import torch

from bench_volume import sphere_view

WIDE, HIGH = 1920, 1080


def sphere_image(cam, depth, distance):
    """(3, H, W): 0.5 + 0.4 n at the hit point of every covered pixel of sphere_view's depth, 0 elsewhere."""
    side = depth.shape[0]
    x = ((torch.arange(side, device=depth.device, dtype=torch.float64) + 0.5) / (0.5 * side) - 1.0) * cam.tan_fovx
    t = depth.to(torch.float64)
    hit = torch.stack([x[None, :] * t, x[:, None] * t, t - distance])
    colour = 0.5 + 0.4 * hit / hit.norm(dim=0, keepdim=True).clamp(min=1e-30)
    return torch.where(depth[None] > 0, colour, torch.zeros_like(colour)).to(torch.float32).contiguous()


def measure(G, args, dev):
    from diff_recon_hip import MeshRenderer
    from diff_recon_hip import color_volume as CV
    from diff_recon_hip.volume import TSDFVolume
    side = args.view
    n = G ** 3
    h = 2.0 / (G - 1)  # the cube [-1, 1]^3
    vol = CV.ColorTSDFVolume((-1.0, -1.0, -1.0), h, (G, G, G), 4.0 * h, dev)
    cam, depth = sphere_view(side, 0.6, 3.0, 0.45, dev)
    image = sphere_image(cam, depth, 3.0)
    updated, coloured = torch.zeros(1, device=dev, dtype=torch.int64), torch.zeros(1, device=dev, dtype=torch.int64)
    vol.integrate(cam, depth, image=image, carve_uncovered=True, updated=updated, colored=coloured)
    mesh = vol.extract()
    TSDFVolume.integrate(vol, cam, depth, updated=updated.zero_())
    n_updated, n_coloured = int(updated.item()), int(coloured.item())
    field = vol.color_field()
    vertices, faces, colour = mesh.vertices, mesh.faces, mesh.vertex_color
    N, F = vertices.shape[0], faces.shape[0]
    g = ((vertices.to(torch.float64) + 1.0) / h).floor().clamp(max=G - 2).to(torch.int64)
    base = (g[:, 2] * G + g[:, 1]) * G + g[:, 0]
    corners = torch.cat([base + dx + dy * G + dz * G * G for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    touched = int(torch.unique(corners).numel())  # the grid samples the sampler reads, each counted once
    wide, _ = sphere_view(HIGH, 0.6, 3.0, 0.45, dev)
    wide.image_width, wide.tan_fovx = WIDE, 0.45 * WIDE / HIGH
    face_idx = MeshRenderer(wide).render(vertices=vertices, faces=faces, faces_color=torch.zeros((F, 3), device=dev))["face_idx"]
    drawn = int((face_idx >= 0).sum())
    bg = torch.zeros(3, device=dev)
    src, dst = torch.empty((28 * n,), device=dev, dtype=torch.uint8).fill_(1), torch.empty((28 * n,), device=dev, dtype=torch.uint8)

    def color_integrate():
        rc = CV._lib.tsc_integrate(G, G, G, *vol.origin, vol.voxel_size, vol.trunc, cam.world_view_transform.data_ptr(), cam.tan_fovx, cam.tan_fovy,
                                   side, side, depth.data_ptr(), None, image.data_ptr(), vol.csum.data_ptr(), vol.cweight.data_ptr(), None,
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, CV._lib.tsc_last_error()

    parts = {
        "color_integrate": color_integrate,
        "tsdf_integrate": lambda: TSDFVolume.integrate(vol, cam, depth),
        "copy": lambda: dst.copy_(src),
        "color_field": lambda: vol.color_field(),
        "sample": lambda: CV.sample_grid(field, vol.origin, vol.voxel_size, vertices),
        "interpolate": lambda: CV.interpolate_vertex_attributes(wide, vertices, faces, face_idx, colour, bg),
    }

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
    out = {k: {"ms": round(statistics.median(v), 4), "min_block_ms": round(min(v), 4), "max_block_ms": round(max(v), 4)} for k, v in times.items()}
    print(", ".join(f"{k} {v['ms']:.3f} ms" for k, v in out.items()), file=sys.stderr, flush=True)
    model = {  # bytes each part has to move at the least
        "color_integrate": 56 * n_coloured + 16 * side * side,  # the 28 bytes of a coloured sample read and written, depth and colour once
        "tsdf_integrate": 24 * n_updated + 4 * side * side,     # the 12 bytes of an updated sample read and written, the depth once
        "copy": 56 * n,
        "color_field": 16 * n + 24 * n_coloured,                # the weight read, 12 bytes written per sample; the sums of a coloured one
        "sample": 25 * N + 12 * touched,                        # the point, its colour and its flag; every grid sample it reads once
        "interpolate": 16 * WIDE * HIGH + 12 * F + 24 * N,      # face_idx read, three planes written; the mesh and its colours once
    }
    for k, v in out.items():
        v["model_bytes"] = model[k]
        v["model_GB_per_s"] = round(model[k] / (v["ms"] * 1e-3) / 1e9, 1)
        v["of_copy_rate"] = round(v["model_GB_per_s"] / (model["copy"] / (out["copy"]["ms"] * 1e-3) / 1e9), 3)
    for k, count in (("color_integrate", n_coloured), ("tsdf_integrate", n_updated)):  # what the two cost is the projection of every sample
        out[k].update({"samples": n, "touched": count, "Gsamples_per_s": round(n / (out[k]["ms"] * 1e-3) / 1e9, 1)})
    out["sample"].update({"points": N, "grid_samples_touched": touched})
    out["interpolate"].update({"pixels": WIDE * HIGH, "drawn": drawn, "faces": F})
    return {
        "workload": f"a {G}^3 volume over [-1, 1]^3, trunc = 4 voxels; one {side} x {side} analytic depth and colour (0.5 + 0.4 n) image of a sphere of "
                    f"radius 0.6 seen from distance 3, tan(fov / 2) = 0.45: {n_coloured} of {n} samples coloured, {n_updated} updated without carving; "
                    f"sample: the {N} welded vertices of the extracted surface ({F} faces); interpolate: that mesh at {WIDE} x {HIGH} ({drawn} pixels "
                    f"drawn); copy: {28 * n} bytes device to device",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation and conversion of arguments included) except color_integrate, which is the C ABI call alone; "
                  "model_bytes is the least each part must move, not a counter reading; the weights grow by one per integrate call",
        "parts": out,
        "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume")
    ap.add_argument("--view", type=int, default=800, help="the depth and colour images are --view x --view pixels")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--large", type=int, default=0, help="measure a second volume of this many samples a side (0: none)")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_volume.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color_volume.py needs a HIP device (the colour volume kernels have no CPU fallback)")
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
