"""Times the two kernels of diff_recon_hip.volume (csrc/volume.hip) at the size a reconstruction uses, a first measurement:

    python tools/bench_volume.py [--grid 256 --large 512 --view 800 --blocks 10 --iters 20 --warmup 3 --out profiles/volume.json]

    integrate    TSDFVolume.integrate of one --view x --view depth image of a sphere (carving on) into a --grid^3 volume
    field        TSDFVolume.field of that volume
    extract      extract_isosurface of the fused field: the counting call, the read-back of the total, the allocation, the writing call
    count        the counting call alone (capacity 0) through the C ABI: what the extraction costs before any triangle is written
    copy         dst.copy_(src) of 12 bytes per sample, the volume's state: the streaming yardstick, measured in the same blocks

Timed with device events, in alternating blocks after a warm-up, like tools/bench_mesh_distance.py.  Every part is reported with the bytes its
cost model moves and the rate that gives; profiles/hbm_traffic.json prices kernels by their profiler counters and holds no copy rate, so the
yardstick is the `copy` part.  The state of a 256^3 volume (192 MiB) fits the 256 MiB Infinity Cache, so its rates are not HBM rates: --large N
repeats the measurement at N^3 (512^3 = 2^27 samples, the largest grid the library takes) under the key "large".  Writes, and prints as one
JSON line, the median block time of every part with the slowest and fastest block.
Needs a HIP device; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "triangle-splatting_amd")]
import torch


def sphere_view(side, radius, distance, tan_fov, dev):
    """(cam, depth): a camera on the -z axis looking at the origin, and the analytic view-space depth of a sphere there, 0 where a ray misses."""
    view = torch.eye(4, dtype=torch.float32)
    view[3, 2] = distance  # view = world + (0, 0, distance)
    cam = SimpleNamespace(world_view_transform=view.to(dev), tan_fovx=tan_fov, tan_fovy=tan_fov, image_width=side, image_height=side, device=dev)
    x = ((torch.arange(side, device=dev, dtype=torch.float64) + 0.5) / (0.5 * side) - 1.0) * tan_fov
    dx, dy = x[None, :].expand(side, side), x[:, None].expand(side, side)
    a = dx * dx + dy * dy + 1.0  # |o + t d|^2 = r^2 with o = (0, 0, -distance), d = (dx, dy, 1)
    b = -2.0 * distance
    disc = b * b - 4.0 * a * (distance * distance - radius * radius)
    t = (-b - disc.clamp(min=0).sqrt()) / (2.0 * a)
    return cam, torch.where(disc > 0, t, torch.zeros_like(t)).to(torch.float32).contiguous()


def measure(G, args, dev):
    from diff_recon_hip import volume as V
    side = args.view
    n = G ** 3
    h = 2.0 / (G - 1)  # the cube [-1, 1]^3
    vol = V.TSDFVolume((-1.0, -1.0, -1.0), h, (G, G, G), 4.0 * h, dev)
    cam, depth = sphere_view(side, 0.6, 3.0, 0.45, dev)
    updated = torch.zeros(1, device=dev, dtype=torch.int64)
    vol.integrate(cam, depth, carve_uncovered=True, updated=updated)
    n_updated = int(updated.item())
    field = vol.field()
    triangles = V.extract_isosurface(field, vol.origin, vol.voxel_size)[1].shape[0]
    ws = torch.empty((V._lib.tsv_extract_workspace_bytes(G, G, G),), device=dev, dtype=torch.uint8)
    total = torch.empty((1,), device=dev, dtype=torch.int64)
    src, dst = torch.empty((12 * n,), device=dev, dtype=torch.uint8).fill_(1), torch.empty((12 * n,), device=dev, dtype=torch.uint8)

    def count():
        rc = V._lib.tsv_extract(G, G, G, *vol.origin, vol.voxel_size, field.data_ptr(), 0.0, 0, None, None, total.data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, V._lib.tsv_last_error()

    parts = {
        "integrate": lambda: vol.integrate(cam, depth, carve_uncovered=True),
        "field": lambda: vol.field(),
        "extract": lambda: V.extract_isosurface(field, vol.origin, vol.voxel_size),
        "count": count,
        "copy": lambda: dst.copy_(src),
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
    blocks = (n + 255) // 256
    model = {  # bytes each part has to move at the least
        "integrate": 24 * n_updated + 4 * side * side,       # the 12 bytes of an updated sample read and written, the image once
        "field": 16 * n,                                     # 12 bytes read, 4 written per sample
        "count": 5 * n + 4 * blocks,                         # the field once, a count byte per cell, a sum per block
        "extract": 2 * (5 * n + 4 * blocks) + n + 36 * triangles,  # the counting call twice, the counts read again, 36 bytes per triangle
        "copy": 24 * n,
    }
    for k, v in out.items():
        v["model_bytes"] = model[k]
        v["model_GB_per_s"] = round(model[k] / (v["ms"] * 1e-3) / 1e9, 1)
        v["of_copy_rate"] = round(v["model_GB_per_s"] / (model["copy"] / (out["copy"]["ms"] * 1e-3) / 1e9), 3)
    out["integrate"].update({"samples": n, "updated": n_updated, "GB_per_s_at_12_bytes_per_sample": round(12 * n / (out["integrate"]["ms"] * 1e-3) / 1e9, 1)})
    out["extract"]["triangles"] = triangles
    return {
        "workload": f"a {G}^3 volume over [-1, 1]^3, trunc = 4 voxels; integrate: one {side} x {side} analytic depth image of a sphere of radius 0.6 seen "
                    f"from distance 3, tan(fov / 2) = 0.45, carving on ({n_updated} of {n} samples updated); extract: the level set of the fused field "
                    f"({triangles} triangles); copy: {12 * n} bytes device to device",
        "method": f"{args.blocks} alternating blocks x {args.iters} calls of every part after {args.warmup} warm-up calls each, device events around each "
                  "block; public wrappers (allocation of outputs and workspaces included; extract reads the total back between its two calls); "
                  "model_bytes is the least each part must move, not a counter reading; the weight of every sample grows by one per integrate call",
        "parts": out,
        "device": torch.cuda.get_device_name(dev),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256, help="samples along each side of the volume")
    ap.add_argument("--view", type=int, default=800, help="the depth image is --view x --view pixels")
    ap.add_argument("--blocks", type=int, default=10, help="alternating blocks per part")
    ap.add_argument("--large", type=int, default=0, help="measure a second volume of this many samples a side, past the Infinity Cache (0: none)")
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume.py needs a HIP device (the volume kernels have no CPU fallback)")
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
