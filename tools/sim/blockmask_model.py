"""numpy (float32) model of the 4x4 BLOCK masks of csrc/ts2d_support.h (block_mask, quad_anchor + block_mask_affine, on a quad_setup<3>): the emission kernel
forms them once per instance and hands them to the blend kernels in the spare bits of the tile key.  A block that holds a pixel the blend kernels'
per-pixel test accepts (render_group.hip: barycentrics -> ecc -> ecc_in_range, alpha >= 1/255) must never be left unflagged.  Same populations as
qmask_model.py (slivers, 0.2 - 600 px, opacities around 1/255, gamma 0.5 - 50, rectangles of up to 41 x 41 tiles); also reports how many blocks
the masks flag against the in-kernel block_cull they replace, restated here too.   python tools/sim/blockmask_model.py [n] [seed]

Bit 4 q + g of a mask: quadrant q = qy << 1 | qx of the tile, block g = gy << 1 | gx of the quadrant, i.e. the 4x4 block at pixel offset
(8 qx + 4 gx, 8 qy + 4 gy) from the tile's origin."""
import sys
import numpy as np

from qmask_model import f32, fma32, quad_setup, support_scale

# column i / row j of the tile's 4 x 4 blocks -> mask bit
BIT = np.array([[4 * (2 * (j >> 1) + (i >> 1)) + 2 * (j & 1) + (i & 1) for i in range(4)] for j in range(4)])  # [j][i]


def block_offsets(q):
    """The 4x4 sample box's acceptance offsets (quad_setup<3>)."""
    m = (f32(1.0) - q["E"]) * f32(1.0 / 3.0)
    out = []
    for k in "123":
        A, B = q["A" + k], q["B" + k]
        out.append((np.maximum(f32(0), f32(3) * A) + np.maximum(f32(0), f32(3) * B) - m + (f32(2e-6) * f32(15)) * (np.abs(A) + np.abs(B))).astype(f32))
    return out


def block_bits(k, A, B, bminx, bmaxx, bminy, bmaxy, live, TX, TY):
    """ts2d_support.h: block_bits -- k[e] = edge e's acceptance value at the tile's origin; separable: four x terms, four y terms per edge."""
    n = len(TX)
    ok = np.ones((n, 4, 4), bool)  # [n, j, i]
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(3):
            kx = np.stack([fma32(np.full_like(A[e], 4 * i), A[e], k[e]) for i in range(4)], 1)
            nyb = np.stack([(f32(-4 * j) * B[e]).astype(f32) for j in range(4)], 1)
            ok &= kx[:, None, :] >= nyb[:, :, None]
    xs = np.stack([live & (bminx <= TX + f32(4 * i + 3)) & (bmaxx >= TX + f32(4 * i)) for i in range(4)], 1)
    ys = np.stack([(bminy <= TY + f32(4 * j + 3)) & (bmaxy >= TY + f32(4 * j)) for j in range(4)], 1)
    ok &= xs[:, None, :] & ys[:, :, None]
    return (ok.astype(np.int64) << BIT[None]).sum((1, 2))


def block_mask(q, Q, TX, TY):
    """ts2d_support.h: block_mask -- per tile, the constants evaluated at the tile's own origin."""
    v = q["v"]
    u1x, u1y, u2x, u2y, u3x, u3y = v[:, 0] - TX, v[:, 1] - TY, v[:, 2] - TX, v[:, 3] - TY, v[:, 4] - TX, v[:, 5] - TY
    t1a, t1b, t2a, t2b, aia = u2x * u3y, u2y * u3x, u3x * u1y, u3y * u1x, np.abs(q["ia"])
    C1 = (t1a - t1b) * q["ia"]; C2 = (t2a - t2b) * q["ia"]; C3 = f32(1.0) - C1 - C2
    r1 = f32(4e-7) * (np.abs(t1a) + np.abs(t1b)) * aia; r2 = f32(4e-7) * (np.abs(t2a) + np.abs(t2b)) * aia
    k = [(C1 + Q[0] + r1).astype(f32), (C2 + Q[1] + r2).astype(f32), (C3 + Q[2] + (r1 + r2 + f32(4e-7))).astype(f32)]
    return block_bits(k, [q["A" + c] for c in "123"], [q["B" + c] for c in "123"], q["bminx"], q["bmaxx"], q["bminy"], q["bmaxy"], q["live"], TX, TY)


def block_anchor(q, Q, TX0, TY0, Wpx, Hpx):
    """ts2d_support.h: quad_anchor on a quad_setup<3> -- the block form's constants over the triangle's tile rectangle (margins as the quadrant form's)."""
    v = q["v"]
    u = [v[:, i] - (TX0 if i % 2 == 0 else TY0) for i in range(6)]
    aia = np.abs(q["ia"])
    C1 = (u[2] * u[5] - u[3] * u[4]) * q["ia"]; C2 = (u[4] * u[1] - u[5] * u[0]) * q["ia"]; C3 = f32(1.0) - C1 - C2
    U = [np.maximum(np.abs(u[i]), np.abs(u[i] - (Wpx if i % 2 == 0 else Hpx))) for i in range(6)]
    r1 = f32(4e-7) * (U[2] * U[5] + U[3] * U[4]) * aia; r2 = f32(4e-7) * (U[4] * U[1] + U[5] * U[0]) * aia
    s = [f32(6e-7) * (np.abs(q["A" + c]) * Wpx + np.abs(q["B" + c]) * Hpx) + f32(2.5e-7) * np.abs(C) for c, C in zip("123", (C1, C2, C3))]
    K = [(C1 + Q[0] + r1 + s[0]).astype(f32), (C2 + Q[1] + r2 + s[1]).astype(f32), (C3 + Q[2] + (r1 + r2 + f32(4e-7)) + s[2]).astype(f32)]
    return dict(K=K, A=[q["A" + c] for c in "123"], B=[q["B" + c] for c in "123"], bminx=np.where(q["live"], q["bminx"], f32(3e38)),
                bmaxx=np.where(q["live"], q["bmaxx"], f32(-3e38)), bminy=q["bminy"], bmaxy=q["bmaxy"])


def block_mask_affine(o, fx, fy, TX, TY):
    k = [fma32(o["B"][i], fy, fma32(o["A"][i], fx, o["K"][i])) for i in range(3)]
    return block_bits(k, o["A"], o["B"], o["bminx"], o["bmaxx"], o["bminy"], o["bmaxy"], np.ones(len(TX), bool), TX, TY)


def block_cull(v, ia, op, g2, TX, TY):
    """render_group.hip: block_cull, the in-kernel test the masks replace (kept as the kernels' second instantiation): one quadrant at a time."""
    E = support_scale(op, g2)
    out = np.zeros(len(v), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for qi in range(4):
            OX, OY = TX + f32(8 * (qi & 1)), TY + f32(8 * (qi >> 1))
            u1x, u1y, u2x, u2y, u3x, u3y = [(v[:, i] - (OX if i % 2 == 0 else OY)).astype(f32) for i in range(6)]
            C1 = (u2x * u3y - u2y * u3x) * ia; A1 = (v[:, 3] - v[:, 5]) * ia; B1 = (v[:, 4] - v[:, 2]) * ia
            C2 = (u3x * u1y - u3y * u1x) * ia; A2 = (v[:, 5] - v[:, 1]) * ia; B2 = (v[:, 0] - v[:, 4]) * ia
            A3 = -A1 - A2; B3 = -B1 - B2; C3 = f32(1.0) - C1 - C2
            cx = (u1x + u2x + u3x) * f32(1.0 / 3.0); cy = (u1y + u2y + u3y) * f32(1.0 / 3.0)
            ex = np.stack([E * (u1x - cx), E * (u2x - cx), E * (u3x - cx)]); ey = np.stack([E * (u1y - cy), E * (u2y - cy), E * (u3y - cy)])
            pad = f32(0.05)
            bminx, bmaxx, bminy, bmaxy = cx + ex.min(0) - pad, cx + ex.max(0) + pad, cy + ey.min(0) - pad, cy + ey.max(0) + pad
            live = E > 0
            xs = [live & (bminx <= 3) & (bmaxx >= 0), live & (bminx <= 7) & (bmaxx >= 4)]
            ys = [(bminy <= 3) & (bmaxy >= 0), (bminy <= 7) & (bmaxy >= 4)]
            m = (f32(1.0) - E) * f32(1.0 / 3.0)
            kk = [(C + np.maximum(f32(0), f32(3) * A) + np.maximum(f32(0), f32(3) * B) - m + f32(1e-6) * (np.abs(C) + f32(7) * (np.abs(A) + np.abs(B)))).astype(f32)
                  for A, B, C in ((A1, B1, C1), (A2, B2, C2), (A3, B3, C3))]
            AB = ((A1, B1), (A2, B2), (A3, B3))
            for g in range(4):
                gx, gy = g & 1, g >> 1
                ok = xs[gx] & ys[gy]
                for e in range(3):
                    ok &= (kk[e] + (f32(4) * AB[e][0] if gx else 0) + (f32(4) * AB[e][1] if gy else 0)) >= 0
                out |= ok.astype(np.int64) << (4 * qi + g)
    return out


def pixel_hits_blocks(v, ia, op, g2, TX, TY, dtype):
    """Mask of the blocks in which the per-pixel test accepts a pixel, evaluated like render_group.hip (vertices relative to the QUADRANT's origin,
    then the pixel; barycentrics; ecc in [0, 10] and alpha >= 1/255)."""
    out = np.zeros(len(v), np.int64)
    lx, ly = np.meshgrid(np.arange(8), np.arange(8))
    lx, ly = lx.ravel(), ly.ravel()
    grp = (ly >> 2) * 2 + (lx >> 2)
    lxf, lyf = lx.astype(dtype), ly.astype(dtype)
    for qi in range(4):
        OX, OY = (TX + 8 * (qi & 1)).astype(dtype), (TY + 8 * (qi >> 1)).astype(dtype)
        u = [(v[:, i].astype(dtype) - (OX if i % 2 == 0 else OY)).astype(dtype) for i in range(6)]
        p = [(u[i][:, None] - (lxf if i % 2 == 0 else lyf)[None, :]).astype(dtype) for i in range(6)]
        iad = ia.astype(dtype)[:, None]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            a1 = ((p[2] * p[5] - p[3] * p[4]) * iad).astype(dtype); a2 = ((p[4] * p[1] - p[5] * p[0]) * iad).astype(dtype)
            a3 = (1 - a1 - a2).astype(dtype)
            ecc = (1 - 3 * np.minimum(np.minimum(a1, a2), a3)).astype(dtype)
            pw = np.power(np.maximum(ecc, 0), g2.astype(dtype)[:, None]).astype(dtype)
            alpha = np.minimum(0.99, op.astype(dtype)[:, None] * np.exp2(pw * dtype(-0.7213475204444817))).astype(dtype)
            h = (ecc >= 0) & (ecc <= 10) & (alpha >= dtype(1.0 / 255.0))
        for g in range(4):
            out |= h[:, grp == g].any(1).astype(np.int64) << (4 * qi + g)
    return out


def popcount16(m):
    return sum(((m >> b) & 1) for b in range(16)).sum()


def population(n, rng):
    """qmask_model.main's population."""
    c = rng.uniform(-40, 1960, (n, 2))
    size = np.exp(rng.uniform(np.log(0.2), np.log(600), n))
    ang = rng.uniform(0, 2 * np.pi, (n, 3))
    rad = size[:, None] * rng.uniform(0.05, 1.0, (n, 3))
    sliver = rng.random(n) < 0.3  # nearly collinear vertices
    ang[sliver, 1] = ang[sliver, 0] + np.pi + rng.normal(0, 1e-3, sliver.sum()); ang[sliver, 2] = ang[sliver, 0] + rng.normal(0, 1e-3, sliver.sum())
    v = np.zeros((n, 6))
    for k in range(3):
        v[:, 2 * k] = c[:, 0] + rad[:, k] * np.cos(ang[:, k]); v[:, 2 * k + 1] = c[:, 1] + rad[:, k] * np.sin(ang[:, k])
    v = v.astype(f32)
    op = np.where(rng.random(n) < 0.2, rng.uniform(0.0035, 0.0045, n), rng.uniform(0.0, 1.0, n)).astype(f32)
    op[rng.random(n) < 0.05] = 1.0
    g2 = (2 * rng.choice([0.5, 1.0, 1.0, 2.0, 8.0, 50.0], n)).astype(f32)
    return c, size, v, op, g2


def run(n, seed):
    """Returns the counts as a dict: blocks flagged per form, blocks with a hit, blocks with a hit that a form left unflagged."""
    rng = np.random.default_rng(seed)
    c, size, v, op, g2 = population(n, rng)
    E = support_scale(op, g2)
    q = quad_setup(v, E)
    q["E"] = E
    Q = block_offsets(q)
    area_ok = np.abs(1.0 / q["ia"].astype(np.float64)) >= 1e-8
    cxi, cyi = np.floor(c[:, 0] / 16), np.floor(c[:, 1] / 16)
    reach = np.ceil(np.minimum(size * 3.0, np.where(size > 100, 310, 80)) / 16).astype(int) + 1
    TX0 = ((cxi - reach) * 16).astype(f32); TY0 = ((cyi - reach) * 16).astype(f32)
    ext = (2 * reach * 16).astype(f32)
    anchor = block_anchor(q, Q, TX0, TY0, ext, ext)
    r = dict(triangles=n, instances=0, hit_blocks=0, flagged_per_tile=0, flagged_affine=0, flagged_block_cull=0,
             missed32_per_tile=0, missed64_per_tile=0, missed32_affine=0, missed64_affine=0, missed32_block_cull=0, first_miss=None)
    R = int(reach.max())
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sel = (np.abs(dx) <= reach) & (np.abs(dy) <= reach) & area_ok
            if not sel.any():
                continue
            idx = np.nonzero(sel)[0]
            TX = ((cxi[idx] + dx) * 16).astype(f32); TY = ((cyi[idx] + dy) * 16).astype(f32)
            sub = {k_: (val[idx] if isinstance(val, np.ndarray) else val) for k_, val in q.items()}
            m = block_mask(sub, [x[idx] for x in Q], TX, TY)
            suba = {k_: ([x[idx] for x in val] if isinstance(val, list) else val[idx]) for k_, val in anchor.items()}
            ma = block_mask_affine(suba, (TX - TX0[idx]).astype(f32), (TY - TY0[idx]).astype(f32), TX, TY)
            mc = block_cull(v[idx], q["ia"][idx], op[idx], g2[idx], TX, TY)
            h32 = pixel_hits_blocks(v[idx], q["ia"][idx], op[idx], g2[idx], TX, TY, np.float32)
            h64 = pixel_hits_blocks(v[idx], q["ia"][idx], op[idx], g2[idx], TX, TY, np.float64)
            bad = (h32 & ~m) | (h32 & ~ma)
            if bad.any() and r["first_miss"] is None:
                j = np.nonzero(bad)[0][0]
                r["first_miss"] = (v[idx[j]].tolist(), float(op[idx[j]]), float(g2[idx[j]]), float(TX[j]), float(TY[j]), hex(int(m[j])), hex(int(ma[j])), hex(int(h32[j])))
            r["instances"] += len(idx)
            r["hit_blocks"] += int(popcount16(h32 | h64))
            r["flagged_per_tile"] += int(popcount16(m)); r["flagged_affine"] += int(popcount16(ma)); r["flagged_block_cull"] += int(popcount16(mc))
            r["missed32_per_tile"] += int(popcount16(h32 & ~m)); r["missed64_per_tile"] += int(popcount16(h64 & ~m))
            r["missed32_affine"] += int(popcount16(h32 & ~ma)); r["missed64_affine"] += int(popcount16(h64 & ~ma))
            r["missed32_block_cull"] += int(popcount16(h32 & ~mc))
    return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    r = run(n, seed)
    print(f"triangles {n} seed {seed}: instances {r['instances']}, blocks with a hit {r['hit_blocks']}")
    for form in ("per_tile", "affine"):
        f = r["flagged_" + form]
        print(f"block masks, {form}: blocks flagged {f} (tightness {r['hit_blocks'] / max(f, 1):.3f}, {f / max(r['flagged_block_cull'], 1):.4f} x block_cull's); "
              f"missed fp32 {r['missed32_' + form]}, fp64 {r['missed64_' + form]}")
    print(f"in-kernel block_cull: blocks flagged {r['flagged_block_cull']} (tightness {r['hit_blocks'] / max(r['flagged_block_cull'], 1):.3f}); missed fp32 {r['missed32_block_cull']}")
    if r["first_miss"]:
        print("first miss:", r["first_miss"])
    return 1 if (r["missed32_per_tile"] or r["missed32_affine"]) else 0


if __name__ == "__main__":
    sys.exit(main())
