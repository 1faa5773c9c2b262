"""numpy reference of include/ts_atlas.h, operation by operation: the texels of a face, the texel of a pixel, the atlas placement and its
inverse, the UVs, the face totals, the resolve and the draw.  Everything that is not an integer is float64 on fp32 inputs widened, every
operation rounded (numpy float64 arrays never contract).

The barycentrics are ref_color_volume.interpolate's.  That function returns them rounded to fp32 only, and the texel needs them in float64
(floor(beta R) of the rounded value can be the next texel), so `barycentrics` below carries the same operations in float64 and every call
HOLDS ITS RESULT AGAINST ref_color_volume.interpolate: the same drawn pixels, and fp32(alpha, beta, gamma) equal to its `bary` bit for bit.
The accumulator is ref_mesh_census.census_add (np.add.at on int64) with the texel index as its key image: the Q16 and mask rules are not
restated here."""
from __future__ import annotations

import numpy as np

import ref_color_volume as cref
import ref_mesh_census as census

INT32_MAX = 2 ** 31 - 1
MAX_RES = 64


# ---- texels and the atlas: integers ---------------------------------------------------------------------------------------------------------
def texels_per_face(R):
    return R * (R + 1) // 2


def compact_index(f, i, j, R):
    """n = f T + j R - j (j - 1) / 2 + i (arrays or ints)."""
    return f * texels_per_face(R) + j * R - j * (j - 1) // 2 + i


def face_texels(R):
    """(T, 2) int64: (i, j) of a face's texels in the order of their compact index."""
    return np.array([(i, j) for j in range(R) for i in range(R - j)], np.int64).reshape(-1, 2)


def default_cells_per_row(F, R):
    """The smallest Cx >= 1 with Cx Cx (R + 1) >= K R, by counting up."""
    K = (F + 1) // 2
    Cx = 1
    while Cx * Cx * (R + 1) < K * R:
        Cx += 1
    return Cx


def layout(F, R, Cx=None):
    """(R, T, Cx, Cy, Wa, Ha)."""
    assert F >= 0 and 1 <= R <= MAX_RES
    K = (F + 1) // 2
    Cx = default_cells_per_row(F, R) if Cx is None else Cx
    assert Cx >= 1
    Cy = max(1, -(-K // Cx))
    return R, texels_per_face(R), Cx, Cy, Cx * (R + 1), Cy * R


def texel_position(f, i, j, R, Cx):
    """(x, y) of texel (f, i, j) in the atlas (arrays or ints)."""
    f, i, j = (np.asarray(a, np.int64) for a in (f, i, j))
    k = f // 2
    X0, Y0 = (k % Cx) * (R + 1), (k // Cx) * R
    upper = f % 2 == 1
    return np.where(upper, X0 + R - i, X0 + i), np.where(upper, Y0 + R - 1 - j, Y0 + j)


def invert_position(x, y, R, Cx):
    """(f, i, j) of atlas texel (x, y), by the lx + ly <= R - 1 test; f may be >= F."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    lx, ly = x % (R + 1), y % R
    k = (y // R) * Cx + x // (R + 1)
    lower = lx + ly <= R - 1
    return np.where(lower, 2 * k, 2 * k + 1), np.where(lower, lx, R - lx), np.where(lower, ly, R - 1 - ly)


def face_uvs(F, R, Cx, Cy):
    """(F, 3, 2) float32: the corners (a, b, c) in texel units over (Wa, Ha), one division in float64, one rounding to fp32."""
    Wa, Ha = Cx * (R + 1), Cy * R
    uv = np.zeros((F, 3, 2), np.float32)
    for f in range(F):
        k = f // 2
        X0, Y0 = (k % Cx) * (R + 1), (k // Cx) * R
        corners = ((X0 + R + 1, Y0 + R), (X0 + 1, Y0 + R), (X0 + R + 1, Y0)) if f % 2 else ((X0, Y0), (X0 + R, Y0), (X0, Y0 + R))
        for m, (x, y) in enumerate(corners):
            uv[f, m] = (np.float32(np.float64(x) / np.float64(Wa)), np.float32(np.float64(y) / np.float64(Ha)))
    return uv


# ---- the texel of a pixel -------------------------------------------------------------------------------------------------------------------
def barycentrics(view, tan_fovx, tan_fovy, W, H, vertices, faces, face_idx):
    """(drawn (H W,) bool, alpha, beta, gamma (H W,) float64): the operations of ts_color.h's interpolation, checked against
    ref_color_volume.interpolate on every call (see the module text)."""
    M = np.asarray(view, np.float32).astype(np.float64).reshape(4, 4)
    tx, ty = float(np.float32(tan_fovx)), float(np.float32(tan_fovy))
    P = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    Fc = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    V, F = len(P), len(Fc)
    fi = np.asarray(face_idx, np.int32).reshape(-1).astype(np.int64)
    drawn = (fi >= 0) & (fi < F)
    tri = Fc[np.where(drawn, fi, 0)] if F else np.zeros((len(fi), 3), np.int64)
    drawn &= ((tri >= 0) & (tri < V)).all(axis=1)
    tri = np.where(drawn[:, None], tri, 0)
    if V == 0:
        P = np.zeros((1, 3))
    p = np.arange(W * H)
    col, row = (p % W).astype(np.float64), (p // W).astype(np.float64)
    with np.errstate(all="ignore"):
        corner = []
        for m in range(3):
            q = P[tri[:, m]]
            corner.append([((q[:, 0] * M[0, k] + q[:, 1] * M[1, k]) + q[:, 2] * M[2, k]) + M[3, k] for k in range(3)])
        a, b, c = corner
        r0 = ((col + 0.5) / (0.5 * W) - 1.0) * tx
        r1 = ((row + 0.5) / (0.5 * H) - 1.0) * ty

        def rdc(x, y):
            n0, n1, n2 = x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]
            return (r0 * n0 + r1 * n1) + n2

        wa, wb, wc = rdc(b, c), rdc(c, a), rdc(a, b)
        neg = (wa + wb) + wc < 0
        wa, wb, wc = (np.where(neg, -w, w) for w in (wa, wb, wc))
        wa, wb, wc = (np.where(w >= 0, w, 0.0) for w in (wa, wb, wc))
        s = (wa + wb) + wc
        good = np.isfinite(s) & (s > 0)
        al, be, ga = (np.where(good, w / np.where(good, s, 1.0), 1.0 / 3.0) for w in (wa, wb, wc))
    # the yardstick: ref_color_volume's own interpolation of no attribute at all
    _, bary32 = cref.interpolate(view, tan_fovx, tan_fovy, W, H, np.asarray(vertices, np.float32).reshape(-1, 3), faces, face_idx,
                                 np.zeros((V, 1), np.float32), np.zeros(1, np.float32))
    mine = np.stack([np.where(drawn, w.astype(np.float32), np.float32(0)) for w in (al, be, ga)]).astype(np.float32)
    assert np.array_equal(mine.view(np.uint32), bary32.reshape(3, -1).view(np.uint32)), "ref_mesh_texture.barycentrics left ref_color_volume.interpolate"
    return drawn, al, be, ga


def texel_index(view, tan_fovx, tan_fovy, W, H, vertices, faces, face_idx, R, Cx):
    """(texel_idx (H, W) int32, atlas_idx (H, W) int32, bary (3, H, W) float32)."""
    drawn, al, be, ga = barycentrics(view, tan_fovx, tan_fovy, W, H, vertices, faces, face_idx)
    F = len(np.asarray(faces).reshape(-1, 3))
    _, T, Cx, Cy, Wa, Ha = layout(F, R, Cx)
    assert F * T <= INT32_MAX and Wa * Ha <= INT32_MAX
    f = np.where(drawn, np.asarray(face_idx, np.int32).reshape(-1).astype(np.int64), 0)
    i = np.minimum(np.floor(be * np.float64(R)).astype(np.int64), R - 1)
    j = np.minimum(np.floor(ga * np.float64(R)).astype(np.int64), R - 1 - i)
    n = compact_index(f, i, j, R)
    x, y = texel_position(f, i, j, R, Cx)
    texel = np.where(drawn, n, -1).astype(np.int32)
    atlas = np.where(drawn, y * Wa + x, -1).astype(np.int32)
    bary = np.stack([np.where(drawn, w.astype(np.float32), np.float32(0)) for w in (al, be, ga)]).astype(np.float32)
    return texel.reshape(H, W), atlas.reshape(H, W), bary.reshape(3, H, W)


# ---- accumulator, totals, resolve, draw -----------------------------------------------------------------------------------------------------------
def accumulate(texels, texel_idx, target=None, pixel_mask=None):
    """One view into `texels` ((F T, 4) int64) in place: ref_mesh_census.census_add with the texel as the key."""
    return census.census_add(texels, texel_idx, target, pixel_mask)


def face_totals(texels, F, R):
    """(F, 4) int64: the integer sum of every face's T rows."""
    return texels.reshape(F, texels_per_face(R), 4).sum(axis=1, dtype=np.int64)


def to_byte(c):
    """(uint8) rint(min(max(c, 0), 1) 255) in double; a NaN gives 0."""
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        lo = np.where(c > 0, c, 0.0)
        return np.rint(np.where(lo < 1.0, lo, 1.0) * 255.0).astype(np.uint8)


def resolve(texels, F, R, Cx, Cy, min_count=1, face_fallback=None, fill=(0.5, 0.5, 0.5)):
    """(image (3, Ha, Wa) float32, state (Ha, Wa) uint8, rgb8 (Ha, Wa, 3) uint8)."""
    assert min_count >= 1 and Cx * Cy >= (F + 1) // 2
    Wa, Ha = Cx * (R + 1), Cy * R
    T = texels_per_face(R)
    totals = face_totals(texels, F, R) if F else np.zeros((0, 4), np.int64)
    y, x = np.divmod(np.arange(Wa * Ha, dtype=np.int64), Wa)
    f, i, j = invert_position(x, y, R, Cx)
    exists = f < F
    fs = np.where(exists, f, 0)
    n = np.where(exists, compact_index(fs, i, j, R), 0)
    rows = texels[n] if F else np.zeros((Wa * Ha, 4), np.int64)
    face_rows = totals[fs] if F else np.zeros((Wa * Ha, 4), np.int64)
    own = exists & (rows[:, 0] >= min_count)
    face = exists & ~own & (face_rows[:, 0] >= 1)
    fall = exists & ~own & ~face & (face_fallback is not None)
    image = np.empty((3, Wa * Ha), np.float32)
    with np.errstate(all="ignore"):
        for c in range(3):
            own_mean = (rows[:, 1 + c].astype(np.float64) / (rows[:, 0].astype(np.float64) * 65536.0)).astype(np.float32)
            face_mean = (face_rows[:, 1 + c].astype(np.float64) / (face_rows[:, 0].astype(np.float64) * 65536.0)).astype(np.float32)
            value = np.full(Wa * Ha, np.float32(fill[c]), np.float32)
            if face_fallback is not None and F:
                value = np.where(fall, np.asarray(face_fallback, np.float32).reshape(F, 3)[fs, c], value)
            value = np.where(face, face_mean, value)
            image[c] = np.where(own, own_mean, value)
    state = np.where(own, 3, np.where(face, 2, np.where(fall, 1, 0))).astype(np.uint8)
    rgb8 = np.ascontiguousarray(to_byte(image).T)
    return image.reshape(3, Ha, Wa), state.reshape(Ha, Wa), rgb8.reshape(Ha, Wa, 3)


def render(atlas_idx, image, background):
    """(3, H, W) float32: image[ch, atlas_idx] where the index lies in [0, Wa Ha), background[ch] elsewhere.  Nothing is clamped."""
    a = np.asarray(atlas_idx, np.int32).astype(np.int64)
    flat = np.asarray(image, np.float32).reshape(3, -1)
    ok = (a >= 0) & (a < flat.shape[1])
    bg = np.asarray(background, np.float32).reshape(3)
    return np.stack([np.where(ok, flat[ch][np.where(ok, a, 0)], bg[ch]) for ch in range(3)]).astype(np.float32)


# ---- PNG: a reader for the writer's test ----------------------------------------------------------------------------------------------------------
def read_png_rgb8(data):
    """(H, W, 3) uint8 of a PNG with colour type 2, 8 bits and filter 0 on every row; checks the signature, every CRC and the chunk order."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, chunks = 8, []
    while off < len(data):
        (n,) = struct.unpack_from(">I", data, off)
        kind, body = data[off + 4:off + 8], data[off + 8:off + 8 + n]
        (crc,) = struct.unpack_from(">I", data, off + 8 + n)
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        off += 12 + n
    assert off == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3).copy()
