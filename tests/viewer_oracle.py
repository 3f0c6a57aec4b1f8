"""numpy restatement of the point-splat renderer (csrc/nid_splat_kernels.hpp: k_splat_depth, k_splat_resolve) -- TEST
INFRASTRUCTURE ONLY.  The projection is the CPU oracle's (oracle_lib.project, as tests/test_image_edges.py takes it); the camera-frame
point, the FoV gate, the truncating cast and the in-image test are written out in the kernel's association order; the depth is
``sq.astype(np.float32)``; the keys go through a Python loop over the splat's offsets; the blend is integer.  Nothing here is
tolerant: the GPU image and index image must equal these arrays."""
import numpy as np

import oracle_lib

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def point_to_pixel(model, intr, dist, pts, T, W, H, min_nz):
    """``(q, sq)``: pixel index ``py * W + px`` or -1 per point, and the fp64 squared camera-frame distance
    (nid_render_kernels.hpp point_to_pixel: products summed left to right, gate on the normalised 3-vector)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    n = len(pts)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0)
    m = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z, w = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    with np.errstate(all="ignore"):
        c = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] * w for r in range(3)]
        sq = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        zn = np.where(sq > 0.0, c[2] / np.sqrt(np.where(sq > 0.0, sq, 1.0)), c[2])
        gate = ~(zn < min_nz)
        uv = oracle_lib.project(model, intr, dist, np.stack(c, axis=1))
        u, v = uv[:, 0], uv[:, 1]
        inside = gate & (u > -1.0) & (u < float(W)) & (v > -1.0) & (v < float(H))
        ui = np.where(inside, u, 0.0).astype(np.int64)  # truncation toward zero: (-1, 0) belongs to pixel 0
        vi = np.where(inside, v, 0.0).astype(np.int64)
    return np.where(inside, vi * W + ui, -1), sq


def splat_keys(q, sq, W, H, radius):
    """The key buffer after k_splat_depth: per pixel the minimum of (bits(float32(sq)) << 32) | (0xFFFFFFFF - i) over the points
    whose (2 radius + 1)^2 square covers it; EMPTY where there is none."""
    zkey = np.full(W * H, EMPTY, dtype=np.uint64)
    with np.errstate(all="ignore"):
        d = np.asarray(sq, dtype=np.float64).astype(np.float32)
    ok = (q >= 0) & np.isfinite(d)
    i = np.nonzero(ok)[0]
    key = (d[i].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - i.astype(np.uint64))
    px, py = q[i] % W, q[i] // W
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            xx, yy = px + dx, py + dy
            inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.minimum.at(zkey, (yy * W + xx)[inb], key[inb])
    return zkey


def resolve(zkey, W, H, rgba, background, alpha):
    """k_splat_resolve: ``(rgb uint8 (H, W, 3), index int32 (H, W))``"""
    hit = zkey != EMPTY
    index = np.where(hit, np.int64(0xFFFFFFFF) - (zkey & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    out = np.zeros((W * H, 3), dtype=np.int64) if background is None else np.asarray(background, dtype=np.uint8).reshape(H * W, 3).astype(np.int64)
    if hit.any():
        c = np.asarray(rgba, dtype=np.uint8).reshape(-1, 4).astype(np.int64)[index[hit]]
        a = (int(alpha) * c[:, 3] + 127) // 255
        out[hit] = (out[hit] * (255 - a)[:, None] + c[:, :3] * a[:, None] + 127) // 255
    return out.astype(np.uint8).reshape(H, W, 3), index.astype(np.int32).reshape(H, W)


def draw(model, intr, dist, pts, rgba, T, W, H, min_nz, radius=1, background=None, alpha=255):
    q, sq = point_to_pixel(model, intr, dist, pts, T, W, H, min_nz)
    return resolve(splat_keys(q, sq, W, H, radius), W, H, rgba, background, alpha)
