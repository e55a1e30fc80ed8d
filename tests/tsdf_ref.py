"""The numpy statement of `ops.tsdf_fragment` (include/dgr_hip.h at dgr_tsdf_fragment): every step is one
correctly rounded float64 operation in the order written here, so the GPU result is compared with it bit for bit.
Vectorised over pixels and voxels; `np.unique` supplies the first occurrence of a block."""
import numpy as np

BLOCK_LIMIT = 2 ** 26   # DGR_TSDF_BLOCK_LIMIT: block coordinates lie in [-2^26, 2^26)


def _rigid(M, x, y, z):
    """rows 0..2 of M applied as ((M0 x + M1 y) + M2 z) + M3"""
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def tsdf_blocks(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale, depth_trunc, block, stride):
    """int32 [nb,3]: the distinct blocks the strided pixels touch, in ascending order of their first candidate number
    (((f Hs + vs) Ws + us) 8 + corner); bit a of `corner` selects hi over lo on axis a."""
    fx, fy, cx, cy = (np.float64(v) for v in intrinsic)
    F, H, W = depth.shape
    bl = np.float64(voxel_length) * np.float64(block)
    us = np.arange(0, W, stride, dtype=np.float64)
    vs = np.arange(0, H, stride, dtype=np.float64)
    raw = depth[:, ::stride, ::stride]
    d = raw.astype(np.float64) / np.float64(depth_scale)
    valid = (raw > 0) & (d <= depth_trunc)
    xn = ((us - cx) / fx)[None, None, :]
    yn = ((vs - cy) / fy)[None, :, None]
    P = np.moveaxis(np.asarray(pose, np.float64), 0, 2)[:, :, :, None, None]    # [4,4,F,1,1]: P[r, c] broadcasts over a frame
    pw = _rigid(P, xn * d, yn * d, d)
    lo = [np.floor((p - sdf_trunc) / bl) for p in pw]
    hi = [np.floor((p + sdf_trunc) / bl) for p in pw]
    for a in range(3):
        valid &= (lo[a] >= -BLOCK_LIMIT) & (hi[a] < BLOCK_LIMIT)
    keys = np.zeros(d.shape + (8, 3), np.int64)
    for c in range(8):
        for a in range(3):
            keys[..., c, a] = np.where(valid, hi[a] if (c >> a) & 1 else lo[a], 0)
    keys = keys[valid].reshape(-1, 3)          # candidate order: f, vs, us, corner
    if len(keys) == 0:
        return np.zeros((0, 3), np.int32)
    uniq, first = np.unique(keys, axis=0, return_index=True)
    return uniq[np.argsort(first, kind='stable')].astype(np.int32)


def _local(B):
    l = np.arange(B ** 3)
    return np.stack([l % B, (l // B) % B, l // (B * B)], 1)    # l = (lz B + ly) B + lx


def tsdf_integrate(blocks, depth, intrinsic, extrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc, block,
                   return_updated=False):
    """(tsdf float32 [nb,B^3], weight int32 [nb,B^3]) after the frames 0..F-1 in order.  With `return_updated` also a bool
    [nb,F]: frame f updates at least one voxel of the block (what a run on that frame alone leaves with weight > 0)."""
    fx, fy, cx, cy = (np.float64(v) for v in intrinsic)
    F, H, W = depth.shape
    B, nb = block, len(blocks)
    i = (blocks.astype(np.int64)[:, None, :] * B + _local(B)[None]).reshape(-1, 3)
    pw = (i.astype(np.float64) + 0.5) * np.float64(voxel_length)
    x, y, z = pw[:, 0], pw[:, 1], pw[:, 2]
    tsdf = np.zeros(len(pw), np.float32)
    weight = np.zeros(len(pw), np.int32)
    E = np.asarray(extrinsic, np.float64)
    updated = np.zeros((nb, F), bool)
    for f in range(F):
        pcx, pcy, pcz = _rigid(E[f], x, y, z)
        sel = np.nonzero(pcz > 0)[0]
        uf = ((fx * pcx[sel]) / pcz[sel] + cx) + 0.5
        vf = ((fy * pcy[sel]) / pcz[sel] + cy) + 0.5
        ok = (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        sel, u, v = sel[ok], uf[ok].astype(np.int64), vf[ok].astype(np.int64)
        raw = depth[f, v, u]
        d = raw.astype(np.float64) / np.float64(depth_scale)
        ok = (raw > 0) & (d <= depth_trunc)
        sel, u, v, d = sel[ok], u[ok], v[ok], d[ok]
        xn = (u.astype(np.float64) - cx) / fx
        yn = (v.astype(np.float64) - cy) / fy
        m = np.sqrt((1.0 + xn * xn) + yn * yn)
        sdf = (d - pcz[sel]) * m
        ok = sdf > -sdf_trunc
        sel, sdf = sel[ok], sdf[ok]
        val = np.minimum(1.0, sdf / np.float64(sdf_trunc))
        w = weight[sel].astype(np.float64)
        tsdf[sel] = ((tsdf[sel].astype(np.float64) * w + val) / (w + 1.0)).astype(np.float32)
        weight[sel] += 1
        updated[sel // B ** 3, f] = True
    if return_updated:
        return tsdf.reshape(nb, B ** 3), weight.reshape(nb, B ** 3), updated
    return tsdf.reshape(nb, B ** 3), weight.reshape(nb, B ** 3)


def cull_keeps(blocks, intrinsic, extrinsic, height, width, voxel_length, sdf_trunc, depth_trunc, block, row_norm=True):
    """bool [nb,F]: the per-frame block cull of `ts_integrate` (csrc/tsdf.hip) restated -- a frame is kept for a block unless
    the ball of radius sqrt(3)/2 bl around the block's centre, stretched by max(1, the largest row norm of the extrinsic's
    3x3 part), lies outside one of the six half-spaces an update needs.  `row_norm=False` leaves the stretch out: the rule
    before it was made conservative for poses that are not rigid.  An instrument for the tests' premises (what would the
    suite see if the rule were wrong?), NOT a second definition of the result: the cull never reaches the result."""
    fx, fy, cx, cy = (np.float64(v) for v in intrinsic)
    bl = np.float64(voxel_length) * np.float64(block)
    c = (np.asarray(blocks, np.float64) + 0.5) * bl                              # [nb,3]
    E = np.asarray(extrinsic, np.float64).reshape(-1, 4, 4)[:, :3]                # [F,3,4]
    rad = 0.8660254037844387 * bl
    margin = (rad * 1.01 + 1e-6 + 1e-9 * np.abs(c).sum(1))[:, None]              # [nb,1]
    p = np.einsum('frk,bk->rbf', E[:, :, :3], c) + E[:, :, 3].T[:, None, :]      # [3,nb,F]
    px, py, pz = p
    stretch = np.maximum(1.0, np.sqrt((E[:, :, :3] ** 2).sum(2).max(1)))[None, :] if row_norm else 1.0
    mg = margin * stretch + 1e-9 * np.abs(p).sum(0)
    l, r, t, b = cx + 0.5, width - cx - 0.5, cy + 0.5, height - cy - 0.5
    keep = (pz > -mg) & (pz - mg < depth_trunc + sdf_trunc) \
        & (fx * px + l * pz >= -mg * (fx + abs(l))) & (fx * px - r * pz <= mg * (fx + abs(r))) \
        & (fy * py + t * pz >= -mg * (fy + abs(t))) & (fy * py - b * pz <= mg * (fy + abs(b)))
    return keep | ~(np.abs(p).sum(0) < 1e300)


def tsdf_points(blocks, tsdf, weight, voxel_length, block, min_weight, return_cross=False):
    """float64 [P,3]: the zero crossings on the +x, +y, +z edges of every voxel, blocks in list order, voxels by l, axes
    0, 1, 2.  With `return_cross` also a bool [P]: the edge's far end lies in another block."""
    B, nb = block, len(blocks)
    if nb == 0:
        return (np.zeros((0, 3)), np.zeros(0, bool)) if return_cross else np.zeros((0, 3))
    index = {tuple(b): k for k, b in enumerate(blocks.tolist())}
    T = tsdf.reshape(nb, B, B, B)      # [block, lz, ly, lx]
    Wt = weight.reshape(nb, B, B, B)
    f1 = np.zeros((nb, B, B, B, 3), np.float32)
    w1 = np.zeros((nb, B, B, B, 3), np.int32)
    cross = np.zeros((nb, B, B, B, 3), bool)
    for a in range(3):
        ax = 3 - a                      # array axis of coordinate a
        nbr = np.array([index.get((b[0] + (a == 0), b[1] + (a == 1), b[2] + (a == 2)), -1) for b in blocks.tolist()])
        have = nbr >= 0
        inner = [slice(None)] * 4
        inner[ax] = slice(0, B - 1)
        shifted = [slice(None)] * 4
        shifted[ax] = slice(1, B)
        f1[tuple(inner) + (a,)] = T[tuple(shifted)]
        w1[tuple(inner) + (a,)] = Wt[tuple(shifted)]
        last = [slice(None)] * 4
        last[ax] = B - 1
        first = [slice(None)] * 4
        first[ax] = 0
        first[0] = nbr[have]
        dst = list(last)
        dst[0] = np.nonzero(have)[0]
        f1[tuple(dst) + (a,)] = T[tuple(first)]
        w1[tuple(dst) + (a,)] = Wt[tuple(first)]
        cross[tuple(last) + (a,)] = True
    f0 = T[..., None]
    w0 = Wt[..., None]
    lim = np.float32(0.98)
    emit = (w0 >= min_weight) & (w1 >= min_weight) & (f0 >= -lim) & (f0 < lim) & (f1 >= -lim) & (f1 < lim) \
        & ((f0 < 0) != (f1 < 0))
    k, lz, ly, lx, a = np.nonzero(emit)
    i = blocks.astype(np.int64)[k] * B + np.stack([lx, ly, lz], 1)
    pw = (i.astype(np.float64) + 0.5) * np.float64(voxel_length)
    r0 = np.abs(np.broadcast_to(f0, emit.shape)[emit].astype(np.float64))
    r1 = np.abs(f1[emit].astype(np.float64))
    n = np.arange(len(pw))
    pw[n, a] = pw[n, a] + np.float64(voxel_length) * (r0 / (r0 + r1))
    return (pw, cross[emit]) if return_cross else pw


def tsdf_fragment(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale=1000.0, depth_trunc=4.5, block=16, stride=4,
                  min_weight=1, return_cross=False, return_updated=False):
    """dict(xyz, blocks, tsdf, weight[, cross][, updated]) of numpy arrays: the whole statement.  extrinsic = inv(pose) is taken on
    the host exactly as the wrapper takes it; the statement itself never inverts."""
    depth = np.ascontiguousarray(depth, np.uint16)
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 4, 4)
    extrinsic = np.linalg.inv(pose)
    blocks = tsdf_blocks(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale, depth_trunc, block, stride)
    tsdf, weight, updated = tsdf_integrate(blocks, depth, intrinsic, extrinsic, voxel_length, sdf_trunc, depth_scale,
                                           depth_trunc, block, return_updated=True)
    out = {'blocks': blocks, 'tsdf': tsdf, 'weight': weight}
    if return_updated:
        out['updated'] = updated
    if return_cross:
        out['xyz'], out['cross'] = tsdf_points(blocks, tsdf, weight, voxel_length, block, min_weight, True)
    else:
        out['xyz'] = tsdf_points(blocks, tsdf, weight, voxel_length, block, min_weight)
    return out
