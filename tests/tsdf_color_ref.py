"""The numpy statement of colour in `ops.tsdf_fragment(..., color=)` and `ops.tsdf_mesh(..., rgb_sum=)` (include/dgr_hip.h at
dgr_tsdf_fragment_rgb), built on tests/tsdf_ref.py: the same integration loop with the three integer colour
sums of a voxel added, and `tsdf_points`' edge selection with the colour of a point added.  The colour formula is float64,
every step one correctly rounded operation in the order written, so the GPU result is compared with it bit for bit.  A
mesh's vertices are the fragment's points in the same order (tests/tsdf_mesh_ref.py), so their colours are `tsdf_colors`."""
import numpy as np

import tsdf_ref

MAX_FRAMES = 8421504   # DGR_TSDF_COLOR_MAX_FRAMES: 255 F fits an int32


def tsdf_integrate(blocks, depth, color, intrinsic, extrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc, block):
    """(tsdf float32 [nb,B^3], weight int32 [nb,B^3], rgb_sum int32 [nb,B^3,3]) after the frames 0..F-1 in order:
    `tsdf_ref.tsdf_integrate`'s loop, and wherever it updates a voxel from pixel (u, v) of frame f, rgb_sum += color[f, v, u]."""
    fx, fy, cx, cy = (np.float64(v) for v in intrinsic)
    F, H, W = depth.shape
    B, nb = block, len(blocks)
    i = (blocks.astype(np.int64)[:, None, :] * B + tsdf_ref._local(B)[None]).reshape(-1, 3)
    pw = (i.astype(np.float64) + 0.5) * np.float64(voxel_length)
    x, y, z = pw[:, 0], pw[:, 1], pw[:, 2]
    tsdf = np.zeros(len(pw), np.float32)
    weight = np.zeros(len(pw), np.int32)
    rgb = np.zeros((len(pw), 3), np.int32)
    E = np.asarray(extrinsic, np.float64)
    for f in range(F):
        pcx, pcy, pcz = tsdf_ref._rigid(E[f], x, y, z)
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
        sel, u, v, sdf = sel[ok], u[ok], v[ok], sdf[ok]
        val = np.minimum(1.0, sdf / np.float64(sdf_trunc))
        w = weight[sel].astype(np.float64)
        tsdf[sel] = ((tsdf[sel].astype(np.float64) * w + val) / (w + 1.0)).astype(np.float32)
        weight[sel] += 1
        rgb[sel] += color[f, v, u].astype(np.int32)
    return tsdf.reshape(nb, B ** 3), weight.reshape(nb, B ** 3), rgb.reshape(nb, B ** 3, 3)


def neighbour_index(blocks, block):
    """int64 [nb,B,B,B,3]: the flat index (block B^3 + l) of every voxel's +a neighbour, -1 where its block is not in the list"""
    B, nb = block, len(blocks)
    index = {tuple(b): k for k, b in enumerate(np.asarray(blocks).tolist())}
    own = np.arange(nb * B ** 3, dtype=np.int64).reshape(nb, B, B, B)     # [block, lz, ly, lx]
    out = np.full((nb, B, B, B, 3), -1, np.int64)
    for a in range(3):
        ax = 3 - a
        inner, shifted, last, first = ([slice(None)] * 4 for _ in range(4))
        inner[ax], shifted[ax], last[ax], first[ax] = slice(0, B - 1), slice(1, B), B - 1, 0
        out[tuple(inner) + (a,)] = own[tuple(shifted)]
        nbr = np.array([index.get((b[0] + (a == 0), b[1] + (a == 1), b[2] + (a == 2)), -1) for b in np.asarray(blocks).tolist()])
        have = nbr >= 0
        first[0], last[0] = nbr[have], np.nonzero(have)[0]
        out[tuple(last) + (a,)] = own[tuple(first)]
    return out


def tsdf_colors(blocks, tsdf, weight, rgb_sum, voxel_length, block, min_weight, return_ends=False):
    """(xyz float64 [P,3], color float64 [P,3]): `tsdf_ref.tsdf_points`' points in its order -- blocks in list order, voxels
    by l, axes 0, 1, 2 -- and their colours: m0 = rgb_sum0 / w0, m1 = rgb_sum1 / w1, c = (m0 + r (m1 - m0)) / 255 with the r
    of the position.  With `return_ends` also int64 [P,2]: the flat indices of the two voxels a point reads."""
    B, nb = block, len(blocks)
    if nb == 0:
        out = (np.zeros((0, 3)), np.zeros((0, 3)))
        return out + (np.zeros((0, 2), np.int64),) if return_ends else out
    T, Wt = np.asarray(tsdf, np.float32).reshape(-1), np.asarray(weight, np.int32).reshape(-1)
    S = np.asarray(rgb_sum, np.int32).reshape(-1, 3)
    i1 = neighbour_index(blocks, B)
    j = np.maximum(i1, 0)
    f0, w0 = T.reshape(nb, B, B, B, 1), Wt.reshape(nb, B, B, B, 1)
    f1, w1 = np.where(i1 >= 0, T[j], np.float32(0)), np.where(i1 >= 0, Wt[j], 0)
    lim = np.float32(0.98)
    emit = (w0 >= min_weight) & (w1 >= min_weight) & (f0 >= -lim) & (f0 < lim) & (f1 >= -lim) & (f1 < lim) \
        & ((f0 < 0) != (f1 < 0))
    k, lz, ly, lx, a = np.nonzero(emit)
    i = np.asarray(blocks, np.int64)[k] * B + np.stack([lx, ly, lz], 1)
    pw = (i.astype(np.float64) + 0.5) * np.float64(voxel_length)
    o0, o1 = (k * B + lz) * B * B + ly * B + lx, i1[emit]
    r0, r1 = np.abs(T[o0].astype(np.float64)), np.abs(T[o1].astype(np.float64))
    r = r0 / (r0 + r1)
    n = np.arange(len(pw))
    pw[n, a] = pw[n, a] + np.float64(voxel_length) * r
    m0 = S[o0].astype(np.float64) / Wt[o0].astype(np.float64)[:, None]
    m1 = S[o1].astype(np.float64) / Wt[o1].astype(np.float64)[:, None]
    c = (m0 + r[:, None] * (m1 - m0)) / 255.0
    return (pw, c, np.stack([o0, o1], 1)) if return_ends else (pw, c)


def tsdf_fragment(depth, color, intrinsic, pose, voxel_length, sdf_trunc, depth_scale=1000.0, depth_trunc=4.5, block=16,
                  stride=4, min_weight=1):
    """dict(xyz, color, blocks, tsdf, weight, rgb_sum, ends) of numpy arrays: the whole statement with colour"""
    depth = np.ascontiguousarray(depth, np.uint16)
    color = np.ascontiguousarray(color, np.uint8)
    assert color.shape == depth.shape + (3,) and len(depth) <= MAX_FRAMES
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 4, 4)
    extrinsic = np.linalg.inv(pose)
    blocks = tsdf_ref.tsdf_blocks(depth, intrinsic, pose, voxel_length, sdf_trunc, depth_scale, depth_trunc, block, stride)
    tsdf, weight, rgb_sum = tsdf_integrate(blocks, depth, color, intrinsic, extrinsic, voxel_length, sdf_trunc, depth_scale,
                                           depth_trunc, block)
    xyz, c, ends = tsdf_colors(blocks, tsdf, weight, rgb_sum, voxel_length, block, min_weight, return_ends=True)
    return {'blocks': blocks, 'tsdf': tsdf, 'weight': weight, 'rgb_sum': rgb_sum, 'xyz': xyz, 'color': c, 'ends': ends}


def noise_color(depth, seed=0):
    """uint8 [F,H,W,3] of seeded noise: a wrong pixel, frame or channel cannot hide in it"""
    return np.random.default_rng(seed).integers(0, 256, tuple(depth.shape) + (3,), np.uint8)
