"""Seeded synthetic inputs and weights for tests and `bench.py`.

There is no dataset and no released checkpoint offline, so the harness uses
3DMatch-/KITTI-shaped synthetic pairs and a seeded state_dict in the
reference's checkpoint layout (`core/trainer.py:527-549`; MinkowskiEngine key
names `conv1.kernel [K,Cin,Cout]`, `norm1.bn.*`, `block1.conv1.kernel`, ...,
`final.kernel`, `final.bias [1,Cout]`).  numpy only; no torch, no HIP.
"""
import numpy as np

CHANNELS = [None, 32, 64, 128, 256]      # model/resunet.py:664 (ResUNetBN2C)
TR_CHANNELS = [None, 64, 64, 64, 128]    # model/resunet.py:665


# ----------------------------------------------------------------------------
# point clouds
# ----------------------------------------------------------------------------
def _random_rotation(rng, max_angle_deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rng.uniform(0, max_angle_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _sample_box_surface(rng, n, lo, hi):
    """n points area-uniformly on the 6 faces of the axis-aligned box [lo,hi]."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    s = hi - lo
    areas = np.array([s[1] * s[2], s[1] * s[2], s[0] * s[2], s[0] * s[2], s[0] * s[1], s[0] * s[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = lo + rng.random((n, 3)) * s
    axis = face // 2
    side = face % 2
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def _indoor_scene(rng, n):
    room = np.array([4.0, 3.5, 2.6])
    boxes = [(np.zeros(3), room, 1.0)]
    for _ in range(6):
        size = rng.uniform(0.3, 1.2, size=3)
        xy = rng.uniform([0.2, 0.2], room[:2] - size[:2] - 0.2)
        lo = np.array([xy[0], xy[1], 0.0])
        boxes.append((lo, lo + size, 0.6))
    area = np.array([2 * ((h - l)[0] * (h - l)[1] + (h - l)[0] * (h - l)[2] + (h - l)[1] * (h - l)[2]) * wgt
                     for l, h, wgt in boxes])
    counts = rng.multinomial(n, area / area.sum())
    pts = [_sample_box_surface(rng, c, l, h) for (l, h, _), c in zip(boxes, counts)]
    pts = np.concatenate(pts)
    return pts + rng.normal(scale=0.005, size=pts.shape), room


def _outdoor_scan(rng, origin, yaw, scene):
    """64-ring LiDAR model hitting a ground plane and boxes out to 80 m."""
    elev = np.deg2rad(np.linspace(-24.8, 2.0, 64))
    azim = np.linspace(-np.pi, np.pi, 1900, endpoint=False) + yaw
    e, a = np.meshgrid(elev, azim, indexing='ij')
    d = np.stack((np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)), -1).reshape(-1, 3)
    o = np.asarray(origin, float)
    t_hit = np.full(len(d), np.inf)
    # ground plane z = 0
    down = d[:, 2] < -1e-6
    t_hit[down] = -o[2] / d[down, 2]
    # axis aligned boxes: slab test
    for lo, hi in scene:
        with np.errstate(divide='ignore', invalid='ignore'):
            t1 = (lo - o) / d
            t2 = (hi - o) / d
        tmin = np.nanmax(np.minimum(t1, t2), axis=1)
        tmax = np.nanmin(np.maximum(t1, t2), axis=1)
        ok = (tmax >= tmin) & (tmin > 0)
        t_hit = np.where(ok & (tmin < t_hit), tmin, t_hit)
    keep = np.isfinite(t_hit) & (t_hit < 80.0)
    pts = o + d[keep] * t_hit[keep, None]
    return pts + rng.normal(scale=0.02, size=pts.shape)


def synth_pair(seed, n_raw=50000, kind='indoor', max_angle_deg=180.0, grid_align=None):
    """Returns xyz0 [n_raw,3], xyz1 [n_raw,3] float64 and the 4x4 ground truth T with
    xyz1 ~= T . xyz0 on the overlap (the quantity `register()` estimates).

    The pose is a rotation of up to `max_angle_deg` about a random axis and a translation in
    [-0.5, 0.5] m (optionally snapped to multiples of `grid_align`)."""
    rng = np.random.default_rng(seed)
    if kind == 'indoor':
        pts, room = _indoor_scene(rng, 6 * n_raw)
        v0 = pts[pts[:, 0] < 0.65 * room[0]]
        v1 = pts[pts[:, 0] > 0.35 * room[0]]
        v0 = v0[rng.permutation(len(v0))[:n_raw]]
        v1 = v1[rng.permutation(len(v1))[:n_raw]]
        assert len(v0) == n_raw and len(v1) == n_raw
        R = _random_rotation(rng, max_angle_deg)
        t = rng.uniform(-0.5, 0.5, size=3)
        if grid_align:
            t = np.round(t / grid_align) * grid_align
    elif kind == 'outdoor':
        scene = []
        for _ in range(40):
            c = rng.uniform([-70, -70], [70, 70])
            s = rng.uniform([2, 2, 1.5], [12, 12, 8])
            scene.append((np.array([c[0], c[1], 0.0]), np.array([c[0] + s[0], c[1] + s[1], s[2]])))
        v0 = _outdoor_scan(rng, [0, 0, 1.7], 0.0, scene)
        yaw = np.deg2rad(rng.uniform(-5, 5))
        v1w = _outdoor_scan(rng, [10.0, 0, 1.7], yaw, scene)
        # express each scan in its own sensor frame
        c, s = np.cos(yaw), np.sin(yaw)
        Rs = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        v0 = v0 - np.array([0, 0, 1.7])
        v1 = (v1w - np.array([10.0, 0, 1.7])) @ Rs          # world -> sensor-1 frame
        R = Rs.T
        t = -Rs.T @ np.array([10.0, 0, 0])
        if n_raw is not None and n_raw > 0:
            v0 = v0[rng.permutation(len(v0))[:n_raw]]
            v1 = v1[rng.permutation(len(v1))[:n_raw]]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        return np.ascontiguousarray(v0), np.ascontiguousarray(v1), T
    else:
        raise ValueError(kind)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    v1 = v1 @ R.T + t
    return np.ascontiguousarray(v0), np.ascontiguousarray(v1), T


def synth_scene(seed, n_fragments, n_raw=50000, window=0.55, min_overlap=0.5, max_angle_deg=180.0):
    """A scene as a scan sequence sees it: `n_fragments` windows of ONE `_indoor_scene` room, each `window` of the room's
    length wide, their centres evenly spaced along x, every fragment an own random subset of `n_raw` points of its window
    in its own random frame.  Returns (clouds, poses, pairs): clouds[k] [n_raw,3] float64 in fragment k's frame;
    poses [n,4,4] with x_k = poses[k] . x_world; pairs = [(i, j, T_gt), ...] for every i < j whose windows share at
    least `min_overlap` of their width, x_j = T_gt . x_i on the overlap (what `register()` estimates for (i, j)).
    Deterministic in `seed`."""
    if n_fragments < 2:
        raise ValueError('a scene needs at least two fragments')
    rng = np.random.default_rng(seed)
    pts, room = _indoor_scene(rng, 4 * n_raw)
    w = window * room[0]
    centres = np.linspace(w / 2, room[0] - w / 2, n_fragments)
    clouds, poses = [], np.tile(np.eye(4), (n_fragments, 1, 1))
    for k, c in enumerate(centres):
        v = pts[np.abs(pts[:, 0] - c) <= w / 2]
        assert len(v) >= n_raw, (len(v), n_raw)
        v = v[rng.permutation(len(v))[:n_raw]]
        poses[k, :3, :3] = _random_rotation(rng, max_angle_deg)
        poses[k, :3, 3] = rng.uniform(-0.5, 0.5, size=3)
        clouds.append(np.ascontiguousarray(v @ poses[k, :3, :3].T + poses[k, :3, 3]))
    pairs = [(i, j, poses[j] @ np.linalg.inv(poses[i])) for i in range(n_fragments) for j in range(i + 1, n_fragments)
             if w - (centres[j] - centres[i]) >= min_overlap * w]
    return clouds, poses, pairs


# ----------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------
def conv_layer_specs(D, cin, cout, conv1_ks):
    """(name, K, Cin, Cout, bn_name|None, level) for every conv of ResUNetBN2C
    (`model/resunet.py:436-596`), in forward order."""
    C, T = CHANNELS, TR_CHANNELS
    k3 = 3 ** D
    specs = [('conv1', conv1_ks ** D, cin, C[1], 'norm1', 1)]

    def block(name, c, lvl):
        return [(name + '.conv1', k3, c, c, name + '.norm1', lvl),
                (name + '.conv2', k3, c, c, name + '.norm2', lvl)]
    specs += block('block1', C[1], 1)
    specs += [('conv2', k3, C[1], C[2], 'norm2', 2)] + block('block2', C[2], 2)
    specs += [('conv3', k3, C[2], C[3], 'norm3', 4)] + block('block3', C[3], 4)
    specs += [('conv4', k3, C[3], C[4], 'norm4', 8)] + block('block4', C[4], 8)
    specs += [('conv4_tr', k3, C[4], T[4], 'norm4_tr', 4)] + block('block4_tr', T[4], 4)
    specs += [('conv3_tr', k3, C[3] + T[4], T[3], 'norm3_tr', 2)] + block('block3_tr', T[3], 2)
    specs += [('conv2_tr', k3, C[2] + T[3], T[2], 'norm2_tr', 1)] + block('block2_tr', T[2], 1)
    specs += [('conv1_tr', 1, C[1] + T[2], T[1], None, 1), ('final', 1, T[1], cout, None, 1)]
    return specs


def _k_eff(D, name, K, lvl):
    """Rough mean neighbour count so that activations stay O(1) through 23 layers
    (measured on 3DMatch-shaped synthetic clouds)."""
    if K == 1:
        return 1.0
    if D == 3:
        return {343: 70.0, 125: 35.0}.get(K, 14.0)
    return {1: 2.0, 2: 3.0, 4: 6.0, 8: 30.0}[lvl]


def synth_state_dict(D, cin, cout, conv1_ks, seed, dtype=np.float32):
    """Seeded state_dict with MinkowskiEngine 0.5.x key names and shapes."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, K, ci, co, bn, lvl in conv_layer_specs(D, cin, cout, conv1_ks):
        std = np.sqrt(2.0 / (_k_eff(D, name, K, lvl) * ci))
        shape = (ci, co) if K == 1 else (K, ci, co)
        sd[name + '.kernel'] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(dtype)
        if bn is not None:
            sd[bn + '.bn.weight'] = rng.uniform(0.5, 1.5, co).astype(dtype)
            sd[bn + '.bn.bias'] = (rng.standard_normal(co) * 0.1).astype(dtype)
            sd[bn + '.bn.running_mean'] = (rng.standard_normal(co) * 0.1).astype(dtype)
            sd[bn + '.bn.running_var'] = rng.uniform(0.5, 1.5, co).astype(dtype)
            sd[bn + '.bn.num_batches_tracked'] = np.array(1000, np.int64)
    sd['final.bias'] = (rng.standard_normal((1, cout)) * 0.1).astype(dtype)
    return sd


def synth_checkpoint(seed=0, voxel_size=0.05, feat_conv1_kernel_size=7, n_out=32,
                     inlier_feature_type='coords', with_inlier=True):
    """Dict in the layout `DeepGlobalRegistration.__init__` reads
    (`core/deep_global_registration.py:88-129`)."""
    cfg = dict(voxel_size=voxel_size, feat_model='ResUNetBN2C', feat_model_n_out=n_out,
               bn_momentum=0.05, feat_conv1_kernel_size=feat_conv1_kernel_size,
               normalize_feature=True, inlier_model='ResUNetBN2C',
               inlier_conv1_kernel_size=3, inlier_feature_type=inlier_feature_type,
               nn_max_n=250)
    ck = {'config': cfg,
          'state_dict': synth_state_dict(3, 1, n_out, feat_conv1_kernel_size, seed)}
    if with_inlier:
        cin6 = 6 if inlier_feature_type == 'coords' else 1
        ck['state_dict_inlier'] = synth_state_dict(6, cin6, 1, 3, seed + 1)
    return ck


def gt_forced_logits(xyz0_corr, xyz1_corr, T_gt, voxel_size, magnitude=4.0):
    """Teacher-forced inlier logits: +magnitude where the correspondence agrees with the
    ground-truth pose within 2 voxels, -magnitude elsewhere (random weights make the
    learned confidence meaningless)."""
    p = xyz0_corr @ T_gt[:3, :3].T + T_gt[:3, 3]
    d = np.linalg.norm(p - xyz1_corr, axis=1)
    return np.where(d < 2 * voxel_size, magnitude, -magnitude).astype(np.float32).reshape(-1, 1)


def gt_correspondences(xyz0, xyz1, T_gt, voxel_size, frac=0.5, seed=0):
    """Teacher-forced correspondences for synthetic weights: idx [N0] int64 with, for a random
    `frac` of the rows of fragment 0 that have a fragment-1 voxel within one voxel size of their
    ground-truth position, the index of that voxel; -1 elsewhere (= keep the 1-NN result).

    Untrained (seeded random) FCGF weights give descriptors that are not repeatable across views,
    so the feature matcher alone yields ~0 % correct correspondences; real checkpoints give tens of
    percent.  Overriding a share of the matches restores a realistic 6-D neighbourhood structure
    (SURVEY.md section 8d measured 23 % correct) without removing any stage from the timed path."""
    from scipy.spatial import cKDTree
    p = np.asarray(xyz0, np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3]
    d, j = cKDTree(np.asarray(xyz1, np.float64)).query(p, k=1)
    rng = np.random.default_rng(seed)
    take = (d < voxel_size) & (rng.random(len(p)) < frac)
    return np.where(take, j, -1).astype(np.int64)


# ----------------------------------------------------------------------------
# RGB-D sequences for the TSDF front end
# ----------------------------------------------------------------------------
def synth_rgbd(seed, n_frames, width, height, focal, sweep_deg=40.0, radius=0.5, cam_height=0.3):
    """A depth sequence of `_indoor_scene`'s recipe (a 4 x 3.5 x 2.6 m room with six cuboids on its floor), ray-cast
    analytically (ray against axis-aligned box) with its own random stream.  The world origin is the room's CENTRE, so
    block and voxel coordinates take both signs.  The camera (x right, y down, z forward) moves on an arc of `radius`
    around the vertical axis at `cam_height` above the centre -- above every cuboid, so it is never inside one --
    turning through `sweep_deg` while it looks outwards and slightly down.  Returns (depth uint16 [F,H,W] in
    millimetres, z-depth as a depth camera reports it; (fx, fy, cx, cy); poses float64 [F,4,4] camera-to-world;
    boxes = [(lo, hi), ...] with the room first).  Deterministic in `seed`; noise-free, so that the boxes are the
    ground truth of what is fused from it."""
    rng = np.random.default_rng(seed)
    room = np.array([4.0, 3.5, 2.6])
    boxes = [(-room / 2, room / 2)]
    for _ in range(6):
        size = rng.uniform(0.3, 1.2, size=3)
        xy = rng.uniform([0.2, 0.2], room[:2] - size[:2] - 0.2)
        lo = np.array([xy[0], xy[1], 0.0]) - room / 2
        boxes.append((lo, lo + size))
    start = rng.uniform(0, 2 * np.pi)
    fx = fy = float(focal)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    xn = (np.arange(width) - cx) / fx
    yn = (np.arange(height) - cy) / fy
    dirs_c = np.stack(np.broadcast_arrays(xn[None, :], yn[:, None], 1.0), -1).reshape(-1, 3)   # z-component 1: t IS depth
    depth = np.zeros((n_frames, height, width), np.uint16)
    poses = np.tile(np.eye(4), (n_frames, 1, 1))
    for f in range(n_frames):
        th = start + np.deg2rad(sweep_deg) * (f / max(n_frames - 1, 1))
        o = np.array([radius * np.cos(th), radius * np.sin(th), cam_height])
        fwd = np.array([np.cos(th + 0.3), np.sin(th + 0.3), -0.35])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd], 1)
        poses[f, :3, :3], poses[f, :3, 3] = R, o
        d = dirs_c @ R.T
        t_hit = np.full(len(d), np.inf)
        for k, (lo, hi) in enumerate(boxes):
            with np.errstate(divide='ignore', invalid='ignore'):
                t1 = (lo - o) / d
                t2 = (hi - o) / d
            tmin = np.nanmax(np.minimum(t1, t2), axis=1)
            tmax = np.nanmin(np.maximum(t1, t2), axis=1)
            if k == 0:      # the camera is inside the room: the ray leaves it at tmax
                t_hit = np.where(tmax > 0, tmax, t_hit)
            else:
                ok = (tmax >= tmin) & (tmin > 0)
                t_hit = np.where(ok & (tmin < t_hit), tmin, t_hit)
        mm = np.rint(t_hit * 1000.0)
        depth[f] = np.where(np.isfinite(mm) & (mm < 65535), mm, 0).astype(np.uint16).reshape(height, width)
    return depth, (fx, fy, cx, cy), poses, boxes


def color_texture(points, seed=0):
    """uint8 [N,3]: the procedural texture of `synth_color` at world points [N,3] -- per channel e
    rint(127.5 + 100 sin(k_e . p + phi_e)), k_e a seeded direction times 2 pi / wavelength with a wavelength in [1, 2] m,
    phi_e a seeded phase.  A function of the world point alone, so every view of a surface point sees one colour."""
    rng = np.random.default_rng([int(seed), 0xC0102])
    k = rng.standard_normal((3, 3))
    k *= (2 * np.pi / rng.uniform(1.0, 2.0, size=3) / np.linalg.norm(k, axis=1))[:, None]
    phi = rng.uniform(0, 2 * np.pi, size=3)
    return np.rint(127.5 + 100.0 * np.sin(np.asarray(points, np.float64) @ k.T + phi)).astype(np.uint8)


def synth_color(depth, intrinsic, poses, seed=0):
    """uint8 [F,H,W,3] colour images for a depth sequence (`synth_rgbd`'s, or any): every valid pixel (raw > 0) is
    back-projected to the world under its frame's pose (depth in millimetres) and gets `color_texture` there; invalid
    pixels get 0.  View-consistent up to the depth's rounding to millimetres."""
    depth = np.asarray(depth)
    F, H, W = depth.shape
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    xn = ((np.arange(W) - cx) / fx)[None, :]
    yn = ((np.arange(H) - cy) / fy)[:, None]
    out = np.zeros((F, H, W, 3), np.uint8)
    for f in range(F):
        d = depth[f].astype(np.float64) / 1000.0
        pc = np.stack([xn * d, yn * d, d], -1).reshape(-1, 3)
        M = np.asarray(poses[f], np.float64)
        pw = pc @ M[:3, :3].T + M[:3, 3]
        out[f] = np.where((depth[f] > 0)[..., None], color_texture(pw, seed).reshape(H, W, 3), 0)
    return out


def write_rgbd_sequence(directory, depth, intrinsic, poses, color=None):
    """Writes a sequence in the 3DMatch raw layout the reference's util/integration.py reads: `frame-%06d.depth.png`
    (16-bit grayscale, millimetres), `frame-%06d.pose.txt` (4x4 camera-to-world) and `intrinsics.txt` (3x3 K) in
    `directory`; with `color` uint8 [F,H,W,3] (`synth_color`'s) also `frame-%06d.color.png` (8-bit RGB), which
    `util.integration.process_seq(..., color=True)` fuses with the depth.  Returns the number of frames."""
    import os
    from .eval.formats import write_png_gray16, write_png_rgb8
    if color is not None and (np.asarray(color).shape != tuple(depth.shape) + (3,) or np.asarray(color).dtype != np.uint8):
        raise ValueError(f'color must be uint8 {list(depth.shape) + [3]}, got {np.asarray(color).dtype} {list(np.shape(color))}')
    os.makedirs(directory, exist_ok=True)
    fx, fy, cx, cy = intrinsic
    np.savetxt(os.path.join(directory, 'intrinsics.txt'), np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), fmt='%.17g')
    for f in range(len(depth)):
        write_png_gray16(os.path.join(directory, 'frame-%06d.depth.png' % f), depth[f])
        if color is not None:
            write_png_rgb8(os.path.join(directory, 'frame-%06d.color.png' % f), color[f])
        np.savetxt(os.path.join(directory, 'frame-%06d.pose.txt' % f), np.asarray(poses[f], np.float64), fmt='%.17g')
    return len(depth)
