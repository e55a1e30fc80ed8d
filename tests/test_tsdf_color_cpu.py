"""No GPU: the premises of the colour tests (tests/tsdf_color_ref.py is tests/tsdf_ref.py with colour and nothing else), the
colour statement on inputs whose answer is known in closed form, the file formats that carry colour, and the argument
checks of the Python layer."""
import struct
import zlib

import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_color_ref
import tsdf_mesh_ref
import tsdf_ref

from deepglobalregistration_amd import ops, synth
from deepglobalregistration_amd.eval import formats
from deepglobalregistration_amd.util import integration


def _small(block=16, stride=4):
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    return depth, K, poses, s['voxel'], s['trunc'], tsdf_cases.statement('small', 0, block, stride)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- 1. the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block,stride', [(8, 1), (16, 4)])
def test_statement_with_colour_is_the_statement_without(block, stride):
    depth, K, poses, voxel, trunc, want = _small(block, stride)
    got = tsdf_color_ref.tsdf_fragment(depth, tsdf_color_ref.noise_color(depth), K, poses, voxel, trunc, block=block, stride=stride)
    for k in ('blocks', 'tsdf', 'weight', 'xyz'):
        assert got[k].dtype == want[k].dtype and np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got['rgb_sum'].shape == want['tsdf'].shape + (3,) and got['color'].shape == want['xyz'].shape
    assert got['color'].min() >= 0.0 and got['color'].max() <= 1.0 and len(got['color']) > 1000
    # the far end of a crossing edge is the voxel one step along the edge's axis: the ends the colours read are the ends
    # the positions read
    B = block
    o0, o1 = got['ends'][:, 0], got['ends'][:, 1]
    g = [got['blocks'].astype(np.int64)[o // B ** 3] * B + tsdf_ref._local(B)[o % B ** 3] for o in (o0, o1)]
    step = g[1] - g[0]
    assert (np.abs(step).sum(1) == 1).all() and (step.sum(1) == 1).all()
    assert ((o1 // B ** 3) != (o0 // B ** 3)).tolist() == want['cross'].tolist()


def test_constant_colour():
    depth, K, poses, voxel, trunc, want = _small()
    colour = np.array([10, 128, 250], np.uint8)
    got = tsdf_color_ref.tsdf_fragment(depth, np.broadcast_to(colour, depth.shape + (3,)), K, poses, voxel, trunc)
    assert np.array_equal(got['rgb_sum'], got['weight'][..., None] * colour.astype(np.int32))
    assert (got['weight'] > 0).any() and len(got['color']) > 1000
    # m0 == m1 == colour exactly, m1 - m0 == 0, so the blend is exact whatever r is
    assert np.array_equal(_bits(got['color']), _bits(np.broadcast_to(colour / 255.0, got['color'].shape)))


def test_per_frame_constant_colours_sum_over_the_frames_that_update_the_voxel():
    depth, K, poses, voxel, trunc, want = _small()
    F = len(depth)
    per_frame = np.array([[200, 3, 77], [5, 250, 130], [90, 91, 255]], np.uint8)[:F]
    color = np.broadcast_to(per_frame[:, None, None, :], depth.shape + (3,))
    got = tsdf_color_ref.tsdf_fragment(depth, color, K, poses, voxel, trunc)
    # a frame's update condition does not depend on the voxel's state: a run on the frame alone leaves weight > 0 exactly
    # where the frame updates (tsdf_ref.tsdf_integrate's `updated`, per voxel)
    ext = np.linalg.inv(poses)
    expect = np.zeros(want['weight'].shape + (3,), np.int64)
    n_updates = np.zeros(want['weight'].shape, np.int64)
    for f in range(F):
        _, w = tsdf_ref.tsdf_integrate(want['blocks'], depth[f:f + 1], K, ext[f:f + 1], voxel, trunc, 1000.0, 4.5, 16)
        assert set(np.unique(w)) <= {0, 1}
        expect += w[..., None].astype(np.int64) * per_frame[f].astype(np.int64)
        n_updates += w
    assert np.array_equal(n_updates, want['weight']) and len(np.unique(n_updates)) == F + 1
    assert np.array_equal(got['rgb_sum'], expect)


def test_poisoned_sums_of_unusable_voxels_do_not_reach_a_colour():
    depth, K, poses, voxel, trunc, want = _small(8, 4)
    got = tsdf_color_ref.tsdf_fragment(depth, tsdf_color_ref.noise_color(depth), K, poses, voxel, trunc, block=8)
    lim = np.float32(0.98)
    usable = (got['weight'] >= 1) & (got['tsdf'] >= -lim) & (got['tsdf'] < lim)
    assert usable.reshape(-1)[got['ends']].all() and not usable.all()
    poisoned = np.where(usable[..., None], got['rgb_sum'], np.iinfo(np.int32).min)
    _, c = tsdf_color_ref.tsdf_colors(got['blocks'], got['tsdf'], got['weight'], poisoned, voxel, 8, 1)
    assert np.array_equal(_bits(c), _bits(got['color']))


def test_mesh_vertices_are_the_coloured_points():
    depth, K, poses, voxel, trunc, want = _small(8, 4)
    got = tsdf_color_ref.tsdf_fragment(depth, tsdf_color_ref.noise_color(depth), K, poses, voxel, trunc, block=8)
    xyz, _, _ = tsdf_mesh_ref.tsdf_mesh(got['blocks'], got['tsdf'], got['weight'], voxel, 8, 1)
    assert np.array_equal(_bits(xyz), _bits(got['xyz']))


def test_the_frame_limit_is_the_largest_that_fits():
    assert 255 * ops.TSDF_COLOR_MAX_FRAMES <= 2 ** 31 - 1 < 255 * (ops.TSDF_COLOR_MAX_FRAMES + 1)
    assert ops.TSDF_COLOR_MAX_FRAMES == tsdf_color_ref.MAX_FRAMES == 8421504


# ---- 2. synthetic colour ------------------------------------------------------------------------------------------------
def test_synth_color_is_a_function_of_the_world_point():
    depth, K, poses, _ = tsdf_cases.sequence('small')
    c = synth.synth_color(depth, K, poses, seed=3)
    assert c.dtype == np.uint8 and c.shape == depth.shape + (3,)
    assert np.array_equal(c, synth.synth_color(depth, K, poses, seed=3)) and not np.array_equal(c, synth.synth_color(depth, K, poses, seed=4))
    hole = depth.copy()
    hole[:, 10:20, 10:20] = 0
    ch = synth.synth_color(hole, K, poses, seed=3)
    assert (ch[:, 10:20, 10:20] == 0).all() and np.array_equal(ch[:, 30:], c[:, 30:])
    valid = depth > 0
    assert c[valid].min() >= 27 and c[valid].max() <= 228 and c[valid].std() > 20
    # the texture at a pixel's own world point
    fx, fy, cx, cy = K
    f, v, u = 1, 17, 33
    d = depth[f, v, u] / 1000.0
    pw = poses[f][:3, :3] @ np.array([(u - cx) / fx * d, (v - cy) / fy * d, d]) + poses[f][:3, 3]
    assert np.abs(synth.color_texture(pw[None], 3)[0].astype(int) - c[f, v, u].astype(int)).max() <= 1
    # wavelength >= 1 m: over 1 cm a channel moves by at most 100 * 2 pi * 0.01 < 7 levels (+ 1 for the rounding)
    p = np.random.default_rng(0).uniform(-2, 2, (1000, 3))
    step = np.array([0.01, 0.0, 0.0])
    assert np.abs(synth.color_texture(p, 3).astype(int) - synth.color_texture(p + step, 3).astype(int)).max() <= 8
    assert len(synth.synth_rgbd(0, 2, 20, 15, 17.5)) == 4


# ---- 3. files -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filter_type', [0, 1, 2, 3, 4])
def test_png_rgb_round_trip(tmp_path, filter_type):
    rng = np.random.default_rng(filter_type)
    for h, w in ((7, 5), (1, 1), (3, 16)):
        img = rng.integers(0, 256, (h, w, 3), np.uint8)
        name = str(tmp_path / f'{h}x{w}.png')
        formats.write_png_rgb8(name, img, filter_type)
        back = formats.read_png_rgb8(name)
        assert back.dtype == np.uint8 and back.shape == (h, w, 3) and np.array_equal(back, img)
        with pytest.raises(ValueError):
            formats.read_png_gray(name)


def _png(w, h, depth, colour, rows, interlace=0):
    body = b''.join(bytes([ft]) + bytes(r) for ft, r in rows)
    return formats._PNG_MAGIC + formats._png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour, 0, 0, interlace)) \
        + formats._png_chunk(b'IDAT', zlib.compress(body)) + formats._png_chunk(b'IEND', b'')


@pytest.mark.parametrize('filter_type', [0, 1, 2, 3, 4])
def test_png_rgba_round_trip_drops_alpha(tmp_path, filter_type):
    """RGBA scanlines filtered here, byte by byte as the PNG specification states the filters (bpp = 4)"""
    rng = np.random.default_rng(10 + filter_type)
    h, w = 6, 7
    img = rng.integers(0, 256, (h, w, 4), np.uint8)
    raw = img.reshape(h, w * 4).astype(int)
    rows = []
    for y in range(h):
        line = []
        for i in range(w * 4):
            a = raw[y, i - 4] if i >= 4 else 0
            b = raw[y - 1, i] if y else 0
            c = raw[y - 1, i - 4] if y and i >= 4 else 0
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
            line.append((raw[y, i] - [0, a, b, (a + b) // 2, paeth][filter_type]) & 0xff)
        rows.append((filter_type, line))
    name = tmp_path / 'rgba.png'
    name.write_bytes(_png(w, h, 8, 6, rows))
    assert np.array_equal(formats.read_png_rgb8(str(name)), img[:, :, :3])


def test_png_hand_assembled_type_6_and_what_is_refused(tmp_path):
    # 2 x 2 RGBA: row 0 unfiltered, row 1 with Up
    rows = [(0, [1, 2, 3, 255, 250, 251, 252, 0]), (2, [10, 10, 10, 0, 10, 10, 10, 7])]
    name = tmp_path / 'hand.png'
    name.write_bytes(_png(2, 2, 8, 6, rows))
    want = np.array([[[1, 2, 3], [250, 251, 252]], [[11, 12, 13], [4, 5, 6]]], np.uint8)
    assert np.array_equal(formats.read_png_rgb8(str(name)), want)
    for what, data in (('16-bit RGB', _png(1, 1, 16, 2, [(0, [0] * 6)])), ('palette', _png(1, 1, 8, 3, [(0, [0])])),
                       ('gray', _png(1, 1, 8, 0, [(0, [0])])), ('gray + alpha', _png(1, 1, 8, 4, [(0, [0, 0])])),
                       ('interlaced', _png(1, 1, 8, 2, [(0, [0] * 3)], interlace=1)), ('not a PNG', b'nothing')):
        bad = tmp_path / 'bad.png'
        bad.write_bytes(data)
        with pytest.raises(ValueError):
            formats.read_png_rgb8(str(bad))
    with pytest.raises(ValueError):
        formats.write_png_rgb8(str(tmp_path / 'x.png'), np.zeros((2, 2, 4), np.uint8))
    with pytest.raises(ValueError):
        formats.write_png_rgb8(str(tmp_path / 'x.png'), np.zeros((2, 2, 3), np.uint16))
    # the grayscale reader reads what it read
    depth = np.arange(12, dtype=np.uint16).reshape(3, 4) * 5000
    for ft in range(5):
        formats.write_png_gray16(str(tmp_path / 'd.png'), depth, ft)
        assert np.array_equal(formats.read_png_gray(str(tmp_path / 'd.png')), depth)
        with pytest.raises(ValueError):
            formats.read_png_rgb8(str(tmp_path / 'd.png'))


@pytest.mark.parametrize('binary', [True, False])
def test_ply_colour_round_trip(tmp_path, binary):
    rng = np.random.default_rng(5)
    xyz, normals = rng.standard_normal((9, 3)), rng.standard_normal((9, 3))
    colors = rng.uniform(0, 1, (9, 3))
    colors[0], colors[1], colors[2] = (0.0, 1.0, 0.5 / 255), (1.5 / 255, 2.5 / 255, -0.2), (1.2, 254.5 / 255, 0.999)
    want = np.clip(np.rint(255.0 * colors), 0, 255).astype(np.uint8)
    assert want[0].tolist() == [0, 255, 0] and want[1].tolist() == [2, 2, 0] and want[2].tolist() == [255, 254, 255]
    tri = np.array([[0, 1, 2], [3, 4, 8]], np.int32)
    pts, mesh, plain = (str(tmp_path / n) for n in ('p.ply', 'm.ply', 'plain.ply'))
    formats.write_ply(pts, xyz, binary=binary, colors=colors)
    got_xyz, got_c = formats.read_ply(pts, return_colors=True)
    assert np.array_equal(got_xyz, xyz) and got_c.dtype == np.uint8 and np.array_equal(got_c, want)
    assert np.array_equal(formats.read_ply(pts), xyz)                      # the default return stays a bare array
    formats.write_ply_mesh(mesh, xyz, tri, normals, binary=binary, colors=colors)
    m = formats.read_ply_mesh(mesh)
    assert np.array_equal(m['xyz'], xyz) and np.array_equal(m['normals'], normals) and np.array_equal(m['triangles'], tri)
    assert m['colors'].dtype == np.uint8 and np.array_equal(m['colors'], want)
    assert np.array_equal(formats.read_ply(mesh), xyz)
    header = open(mesh, 'rb').read().split(b'end_header')[0].decode().split('\n')
    props = [line.split()[-1] for line in header if line.startswith('property') and 'list' not in line]
    assert props == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue']
    formats.write_ply_mesh(mesh, xyz, tri, binary=binary, colors=colors)     # colours without normals
    m = formats.read_ply_mesh(mesh)
    assert 'normals' not in m and np.array_equal(m['colors'], want)
    # without colours: no colour comes back
    formats.write_ply(plain, xyz, binary=binary)
    assert formats.read_ply(plain, return_colors=True)[1] is None
    formats.write_ply_mesh(plain, xyz, tri, normals, binary=binary)
    assert 'colors' not in formats.read_ply_mesh(plain)
    with pytest.raises(ValueError):
        formats.write_ply(pts, xyz, binary=binary, colors=colors[:5])


def test_ply_without_colours_is_written_as_before(tmp_path):
    """the bytes of a file without colours, spelt out"""
    xyz = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5]])
    normals = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    tri = np.array([[0, 1, 0]], np.int32)
    name = str(tmp_path / 'a.ply')
    formats.write_ply(name, xyz)
    assert open(name, 'rb').read() == (b'ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty double x\nproperty double y\n'
                                       b'property double z\nend_header\n' + xyz.astype('<f8').tobytes())
    formats.write_ply(name, xyz, binary=False)
    assert open(name, 'rb').read() == (b'ply\nformat ascii 1.0\nelement vertex 2\nproperty double x\nproperty double y\n'
                                       b'property double z\nend_header\n0.5 -1.25 3\n0.001 2 -7.5\n')
    formats.write_ply_mesh(name, xyz, tri, normals)
    assert open(name, 'rb').read() == (b'ply\nformat binary_little_endian 1.0\nelement vertex 2\n'
                                       + b''.join(b'property double %s\n' % k for k in (b'x', b'y', b'z', b'nx', b'ny', b'nz'))
                                       + b'element face 1\nproperty list uchar int vertex_indices\nend_header\n'
                                       + np.concatenate([xyz, normals], 1).astype('<f8').tobytes()
                                       + b'\x03' + tri.astype('<i4').tobytes())
    formats.write_ply_mesh(name, xyz, tri, binary=False)
    assert open(name, 'rb').read() == (b'ply\nformat ascii 1.0\nelement vertex 2\nproperty double x\nproperty double y\n'
                                       b'property double z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n'
                                       b'0.5 -1.25 3\n0.001 2 -7.5\n3 0 1 0\n')


# ---- 4. argument checks -------------------------------------------------------------------------------------------------
class _Stub:
    """an array's dtype and shape without its memory"""

    def __init__(self, dtype, shape):
        self.dtype, self.shape, self.ndim = np.dtype(dtype), tuple(shape), len(shape)


def test_colour_argument_checks():
    depth, K, poses, voxel, trunc, _ = _small()
    F, H, W = depth.shape
    good = np.zeros((F, H, W, 3), np.uint8)
    ops.check_tsdf_color_args(good, depth)
    ops.check_tsdf_color_args(torch.from_numpy(good), depth)
    for bad in (good.astype(np.int8), good.astype(np.float32), good[:-1], good[:, :-1], good[..., :2], good[..., 0],
                np.zeros((F, H, W, 4), np.uint8), np.zeros((F, W, H, 3), np.uint8), torch.zeros((F, H, W, 3), dtype=torch.int16),
                [[1, 2, 3]], 'red'):
        with pytest.raises(ValueError):
            ops.check_tsdf_color_args(bad, depth)
        with pytest.raises(ValueError):                         # the call refuses it before it needs a library or a device
            ops.tsdf_fragment(depth, K, poses, voxel, trunc, color=bad)
    # too many frames: shapes alone
    limit = ops.TSDF_COLOR_MAX_FRAMES
    ops.check_tsdf_color_args(_Stub('uint8', (limit, 1, 1, 3)), _Stub('uint16', (limit, 1, 1)))
    with pytest.raises(ValueError, match='frames'):
        ops.check_tsdf_color_args(_Stub('uint8', (limit + 1, 1, 1, 3)), _Stub('uint16', (limit + 1, 1, 1)))


def test_mesh_colour_argument_checks():
    tsdf = torch.zeros((2, 512))
    ops.check_tsdf_mesh_color_args(torch.zeros((2, 512, 3), dtype=torch.int32), tsdf)
    for bad in (torch.zeros((2, 512, 3), dtype=torch.int64), torch.zeros((2, 512, 3)), torch.zeros((2, 512), dtype=torch.int32),
                torch.zeros((3, 512, 3), dtype=torch.int32), torch.zeros((2, 4096, 3), dtype=torch.int32),
                np.zeros((2, 512, 3), np.int32), None):
        with pytest.raises(ValueError):
            ops.check_tsdf_mesh_color_args(bad, tsdf)


def test_process_seq_colour_files_must_match_the_depth_files(tmp_path):
    depth, K, poses, _ = synth.synth_rgbd(4, 4, 20, 15, 17.5)
    color = synth.synth_color(depth, K, poses)
    seq = tmp_path / 'seq-01'
    assert synth.write_rgbd_sequence(str(seq), depth, K, poses, color=color) == 4
    names = sorted(p.name for p in seq.iterdir())
    assert names.count('intrinsics.txt') == 1 and [n for n in names if n.endswith('.color.png')] == \
        ['frame-%06d.color.png' % f for f in range(4)]
    for f in range(4):
        assert np.array_equal(formats.read_png_rgb8(str(seq / ('frame-%06d.color.png' % f))), color[f])
        assert np.array_equal(formats.read_png_gray(str(seq / ('frame-%06d.depth.png' % f))), depth[f])
    assert integration.list_color_files(str(seq), 4) == ['frame-%06d.color.png' % f for f in range(4)]
    # a colour image of another size: ValueError naming the file, before the fusion is asked for anything
    formats.write_png_rgb8(str(seq / 'frame-000002.color.png'), np.zeros((15, 21, 3), np.uint8))
    with pytest.raises(ValueError, match='frame-000002.color.png'):
        integration.process_seq(str(seq), str(tmp_path / 'out'), n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16, color=True)
    # a missing colour file
    (seq / 'frame-000002.color.png').unlink()
    with pytest.raises(ValueError, match='colour files'):
        integration.process_seq(str(seq), str(tmp_path / 'out'), n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16, color=True)
    with pytest.raises(ValueError):
        synth.write_rgbd_sequence(str(tmp_path / 'bad'), depth, K, poses, color=color[:, :, :, :2])
