"""CPU: the numpy statement of the TSDF front end (tests/tsdf_ref.py) against analytic geometry, the argument checks of
`ops.tsdf_fragment`, the PNG reader / writer and the sequence files -- everything that needs no GPU."""
import os

import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_ref
from deepglobalregistration_amd import ops, synth
from deepglobalregistration_amd.eval import formats


def _surface_distance(p, boxes):
    """distance of every point to the nearest face of the nearest box (the room is seen from inside, the cuboids from
    outside: either way the surface is the box's boundary)"""
    best = np.full(len(p), np.inf)
    for lo, hi in boxes:
        outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=1)
        inside = np.minimum(p - lo, hi - p).min(1)
        best = np.minimum(best, np.where(outside > 0, outside, inside))
    return best


# ---- 1. geometric truth of the statement ------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('size', ['small', 'large'])
def test_statement_points_lie_on_the_boxes(size, seed):
    """The statement's points against the analytic box faces the depth was ray-cast from, in voxels.  Conditions (set by
    the issue, not by these figures): median <= 0.1 voxel, >= 95 % within half a voxel, none on the maximum (points at
    depth silhouettes are real).  Measured with the committed renderer, block 16, stride 4:
      small (80x60, f 70, 3 frames, 4 cm / 16 cm)   seeds 0-2: median 0.043 / 0.044 / 0.043, within 100 / 100 / 99.9 %
      large (160x120, f 140, 6 frames, 2 cm / 8 cm) seeds 0-2: median 0.009 / 0.020 / 0.012, within 100 / 100 / 100 %
    (3591-3845 and 21001-22982 points; maximum 0.35-0.50 voxel)."""
    _, _, _, boxes = tsdf_cases.sequence(size, seed)
    want = tsdf_cases.statement(size, seed)
    voxel = tsdf_cases.SIZES[size]['voxel']
    assert len(want['xyz']) > 1000
    d = _surface_distance(want['xyz'], boxes) / voxel
    print(f'{size} seed {seed}: {len(d)} points, median {np.median(d):.4f}, within half a voxel {(d <= 0.5).mean():.4f}, '
          f'max {d.max():.3f}')
    assert np.median(d) <= 0.1
    assert (d <= 0.5).mean() >= 0.95


def test_world_is_centred_and_camera_inside():
    depth, K, poses, boxes = tsdf_cases.sequence('large')
    lo, hi = boxes[0]
    assert np.array_equal(lo, -hi) and len(boxes) == 7
    assert ((poses[:, :3, 3] > lo) & (poses[:, :3, 3] < hi)).all()
    assert depth.dtype == np.uint16 and depth.min() > 0       # every ray ends on a wall or a cuboid
    b = tsdf_cases.statement('large')['blocks']
    assert (b < 0).any() and (b >= 0).any()
    again = synth.synth_rgbd(0, 6, 160, 120, 140)
    assert np.array_equal(again[0], depth) and np.array_equal(again[2], poses)


# ---- 2. crossings into a neighbouring block ---------------------------------------------------------------------------
@pytest.mark.parametrize('block,stride', [(16, 4), (8, 1)])
def test_fixture_has_crossings_into_neighbouring_blocks(block, stride):
    """measured: 630 (block 16) and 6840 (block 8) at the larger size, 57 and 74 at the smaller"""
    assert tsdf_cases.statement('large', 0, block, stride)['cross'].sum() >= 100
    assert tsdf_cases.statement('small', 0, block, stride)['cross'].sum() >= 1


# ---- 3. argument errors -----------------------------------------------------------------------------------------------
def _good():
    return dict(depth=np.ones((2, 6, 8), np.uint16), intrinsic=(10.0, 10.0, 3.5, 2.5), pose=np.tile(np.eye(4), (2, 1, 1)),
                voxel_length=0.01, sdf_trunc=0.04)


def test_check_tsdf_args_accepts_and_inverts():
    a = _good()
    a['pose'] = a['pose'].copy()
    a['pose'][1, :3, 3] = [1.0, 2.0, 3.0]
    intr, pose, ext, shape = ops.check_tsdf_args(**a)
    assert shape == (2, 6, 8) and intr.dtype == np.float64 and pose.shape == (2, 16) and ext.shape == (2, 16)
    assert np.array_equal(ext.reshape(2, 4, 4), np.linalg.inv(a['pose']))
    ops.check_tsdf_args(torch.ones((1, 6, 8), dtype=torch.uint16), a['intrinsic'], np.eye(4), 0.01, 0.04, block=8, stride=1,
                        min_weight=3)


@pytest.mark.parametrize('change', [
    dict(depth=np.ones((2, 6, 8), np.int32)), dict(depth=np.ones((2, 6, 8), np.float32)), dict(depth=np.ones((6, 8), np.uint16)),
    dict(depth=np.ones((2, 0, 8), np.uint16)), dict(depth=[[[1]]]),
    dict(intrinsic=(10.0, 10.0, 3.5)), dict(intrinsic=(10.0, np.nan, 3.5, 2.5)), dict(intrinsic=(np.inf, 10.0, 3.5, 2.5)),
    dict(intrinsic=(0.0, 10.0, 3.5, 2.5)), dict(intrinsic=(10.0, -10.0, 3.5, 2.5)),
    dict(pose=np.tile(np.eye(4), (3, 1, 1))), dict(pose=np.eye(4)), dict(pose=np.full((2, 4, 4), np.nan)),
    dict(pose=np.stack([np.eye(4), np.full((4, 4), np.inf)])), dict(pose=np.zeros((2, 4, 4))), dict(pose=np.zeros((2, 3, 4))),
    dict(block=4), dict(block=32), dict(block=8.0), dict(block=True),
    dict(voxel_length=0.0), dict(voxel_length=-1.0), dict(voxel_length=np.nan), dict(voxel_length='a'),
    dict(sdf_trunc=0.0), dict(sdf_trunc=np.inf), dict(sdf_trunc=0.17), dict(sdf_trunc=0.09, block=8),
    dict(depth_scale=0.0), dict(depth_trunc=-1.0), dict(depth_trunc=np.nan),
    dict(stride=0), dict(stride=-4), dict(stride=1.5), dict(min_weight=0), dict(min_weight=-1), dict(min_weight=1.0),
])
def test_check_tsdf_args_refuses(change):
    with pytest.raises(ValueError):
        ops.check_tsdf_args(**{**_good(), **change})


def test_tsdf_fragment_checks_before_it_needs_a_gpu():
    with pytest.raises(ValueError, match='block'):
        ops.tsdf_fragment(**{**_good(), 'block': 12})


# ---- 4. PNG -----------------------------------------------------------------------------------------------------------
def _images():
    rng = np.random.default_rng(0)
    return [tsdf_cases.sequence('small')[0][0], rng.integers(0, 65536, (7, 5)).astype(np.uint16),
            np.array([[0, 65535, 256, 255]], np.uint16), np.zeros((3, 1), np.uint16)]


@pytest.mark.parametrize('filter_type', [0, 1, 2, 3, 4])
def test_png_round_trip_every_filter(tmp_path, filter_type):
    for k, img in enumerate(_images()):
        name = str(tmp_path / f'{k}.png')
        formats.write_png_gray16(name, img, filter_type)
        got = formats.read_png_gray(name)
        assert got.dtype == np.uint16 and np.array_equal(got, img), (k, filter_type)


def test_png_agrees_with_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(1)
    for k, img in enumerate(_images()):
        for ft in range(5):
            name = str(tmp_path / f'{k}_{ft}.png')
            formats.write_png_gray16(name, img, ft)
            assert np.array_equal(np.asarray(Image.open(name)).astype(np.uint16), img), (k, ft)
    # files PIL writes (its encoder picks filters per line), 16 and 8 bit
    img16 = rng.integers(0, 65536, (33, 47)).astype(np.uint16)
    img16[10:20] = np.arange(47, dtype=np.uint16) * 300        # smooth rows: adaptive filters
    Image.fromarray(img16).save(str(tmp_path / 'pil16.png'))
    assert np.array_equal(formats.read_png_gray(str(tmp_path / 'pil16.png')), img16)
    img8 = (img16 >> 8).astype(np.uint8)
    Image.fromarray(img8).save(str(tmp_path / 'pil8.png'))
    got = formats.read_png_gray(str(tmp_path / 'pil8.png'))
    assert got.dtype == np.uint8 and np.array_equal(got, img8)


def test_png_refuses_what_it_does_not_read(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(tmp_path / 'rgb.png'))
    with pytest.raises(ValueError, match='grayscale'):
        formats.read_png_gray(str(tmp_path / 'rgb.png'))
    (tmp_path / 'not.png').write_bytes(b'hello')
    with pytest.raises(ValueError, match='not a PNG'):
        formats.read_png_gray(str(tmp_path / 'not.png'))
    with pytest.raises(ValueError):
        formats.write_png_gray16(str(tmp_path / 'x.png'), np.zeros((2, 2), np.uint8))


# ---- 5. files ---------------------------------------------------------------------------------------------------------
def test_sequence_files_and_discovery(tmp_path, monkeypatch):
    """write_rgbd_sequence, then process_seq's file discovery, grouping and output names with the GPU call stubbed out"""
    from deepglobalregistration_amd.util import integration
    depth, K, poses, _ = tsdf_cases.sequence('small')
    depth = np.concatenate([depth, depth[:2] + 1])         # 5 frames -> fragments of 2, 2, 1
    poses = np.concatenate([poses, poses[:2]])
    seq = tmp_path / 'scene' / 'seq-01'
    assert synth.write_rgbd_sequence(str(seq), depth, K, poses) == 5
    (seq / 'frame-000000.color.png').write_bytes(b'ignored')       # colour is neither read nor required
    names = sorted(os.listdir(seq))
    assert names[:3] == ['frame-000000.color.png', 'frame-000000.depth.png', 'frame-000000.pose.txt'] and 'intrinsics.txt' in names
    assert integration.read_intrinsics(str(seq / 'intrinsics.txt')) == K
    assert np.array_equal(integration.read_depth(str(seq / 'frame-000003.depth.png')), depth[3])
    assert np.array_equal(integration.read_pose(str(seq / 'frame-000004.pose.txt')), poses[4])
    calls = []

    def stub(d, intrinsic, pose, voxel_length, sdf_trunc, **kw):
        calls.append((d.copy(), intrinsic, pose.copy(), voxel_length, sdf_trunc, kw))
        return torch.full((len(calls), 3), float(len(calls)), dtype=torch.float64)
    monkeypatch.setattr(ops, 'tsdf_fragment', stub)
    out = tmp_path / 'out'
    files = integration.process_seq(str(seq), str(out), n_frames_per_fragment=2, voxel_length=0.04, sdf_trunc=0.16)
    assert files == [str(out / f'fragment-{k}.ply') for k in range(3)]
    assert [len(c[0]) for c in calls] == [2, 2, 1]
    assert np.array_equal(np.concatenate([c[0] for c in calls]), depth)
    assert np.array_equal(np.concatenate([c[2] for c in calls]), poses)
    assert all(c[1] == K and c[3] == 0.04 and c[4] == 0.16 for c in calls)
    assert [len(formats.read_ply(f)) for f in files] == [1, 2, 3]
    # relative_to_first: every fragment starts at the identity; intrinsics one level up
    os.rename(seq / 'intrinsics.txt', seq.parent / 'camera-intrinsics.txt')
    calls.clear()
    integration.process_seq(str(seq), str(out), n_frames_per_fragment=3, relative_to_first=True, stride=2)
    assert [len(c[0]) for c in calls] == [3, 2] and calls[0][5] == {'stride': 2} and calls[0][3:5] == (0.008, 0.04)
    assert np.array_equal(calls[1][2], np.linalg.inv(poses[3]) @ poses[3:])
    assert np.allclose(calls[1][2][0], np.eye(4), atol=1e-15)
    (seq / 'frame-000004.pose.txt').unlink()
    with pytest.raises(ValueError, match='pose files'):
        integration.process_seq(str(seq), str(out))


# ---- 6. the premises of tests/test_gpu_tsdf_edges.py, on the statement alone --------------------------------------------
BLOCKS = (8, 16)


def _lost(name, block, row_norm):
    """(block, frame) pairs the statement updates and the restated cull drops"""
    want = tsdf_cases.edge_statement(name, block)
    keep = tsdf_cases.cull_keeps(tsdf_cases.edge_case(name, block), want['blocks'], block, row_norm)
    return int((want['updated'] & ~keep).sum())


@pytest.mark.parametrize('block', BLOCKS)
def test_updated_pairs_are_what_single_frame_runs_update(block):
    """`updated[:, f]` of the statement = the blocks a run of `tsdf_integrate` on frame f alone leaves with weight > 0"""
    c = tsdf_cases.edge_case('shear', block)
    want = tsdf_cases.edge_statement('shear', block)
    ext = np.linalg.inv(c['poses'])
    for f in range(len(c['depth'])):
        _, w = tsdf_ref.tsdf_integrate(want['blocks'], c['depth'][f:f + 1], c['K'], ext[f:f + 1], c['voxel'], c['trunc'], 1000.0,
                                       4.5, block)
        assert np.array_equal((w > 0).any(1), want['updated'][:, f])
    assert 0 < want['updated'].sum() < want['updated'].size


@pytest.mark.parametrize('block,at_least', [(8, 10), (16, 5)])
def test_second_frame_chunk_has_work_of_its_own(block, at_least):
    """257 frames: blocks that frame 256 -- the only frame of the second chunk -- updates and frame 0 does not, and the
    other way round (measured 106 and 62 of 310 blocks of 8^3, 33 and 10 of 71 of 16^3): a flag of chunk 0 read in chunk 1
    would drop or add updates.  No voxel is seen by all frames of a 120-degree turn (largest weight 125)."""
    want = tsdf_cases.edge_statement('frames257', block)
    up = want['updated']
    assert up.shape[1] == 257 == tsdf_cases.FRAME_CHUNK + 1
    new, gone = int((up[:, 256] & ~up[:, 0]).sum()), int((up[:, 0] & ~up[:, 256]).sum())
    print(f'block {block}: {new} blocks updated by frame 256 and not by frame 0, {gone} the other way, of {len(up)}')
    assert new >= at_least and gone >= at_least
    assert want['weight'].max() > 257 // 3 and len(want['xyz']) > 1000
    rev = tsdf_cases.edge_statement('frames257_reversed', block)
    assert not np.array_equal(rev['blocks'], want['blocks']) and np.array_equal(rev['weight'].max(), want['weight'].max())
    for name, F in tsdf_cases.FRAMES.items():
        assert len(tsdf_cases.edge_case(name, block)['depth']) == F


@pytest.mark.parametrize('block,quarter,half', [(8, 20, 1), (16, 5, 1)])
def test_cull_without_the_row_norm_loses_updates_and_with_it_none(block, quarter, half):
    """The ball rule restated (tsdf_ref.cull_keeps).  Without the row-norm factor it drops pairs the statement updates:
    44 / 9 for poses scaled by 0.25 and 3 / 1 for 0.5 (block 8 / 16), so the GPU comparison of these cases fails on a
    kernel without the factor.  With it no case loses a pair, and the rigid fixtures keep exactly what they kept."""
    assert _lost('quarter', block, False) >= quarter
    assert _lost('half', block, False) >= half
    for name in tuple(tsdf_cases.NON_RIGID) + ('rotation_rounded_to_float32',):
        assert _lost(name, block, True) == 0, name
        assert len(tsdf_cases.edge_statement(name, block)['xyz']) > 1000
    for size in ('small', 'large'):
        for stride in (1, 4):
            depth, K, poses, _ = tsdf_cases.sequence(size)
            s = tsdf_cases.SIZES[size]
            case = dict(depth=depth, K=K, poses=poses, voxel=s['voxel'], trunc=s['trunc'])
            want = tsdf_ref.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=stride, return_updated=True)
            on, off = (tsdf_cases.cull_keeps(case, want['blocks'], block, r) for r in (True, False))
            assert not (want['updated'] & ~on).any() and np.array_equal(on, off), (size, stride)


@pytest.mark.parametrize('block', BLOCKS)
def test_block_limit_cases_sit_on_the_limit(block):
    """measured: 58-118 blocks and 1077-3141 points at block 8, 9-22 blocks at block 16"""
    full = len(tsdf_cases.statement('small', 0, block, 4)['blocks'])
    for name, (axis, sign) in tsdf_cases.LIMIT.items():
        want = tsdf_cases.edge_statement(name, block)
        b = want['blocks'][:, axis]
        assert 0 < len(b) < full and len(want['xyz']) > 500
        assert (b.max() == tsdf_ref.BLOCK_LIMIT - 1) if sign > 0 else (b.min() == -tsdf_ref.BLOCK_LIMIT)
        i = b.astype(np.int64) * block
        assert np.abs(i).max() >= 2 ** 26 * block - 8 * block and np.abs(i).max() + block <= 2 ** 31     # fits an int32
    want = tsdf_cases.edge_statement('beyond_limit', block)
    assert len(want['blocks']) == 0 and len(want['xyz']) == 0


@pytest.mark.parametrize('block', BLOCKS)
def test_intrinsics_and_image_shape_cases_are_what_they_claim(block):
    """3800-7300 points for the four intrinsics; one pixel gives 24 / 5 blocks and no point"""
    for name, (fx, fy, cx, cy) in tsdf_cases.INTRINSICS.items():
        assert len(tsdf_cases.edge_statement(name, block)['xyz']) > 1000
    K = tsdf_cases.INTRINSICS
    assert K['fx_ne_fy'][0] != K['fx_ne_fy'][1] and K['cx_left_of_image'][2] + 0.5 < 0 and K['cy_below_image'][3] + 0.5 > 60
    shapes = {name: tsdf_cases.edge_case(name, block)['depth'].shape for name in tsdf_cases.SHAPES}
    assert shapes == {'one_row': (3, 1, 80), 'one_column': (3, 60, 1), 'one_pixel': (3, 1, 1), 'stride_beyond_image': (3, 60, 80),
                      'one_frame': (1, 60, 80)}
    assert tsdf_cases.edge_case('stride_beyond_image', block)['stride'] > 80
    for name in tsdf_cases.SHAPES:
        want = tsdf_cases.edge_statement(name, block)
        assert len(want['blocks']) > 0 and (len(want['xyz']) > 0) == (name != 'one_pixel')
    one = tsdf_cases.edge_statement('one_pixel', block)
    assert len(one['blocks']) == {8: 24, 16: 5}[block] and one['weight'].max() == 1
