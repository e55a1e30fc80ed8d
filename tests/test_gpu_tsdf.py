"""GPU: `ops.tsdf_fragment` (csrc/tsdf.hip) against its numpy statement (tests/tsdf_ref.py), and the layers above it
(`util.integration.process_seq`, fragments into `DeepGlobalRegistration.extract_fragments`).

`blocks`, `tsdf`, `weight` and `xyz` are compared for EXACT equality (the floats by their bits): both sides perform the same
correctly rounded float64 operations in the same order, without fused multiply-add, and one rounding to float32 per update.
The statement visits every voxel in every frame, the kernel culls whole frames per block: equality also shows the cull
conservative.  No tolerance and no excluded case."""
import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_ref
from tsdf_checks import check as _check, run as _run, same as _same

pytestmark = pytest.mark.gpu


def _small():
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    return depth.copy(), K, poses.copy(), s['voxel'], s['trunc']


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 4])
@pytest.mark.parametrize('block', [8, 16])
@pytest.mark.parametrize('size', ['small', 'large'])
def test_fixture_equals_statement(size, block, stride):
    s = tsdf_cases.SIZES[size]
    depth, K, poses, _ = tsdf_cases.sequence(size)
    want = tsdf_cases.statement(size, 0, block, stride)
    got = _run(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=stride)
    assert len(want['blocks']) > 1 and len(want['xyz']) > 1000 and want['cross'].any()
    assert want['weight'].max() == s['n_frames'] and want['weight'].min() == 0
    _same(got, want, f'{size} block {block} stride {stride}')


@pytest.mark.parametrize('block', [8, 16])
def test_image_size_not_a_multiple_of_the_stride(block):
    from deepglobalregistration_amd import synth
    depth, K, poses, _ = synth.synth_rgbd(3, 2, 81, 61, 70)
    got = _check(depth, K, poses, 0.04, 0.16, '81x61', block=block, stride=4)
    assert len(got['xyz']) > 1000


# ---- 2. degenerate inputs -----------------------------------------------------------------------------------------------
def test_one_valid_pixel():
    depth, K, poses, voxel, trunc = _small()
    one = np.zeros_like(depth[:1])
    one[0, 28, 40] = depth[0, 28, 40]
    for block in (8, 16):
        got = _check(one, K, poses[:1], voxel, trunc, 'one pixel', block=block)
        assert 1 <= len(got['blocks']) <= 8 and got['weight'].max() == 1


def test_no_valid_pixel_is_empty_not_an_error():
    from deepglobalregistration_amd import ops
    depth, K, poses, voxel, trunc = _small()
    got = _check(np.zeros_like(depth), K, poses, voxel, trunc, 'all zero')
    assert got['blocks'].shape == (0, 3) and got['xyz'].shape == (0, 3) and got['tsdf'].shape == (0, 4096)
    xyz = ops.tsdf_fragment(np.zeros_like(depth), K, poses, voxel, trunc)
    assert xyz.shape == (0, 3) and xyz.is_cuda
    # valid pixels, none of them on the stride's grid: still nothing
    off = depth.copy()
    off[:, ::4, ::4] = 0
    got = _check(off, K, poses, voxel, trunc, 'off-grid only', stride=4)
    assert len(got['blocks']) == 0


def test_frame_looking_away_and_camera_inside_the_volume():
    """Frame 2 looks the opposite way from frame 0 at the same place and has no valid pixel on the stride's grid, so it
    allocates nothing and every block is behind it (culled as a whole; its off-grid pixels are valid, so only geometry
    keeps it out).  Then a wall 10-30 cm in front of the cameras: the blocks hold the cameras, so some of their voxels have
    z <= 0 in frames the cull must keep."""
    depth, K, poses, voxel, trunc = _small()
    back = poses[0].copy()
    back[:3, 0], back[:3, 2] = -back[:3, 0], -back[:3, 2]          # half a turn about the camera's y axis
    d = np.concatenate([depth[:2], depth[:1]])
    d[2, ::4, ::4] = 0
    p = np.stack([poses[0], poses[1], back])
    for block in (8, 16):
        got = _check(d, K, p, voxel, trunc, 'looking away', block=block, stride=4)
        assert got['weight'].max() == 2
    near = np.full_like(depth, 100)
    near[:, 20:40] = 300
    for block in (8, 16):
        got = _check(near, K, poses, voxel, trunc, 'camera inside', block=block, stride=4)
        assert 0 < (got['weight'] == 0).sum() and got['weight'].max() >= 2


def test_raw_65535_and_depth_beyond_the_truncation():
    depth, K, poses, voxel, trunc = _small()
    depth[0, 10:20, 10:30] = 65535
    depth[1, 30:50, 40:60] = 5000        # 5 m > depth_trunc
    depth[2, ::3, ::5] = 4501
    depth[2, 1::3, ::5] = 4500           # exactly depth_trunc: valid
    _check(depth, K, poses, voxel, trunc, '65535 / 5 m')
    got = _check(depth, K, poses, voxel, trunc, 'depth_trunc 2', depth_trunc=2.0, stride=1, block=8)
    assert len(got['xyz']) > 0
    _check(depth, K, poses, voxel, trunc, 'depth_scale 500', depth_scale=500.0)


# ---- 3. options ---------------------------------------------------------------------------------------------------------
def test_min_weight():
    depth, K, poses, voxel, trunc = _small()
    full = tsdf_cases.statement('small')
    got = _check(depth, K, poses, voxel, trunc, 'min_weight 2', min_weight=2)
    assert 0 < len(got['xyz']) < len(full['xyz'])
    got = _check(depth, K, poses, voxel, trunc, 'min_weight F + 1', min_weight=len(depth) + 1)
    assert len(got['xyz']) == 0 and len(got['blocks']) == len(full['blocks'])


def test_frame_order_matters_and_is_followed():
    """reversed frames: another block order and other roundings, each equal to the statement on the same order"""
    depth, K, poses, voxel, trunc = _small()
    fwd = tsdf_cases.statement('small')
    got = _check(depth[::-1].copy(), K, poses[::-1].copy(), voxel, trunc, 'reversed')
    assert not np.array_equal(got['blocks'], fwd['blocks'])
    assert sorted(map(tuple, got['blocks'])) == sorted(map(tuple, fwd['blocks']))


def test_two_calls_agree_bit_for_bit_and_inputs_may_live_on_the_device():
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES['large']
    depth, K, poses, _ = tsdf_cases.sequence('large')
    a = _run(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
    b = _run(torch.from_numpy(depth.copy()).cuda(), K, torch.from_numpy(poses.copy()), s['voxel'], s['trunc'], block=8, stride=1)
    _same(a, b, 'second call')
    xyz = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)        # without the volume
    assert np.array_equal(xyz.cpu().numpy(), a['xyz'])
    st = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1, return_stats=True)
    assert st['n_blocks'] == len(a['blocks']) and 0 < st['kept'] <= st['n_blocks'] * len(depth)


def test_more_points_and_blocks_than_the_first_guess(monkeypatch):
    """the wrapper's first output arrays hold 2^10 blocks and (here) 1000 points: the library reports what it needs
    without writing past either, and a second call fetches the result"""
    from deepglobalregistration_amd import ops
    depth, K, poses, _ = tsdf_cases.sequence('large')
    monkeypatch.setattr(ops, 'TSDF_FIRST_POINTS', 1000)
    got = _run(depth, K, poses, 0.01, 0.04, block=8, stride=1)
    assert len(got['blocks']) > 1024
    _same(got, tsdf_ref.tsdf_fragment(depth, K, poses, 0.01, 0.04, block=8, stride=1), '1 cm voxels')


# ---- 4. the layers above ------------------------------------------------------------------------------------------------
def test_process_seq_writes_fragments_the_pipeline_accepts(tmp_path):
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.eval.formats import read_ply
    from deepglobalregistration_amd.util import integration
    from helpers import harness_dgr
    depth, K, poses, _ = synth.synth_rgbd(4, 8, 80, 60, 70, sweep_deg=80.0)
    seq = tmp_path / 'scene' / 'seq-01'
    synth.write_rgbd_sequence(str(seq), depth, K, poses)
    files = integration.process_seq(str(seq), str(tmp_path / 'out'), n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16)
    assert [f.rsplit('/', 1)[1] for f in files] == ['fragment-0.ply', 'fragment-1.ply']
    clouds = [read_ply(f) for f in files]
    for k, c in enumerate(clouds):
        want = ops.tsdf_fragment(depth[4 * k:4 * k + 4], K, poses[4 * k:4 * k + 4], 0.04, 0.16)
        assert len(c) > 1000 and np.array_equal(c, want.cpu().numpy())
    # relative_to_first = the call with premultiplied poses
    rel = integration.process_seq(str(seq), str(tmp_path / 'rel'), n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16,
                                  relative_to_first=True)
    for k, f in enumerate(rel):
        p = np.linalg.inv(poses[4 * k]) @ poses[4 * k:4 * k + 4]
        want = ops.tsdf_fragment(depth[4 * k:4 * k + 4], K, p, 0.04, 0.16)
        assert np.array_equal(read_ply(f), want.cpu().numpy())
        assert not np.array_equal(read_ply(f), clouds[k])
    # the command line: DATASET/seq* -> OUTPUT/<scene>/seq*/fragment-N.ply
    integration.main([str(tmp_path / 'scene'), str(tmp_path / 'cli'), '--frames', '4', '--voxel', '0.04'])
    assert sorted(p.name for p in (tmp_path / 'cli' / 'scene' / 'seq-01').iterdir()) == ['fragment-0.ply', 'fragment-1.ply']
    ck = synth.synth_checkpoint(seed=0, voxel_size=0.05, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))
    bank = dgr.extract_fragments(clouds)
    assert len(bank) == 2 and all(len(bank.xyz_of(i)) > 100 for i in range(2))
