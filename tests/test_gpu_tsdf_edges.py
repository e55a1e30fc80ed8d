"""GPU: `ops.tsdf_fragment` (csrc/tsdf.hip) at the edges no fixture of tests/test_gpu_tsdf.py reaches -- more frames than one
chunk of the cull (256), poses that are not rigid, block coordinates at +-2^26, general intrinsics, images of one row, one
column and one pixel, the capacity protocol of the C ABI with guard rows, side streams.  The inputs are the named cases of
tests/tsdf_cases.py; tests/test_tsdf_cpu.py asserts on the statement alone that each of them is the edge it claims to be.

Every comparison is `tsdf_checks.same`: `blocks`, `weight` and the bits of `tsdf` and `xyz` EQUAL the numpy statement
(tests/tsdf_ref.py).  No tolerance and no excluded case.  Each case also reads `kept`, the (block, frame) pairs the cull let
through: at least the pairs the statement updates (a cull that drops one of those has changed the result), at most nb F."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_ref
from tsdf_checks import run, same

pytestmark = pytest.mark.gpu
BLOCKS = (8, 16)
LIMIT = tsdf_ref.BLOCK_LIMIT


def _edge(name, block):
    """the case on the GPU (volume and `kept`) against its statement; returns (got, want)"""
    c = tsdf_cases.edge_case(name, block)
    want = tsdf_cases.edge_statement(name, block)
    got = run(c['depth'], c['K'], c['poses'], c['voxel'], c['trunc'], block=block, stride=c['stride'], return_stats=True)
    same(got, want, f'{name} block {block}')
    nb, F = len(want['blocks']), len(c['depth'])
    updated = int(want['updated'].sum())
    print(f'{name} block {block}: {nb} blocks, {len(want["xyz"])} points, kept {got["kept"]} of {nb * F}, updated {updated}')
    assert got['n_blocks'] == nb
    assert updated <= got['kept'] <= nb * F, (name, block, updated, got['kept'], nb * F)
    return got, want


# ---- A. more frames than one chunk of the cull ------------------------------------------------------------------------
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('name', tuple(tsdf_cases.FRAMES) + ('frames257_reversed',))
def test_frame_chunks(name, block):
    """255, 256, 257 and 513 frames: the last frame of a chunk, a chunk of one frame, a third chunk.  The camera turns
    through 120 degrees with a field of view of 59, so no voxel is seen by every frame (the statement's largest weight is
    124-125 of 255-257 frames, 249 of 513): the weights are held to the statement's, whose largest lies well above what
    one chunk's remainder could give, and test_tsdf_cpu.py shows blocks that only the second chunk updates."""
    got, want = _edge(name, block)
    F = len(tsdf_cases.edge_case(name, block)['depth'])
    assert got['weight'].max() == want['weight'].max() and want['weight'].max() > F // 3


# ---- B. poses that are not rigid --------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('name', tuple(tsdf_cases.NON_RIGID) + ('rotation_rounded_to_float32',))
def test_poses_that_are_not_rigid(name, block):
    """Any finite, invertible pose is accepted, and the statement is defined for it; the cull's ball is stretched by the
    extrinsic's largest row norm, so it stays conservative.  Without the stretch `quarter` loses 44 / 9 and `half` 3 / 1
    (block, frame) pairs the statement updates (block 8 / 16; tests/test_tsdf_cpu.py)."""
    got, _ = _edge(name, block)
    assert len(got['xyz']) > 1000


# ---- C. the block limit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('name', tuple(tsdf_cases.LIMIT))
def test_block_limit(name, block):
    """the scene moved to 20 cm inside +-2^26 blocks: the pixels beyond are skipped, the rest is hashed, looked up and
    integrated at voxel indices next to +-2^30 (block 16) as anywhere else"""
    got, _ = _edge(name, block)
    axis, sign = tsdf_cases.LIMIT[name]
    assert 0 < len(got['blocks']) < len(tsdf_cases.statement('small', 0, block, 4)['blocks'])
    if sign > 0:
        assert got['blocks'][:, axis].max() == LIMIT - 1
    else:
        assert got['blocks'][:, axis].min() == -LIMIT
    assert len(got['xyz']) > 500


@pytest.mark.parametrize('block', BLOCKS)
def test_beyond_the_block_limit_is_empty_not_an_error(block):
    got, _ = _edge('beyond_limit', block)
    assert got['blocks'].shape == (0, 3) and got['xyz'].shape == (0, 3) and got['kept'] == 0


# ---- D. intrinsics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('name', tuple(tsdf_cases.INTRINSICS))
def test_intrinsics(name, block):
    got, _ = _edge(name, block)
    assert len(got['xyz']) > 1000


# ---- E. image shapes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('name', tsdf_cases.SHAPES)
def test_image_shapes(name, block):
    got, want = _edge(name, block)
    assert len(got['blocks']) > 0
    if name == 'one_pixel':
        assert got['xyz'].shape == (0, 3) and got['weight'].max() == 1      # a result, not an error
    else:
        assert len(got['xyz']) > 0


# ---- F. capacities, through the C ABI ---------------------------------------------------------------------------------
PAD, FILL = 4, -77


def _raw_call(lib, ctx, args, block, xyz, max_points, blocks, tsdf, weight, max_blocks):
    from deepglobalregistration_amd import _lib, ops
    d, (F, H, W), intrinsic, pose, ext, voxel, trunc, stride = args
    nb, npts = C.c_int64(-7), C.c_int64(-7)
    rc = lib.dgr_tsdf_fragment(ctx, _lib.ptr(d), F, H, W, ops._np_ptr(intrinsic), ops._np_ptr(pose), ops._np_ptr(ext), voxel,
                               trunc, 1000.0, 4.5, block, stride, 1, _lib.ptr(xyz), max_points, _lib.ptr(blocks),
                               _lib.ptr(tsdf), _lib.ptr(weight), max_blocks, C.byref(nb), C.byref(npts), None,
                               _lib.stream_ptr(0))
    torch.cuda.synchronize()
    return rc, nb.value, npts.value


@pytest.mark.parametrize('block', BLOCKS)
def test_capacity_protocol_writes_nothing_past_any_array(block):
    from deepglobalregistration_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    ctx = _lib.get_ctx(dev)
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    want = tsdf_cases.statement('small', 0, block, 4)
    nb, P, V = len(want['blocks']), len(want['xyz']), block ** 3
    intrinsic, pose, ext, shape = ops.check_tsdf_args(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=4)
    d = torch.from_numpy(depth.copy().view(np.int16)).to(dev)
    args = (d, shape, intrinsic, pose, ext, s['voxel'], s['trunc'], 4)

    def buffers():
        return (torch.full((P + PAD, 3), float(FILL), dtype=torch.float64, device=dev),
                torch.full((nb + PAD, 3), FILL, dtype=torch.int32, device=dev),
                torch.full((nb + PAD, V), float(FILL), dtype=torch.float32, device=dev),
                torch.full((nb + PAD, V), FILL, dtype=torch.int32, device=dev))

    def untouched(*arrays):
        return all(bool((a == FILL).all()) for a in arrays)

    def ordinary_call_still_right(what):
        same(run(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=4), want, what)

    # one block short: reported before the integration, no byte of any output changed
    xyz, blocks, tsdf, weight = buffers()
    rc, n, p = _raw_call(lib, ctx, args, block, xyz, P, blocks, tsdf, weight, nb - 1)
    assert (rc, n) == (_lib.DGR_ENOMEM, nb), (rc, n, p)
    assert b'blocks' in lib.dgr_last_error()
    assert untouched(xyz, blocks, tsdf, weight)
    ordinary_call_still_right('after too few blocks')
    # one point short: the volume is there, xyz_out untouched, the volume's guard rows intact
    xyz, blocks, tsdf, weight = buffers()
    rc, n, p = _raw_call(lib, ctx, args, block, xyz, P - 1, blocks, tsdf, weight, nb)
    assert (rc, n, p) == (_lib.DGR_ENOMEM, nb, P), (rc, n, p)
    assert b'points' in lib.dgr_last_error()
    assert untouched(xyz, blocks[nb:], tsdf[nb:], weight[nb:])
    assert np.array_equal(blocks[:nb].cpu().numpy(), want['blocks']) and np.array_equal(weight[:nb].cpu().numpy(), want['weight'])
    ordinary_call_still_right('after too few points')
    # no room for points at all and no array for them: the sizes are reported, nothing is dereferenced
    _, blocks, tsdf, weight = buffers()
    rc, n, p = _raw_call(lib, ctx, args, block, None, 0, blocks, tsdf, weight, nb)
    assert P > 0 and (rc, n, p) == (_lib.DGR_ENOMEM, nb, P), (rc, n, p)
    assert untouched(blocks[nb:], tsdf[nb:], weight[nb:])
    ordinary_call_still_right('after xyz_out = NULL')
    # an exact fit
    xyz, blocks, tsdf, weight = buffers()
    rc, n, p = _raw_call(lib, ctx, args, block, xyz, P, blocks, tsdf, weight, nb)
    assert (rc, n, p) == (_lib.DGR_OK, nb, P), (rc, n, p, lib.dgr_last_error())
    assert untouched(xyz[P:], blocks[nb:], tsdf[nb:], weight[nb:])
    same({'xyz': xyz[:P].cpu().numpy(), 'blocks': blocks[:nb].cpu().numpy(), 'tsdf': tsdf[:nb].cpu().numpy(),
          'weight': weight[:nb].cpu().numpy()}, want, 'exact fit')


# ---- G. streams -------------------------------------------------------------------------------------------------------
def test_side_stream_and_partition_stream_give_the_null_streams_bits():
    from deepglobalregistration_amd import ops
    dev = torch.device('cuda:0')
    s = tsdf_cases.SIZES['large']
    depth, K, poses, _ = tsdf_cases.sequence('large')
    want = tsdf_cases.statement('large', 0, 8, 1)
    null = run(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
    same(null, want, 'null stream')
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        got = run(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
    same(got, null, 'side stream')
    try:
        part = ops.partition_stream(dev, 1, 4)
        assert part is not None
        with torch.cuda.stream(part):
            got = run(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
        same(got, null, 'partition stream')
    finally:
        assert ops.partition_stream(dev, 0, 1) is None
    same(run(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1), null, 'partition dropped')


# ---- H. the stretch costs rigid input nothing -------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 4])
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('size', ['small', 'large'])
def test_rigid_fixtures_keep_the_pairs_they_kept_before_the_stretch(size, block, stride):
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES[size]
    depth, K, poses, _ = tsdf_cases.sequence(size)
    st = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=stride, return_stats=True)
    print(f'{size} block {block} stride {stride}: kept {st["kept"]} of {st["n_blocks"] * len(depth)}')
    assert st['kept'] == tsdf_cases.RIGID_KEPT[size, block, stride]
