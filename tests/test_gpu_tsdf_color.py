"""GPU: colour in `ops.tsdf_fragment(..., color=)` (csrc/tsdf.hip) and `ops.tsdf_mesh(..., rgb_sum=)` (csrc/tsdfmesh.hip) against
the numpy statement (tests/tsdf_color_ref.py), and `util.integration.process_seq(color=True)` above them.

Every comparison is EXACT, the floats by their bits: the colour sums are integers, and a point's colour is the same
correctly rounded float64 operations in the same order on both sides, without fused multiply-add.  The colour images are
seeded noise, so a wrong pixel, frame or channel cannot hide.  `blocks`, `tsdf`, `weight` and `xyz` are compared with the
statement AND with the same call without `color`: colour changes nothing it does not add."""
import functools

import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_color_ref
from tsdf_checks import run as _run_plain, same as _same

pytestmark = pytest.mark.gpu
INT32_MIN = np.iinfo(np.int32).min


def _run(depth, color, K, poses, voxel, trunc, **kw):
    from deepglobalregistration_amd import ops
    r = ops.tsdf_fragment(depth, K, poses, voxel, trunc, return_volume=True, color=color, **kw)
    B = kw.get('block', 16)
    assert r['color'].is_cuda and r['color'].dtype == torch.float64 and r['color'].shape == r['xyz'].shape
    assert r['rgb_sum'].is_cuda and r['rgb_sum'].dtype == torch.int32 and r['rgb_sum'].shape == (len(r['blocks']), B ** 3, 3)
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in r.items()}


def _same_color(got, want, what=''):
    _same(got, want, what)
    assert got['rgb_sum'].shape == want['rgb_sum'].shape, f'{what}: rgb_sum {got["rgb_sum"].shape} / {want["rgb_sum"].shape}'
    bad = np.nonzero((got['rgb_sum'] != want['rgb_sum']).reshape(-1, 3).any(1))[0]
    assert len(bad) == 0, f'{what}: rgb_sum differs in {len(bad)} voxels, first {bad[0]}: ' \
                          f'{got["rgb_sum"].reshape(-1, 3)[bad[0]]} / {want["rgb_sum"].reshape(-1, 3)[bad[0]]}'
    g, w = np.ascontiguousarray(got['color']), np.ascontiguousarray(want['color'])
    assert g.shape == w.shape and g.dtype == w.dtype == np.float64, f'{what}: color {g.dtype}{g.shape} / {w.dtype}{w.shape}'
    bad = np.nonzero((g.view(np.int64) != w.view(np.int64)).any(1))[0]
    assert len(bad) == 0, f'{what}: color differs in {len(bad)} of {len(g)} points, first {bad[0]}: {g[bad[0]]} / {w[bad[0]]}'


def _check(depth, color, K, poses, voxel, trunc, what='', **kw):
    """the call with colour == the statement, and its geometry == the call without colour"""
    got = _run(depth, color, K, poses, voxel, trunc, **kw)
    want = tsdf_color_ref.tsdf_fragment(depth, color, K, poses, voxel, trunc, **kw)
    _same_color(got, want, what)
    _same(got, _run_plain(depth, K, poses, voxel, trunc, **kw), what + ' (without colour)')
    return got


@functools.lru_cache(maxsize=None)
def _fixture(size, block, stride):
    """(colour, statement) of a fixture of tsdf_cases with noise colours; read-only"""
    s = tsdf_cases.SIZES[size]
    depth, K, poses, _ = tsdf_cases.sequence(size)
    color = tsdf_color_ref.noise_color(depth, seed=block + stride)
    want = tsdf_color_ref.tsdf_fragment(depth, color, K, poses, s['voxel'], s['trunc'], block=block, stride=stride)
    for a in (color,) + tuple(want.values()):
        a.setflags(write=False)
    return color, want


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 4])
@pytest.mark.parametrize('block', [8, 16])
def test_small_equals_statement_and_the_call_without_colour(block, stride):
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    color, want = _fixture('small', block, stride)
    plain = tsdf_cases.statement('small', 0, block, stride)
    assert len(want['xyz']) > 1000 and plain['cross'].any() and want['weight'].max() == s['n_frames'] == len(depth)
    got = _run(depth, color, K, poses, s['voxel'], s['trunc'], block=block, stride=stride)
    _same_color(got, want, f'small block {block} stride {stride}')
    _same(got, _run_plain(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=stride), 'without colour')
    _same(got, plain, 'statement without colour')
    assert got['color'].min() >= 0.0 and got['color'].max() <= 1.0 and len(np.unique(got['color'])) > 1000


# ---- 2. the 256-frame chunks of the cull --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames257(name, block):
    c = tsdf_cases.edge_case(name, block)
    color = tsdf_color_ref.noise_color(c['depth'], seed=257)
    if name == 'frames257_reversed':
        color = np.ascontiguousarray(tsdf_color_ref.noise_color(c['depth'], seed=257)[::-1])    # frame f keeps ITS image
    want = tsdf_color_ref.tsdf_fragment(c['depth'], color, c['K'], c['poses'], c['voxel'], c['trunc'], block=block, stride=c['stride'])
    return c, color, want


@pytest.mark.parametrize('block', [8, 16])
def test_sums_survive_the_chunk_boundary_and_do_not_depend_on_the_frame_order(block):
    out = {}
    for name in ('frames257', 'frames257_reversed'):
        c, color, want = _frames257(name, block)
        assert len(c['depth']) == tsdf_cases.FRAME_CHUNK + 1 and want['weight'].max() > 1
        got = _run(c['depth'], color, c['K'], c['poses'], c['voxel'], c['trunc'], block=block, stride=c['stride'])
        _same_color(got, want, f'{name} block {block}')
        out[name] = got
    # the statement's own premise: the last frame alone (past the chunk boundary) reaches some sum
    c, color, want = _frames257('frames257', block)
    only_last = tsdf_color_ref.tsdf_integrate(want['blocks'], c['depth'][256:], color[256:], c['K'], np.linalg.inv(c['poses'])[256:],
                                              c['voxel'], c['trunc'], 1000.0, 4.5, block)
    assert only_last[1].max() == 1 and only_last[2].max() > 0
    # integer sums are order-free: the same rgb_sum per voxel, block by block
    fwd, rev = out['frames257'], out['frames257_reversed']
    order = {tuple(b): k for k, b in enumerate(rev['blocks'].tolist())}
    assert sorted(order) == sorted(map(tuple, fwd['blocks'].tolist()))
    perm = np.array([order[tuple(b)] for b in fwd['blocks'].tolist()])
    assert np.array_equal(rev['rgb_sum'][perm], fwd['rgb_sum']) and np.array_equal(rev['weight'][perm], fwd['weight'])


# ---- 3. other shapes and inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', [8, 16])
def test_image_size_not_a_multiple_of_the_stride(block):
    from deepglobalregistration_amd import synth
    depth, K, poses, _ = synth.synth_rgbd(3, 2, 81, 61, 70)
    got = _check(depth, tsdf_color_ref.noise_color(depth, 81), K, poses, 0.04, 0.16, '81x61', block=block, stride=4)
    assert len(got['xyz']) > 1000


@pytest.mark.parametrize('block', [8, 16])
def test_one_pixel(block):
    c = tsdf_cases.edge_case('one_pixel', block)
    assert c['depth'].shape[1:] == (1, 1)
    got = _check(c['depth'], tsdf_color_ref.noise_color(c['depth'], 1), c['K'], c['poses'], c['voxel'], c['trunc'], 'one pixel',
                 block=block, stride=c['stride'])
    assert len(got['blocks']) >= 1 and got['rgb_sum'].max() > 0


def test_no_valid_pixel_is_empty_not_an_error():
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    zero = np.zeros_like(depth)
    for block in (8, 16):
        got = _check(zero, tsdf_color_ref.noise_color(depth), K, poses, s['voxel'], s['trunc'], 'all zero', block=block)
        assert got['xyz'].shape == (0, 3) and got['color'].shape == (0, 3) and got['rgb_sum'].shape == (0, block ** 3, 3)
    r = ops.tsdf_fragment(zero, K, poses, s['voxel'], s['trunc'], color=tsdf_color_ref.noise_color(depth))    # without the volume: a dict too
    assert sorted(r) == ['color', 'xyz'] and r['color'].shape == (0, 3) and r['color'].is_cuda


def test_two_calls_agree_and_inputs_may_live_on_the_device():
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    color, want = _fixture('small', 8, 1)
    a = _run(depth, color, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
    d_dev, c_dev = torch.from_numpy(depth.copy()).cuda(), torch.from_numpy(color.copy()).cuda()
    b = _run(d_dev, c_dev, K, poses, s['voxel'], s['trunc'], block=8, stride=1)
    _same_color(a, b, 'second call, inputs on the device')
    _same_color(_run(d_dev, color, K, poses, s['voxel'], s['trunc'], block=8, stride=1), want, 'depth on the device')
    _same_color(_run(depth, c_dev, K, poses, s['voxel'], s['trunc'], block=8, stride=1), want, 'colour on the device')
    r = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1, color=color)              # without the volume
    assert sorted(r) == ['color', 'xyz']
    assert np.array_equal(r['xyz'].cpu().numpy().view(np.int64), want['xyz'].view(np.int64))
    assert np.array_equal(r['color'].cpu().numpy().view(np.int64), want['color'].view(np.int64))
    with pytest.raises(ValueError):                                            # a colour on the host beside a depth on the device
        ops.tsdf_fragment(d_dev, K, poses, s['voxel'], s['trunc'], color=torch.from_numpy(color.copy()))
    plain = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=8, stride=1)                       # no colour: a bare tensor
    assert torch.is_tensor(plain) and torch.equal(plain, r['xyz'])


def test_more_points_and_blocks_than_the_first_guess(monkeypatch):
    """both capacities are exceeded on `large`: the retry carries the colour arrays, and nothing is lost on the way"""
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES['large']
    depth, K, poses, _ = tsdf_cases.sequence('large')
    color, want = _fixture('large', 16, 4)
    monkeypatch.setattr(ops, 'TSDF_FIRST_POINTS', 1000)
    monkeypatch.setattr(ops, 'TSDF_FIRST_BLOCKS', 8)
    assert len(want['blocks']) > 8 and len(want['xyz']) > 1000
    _same_color(_run(depth, color, K, poses, s['voxel'], s['trunc'], block=16, stride=4), want, 'large, small first arrays')


# ---- 4. the mesh --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', [8, 16])
def test_mesh_vertex_colours_are_the_point_colours(block, monkeypatch):
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    color, want = _fixture('small', block, 4)
    vol = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=4, return_volume=True, color=color)
    m = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block, rgb_sum=vol['rgb_sum'])
    assert m['color'].dtype == torch.float64 and m['color'].shape == m['xyz'].shape and len(m['color']) > 1000
    assert torch.equal(m['color'].view(torch.int64), vol['color'].view(torch.int64))
    assert np.array_equal(m['color'].cpu().numpy().view(np.int64), want['color'].view(np.int64))
    plain = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block)
    assert sorted(plain) == ['normal', 'triangles', 'xyz'] and sorted(m) == ['color', 'normal', 'triangles', 'xyz']
    for k in ('xyz', 'normal'):
        assert torch.equal(m[k].view(torch.int64), plain[k].view(torch.int64)), k
    assert torch.equal(m['triangles'], plain['triangles']) and len(m['triangles']) > 1000
    # poisoned memory: the sums of voxels that cannot end a crossing do not reach an output
    lim = np.float32(0.98)
    usable = (want['weight'] >= 1) & (want['tsdf'] >= -lim) & (want['tsdf'] < lim)
    assert not usable.all()
    poisoned = torch.from_numpy(np.where(usable[..., None], want['rgb_sum'], INT32_MIN)).cuda()
    p = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block, rgb_sum=poisoned)
    assert torch.equal(p['color'].view(torch.int64), m['color'].view(torch.int64))
    # the capacity retry carries the colours
    monkeypatch.setattr(ops, 'TSDF_MESH_FIRST_VERTICES', 100)
    monkeypatch.setattr(ops, 'TSDF_MESH_FIRST_TRIANGLES', 100)
    again = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block, rgb_sum=vol['rgb_sum'], normals=False)
    assert torch.equal(again['color'].view(torch.int64), m['color'].view(torch.int64)) and torch.equal(again['triangles'], m['triangles'])
    with pytest.raises(ValueError):
        ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block, rgb_sum=vol['rgb_sum'][:, :, :2])
    # an empty volume
    e = ops.tsdf_mesh(vol['blocks'][:0], vol['tsdf'][:0], vol['weight'][:0], s['voxel'], block=block, rgb_sum=vol['rgb_sum'][:0])
    assert e['color'].shape == (0, 3) and e['xyz'].shape == (0, 3)


# ---- 5. the layers above ------------------------------------------------------------------------------------------------
def test_process_seq_writes_coloured_fragments(tmp_path):
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.eval.formats import read_ply, read_ply_mesh, write_ply, write_ply_mesh
    from deepglobalregistration_amd.util import integration
    depth, K, poses, _ = synth.synth_rgbd(4, 8, 80, 60, 70, sweep_deg=80.0)
    color = synth.synth_color(depth, K, poses, seed=1)
    seq = tmp_path / 'scene' / 'seq-01'
    synth.write_rgbd_sequence(str(seq), depth, K, poses, color=color)
    kw = dict(n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16)
    files = integration.process_seq(str(seq), str(tmp_path / 'points'), color=True, **kw)
    meshes = integration.process_seq(str(seq), str(tmp_path / 'mesh'), mesh=True, color=True, **kw)
    assert [f.rsplit('/', 1)[1] for f in files] == ['fragment-0.ply', 'fragment-1.ply'] == [f.rsplit('/', 1)[1] for f in meshes]
    for k in range(2):
        sl = slice(4 * k, 4 * k + 4)
        want = ops.tsdf_fragment(depth[sl], K, poses[sl], 0.04, 0.16, color=color[sl], return_volume=True)
        xyz, c = want['xyz'].cpu().numpy(), want['color'].cpu().numpy()
        rgb = np.clip(np.rint(255.0 * c), 0, 255).astype(np.uint8)
        assert len(xyz) > 1000 and len(np.unique(rgb, axis=0)) > 100
        got_xyz, got_rgb = read_ply(files[k], return_colors=True)
        assert np.array_equal(got_xyz, xyz) and got_rgb.dtype == np.uint8 and np.array_equal(got_rgb, rgb)
        m = read_ply_mesh(meshes[k])
        wm = ops.tsdf_mesh(want['blocks'], want['tsdf'], want['weight'], 0.04)
        assert np.array_equal(m['xyz'], xyz) and np.array_equal(m['colors'], rgb)
        assert np.array_equal(m['normals'], wm['normal'].cpu().numpy()) and np.array_equal(m['triangles'], wm['triangles'].cpu().numpy())
    # without `color` the files are what the writers give for the plain call: colour files beside the depth change nothing
    plain = integration.process_seq(str(seq), str(tmp_path / 'plain'), **kw)
    plain_mesh = integration.process_seq(str(seq), str(tmp_path / 'plain_mesh'), mesh=True, **kw)
    for k in range(2):
        sl = slice(4 * k, 4 * k + 4)
        vol = ops.tsdf_fragment(depth[sl], K, poses[sl], 0.04, 0.16, return_volume=True)
        wm = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], 0.04)
        write_ply(str(tmp_path / 'a.ply'), vol['xyz'].cpu().numpy())
        write_ply_mesh(str(tmp_path / 'b.ply'), wm['xyz'].cpu().numpy(), wm['triangles'].cpu().numpy(), wm['normal'].cpu().numpy())
        assert open(plain[k], 'rb').read() == open(tmp_path / 'a.ply', 'rb').read()
        assert open(plain_mesh[k], 'rb').read() == open(tmp_path / 'b.ply', 'rb').read()
        assert b'red' not in open(plain[k], 'rb').read(400) and b'red' in open(files[k], 'rb').read(400)
    # the command line
    integration.main([str(tmp_path / 'scene'), str(tmp_path / 'cli'), '--frames', '4', '--voxel', '0.04', '--color', '--mesh'])
    out = tmp_path / 'cli' / 'scene' / 'seq-01'
    assert sorted(p.name for p in out.iterdir()) == ['fragment-0.ply', 'fragment-1.ply']
    assert 'colors' in read_ply_mesh(str(out / 'fragment-0.ply'))
