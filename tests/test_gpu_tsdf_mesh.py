"""GPU: `ops.tsdf_mesh` (csrc/tsdfmesh.hip) against its numpy statement (tests/tsdf_mesh_ref.py), and the layers above it
(`util.integration.process_seq(mesh=True)`, mesh files into `DeepGlobalRegistration.extract_fragments`).

`xyz`, `normal` and `triangles` are compared for EXACT equality (the floats by their bits): both sides perform the same
correctly rounded float64 operations in the same order, without fused multiply-add.  No tolerance and no excluded case."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_cases
import tsdf_mesh_ref as ref

pytestmark = pytest.mark.gpu


def _run(blocks, tsdf, weight, voxel, block, min_weight=1, normals=True):
    from deepglobalregistration_amd import ops
    dev = torch.device('cuda')
    r = ops.tsdf_mesh(torch.from_numpy(np.ascontiguousarray(blocks, np.int32).reshape(-1, 3)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(tsdf, np.float32).reshape(-1, block ** 3)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(weight, np.int32).reshape(-1, block ** 3)).to(dev),
                      voxel, block=block, min_weight=min_weight, normals=normals)
    assert set(r) == ({'xyz', 'normal', 'triangles'} if normals else {'xyz', 'triangles'})
    assert all(v.is_cuda for v in r.values())
    assert r['xyz'].dtype == torch.float64 and r['xyz'].shape[1:] == (3,)
    assert r['triangles'].dtype == torch.int32 and r['triangles'].shape[1:] == (3,)
    if normals:
        assert r['normal'].dtype == torch.float64 and r['normal'].shape == r['xyz'].shape
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(got, want, what=''):
    """want = the statement's (xyz, normal, tri)"""
    for k, w, bits in (('xyz', want[0], np.int64), ('normal', want[1], np.int64), ('triangles', want[2], np.int32)):
        if k not in got:
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f'{what}: {k} is {g.dtype}{g.shape}, statement {w.dtype}{w.shape}'
        bad = np.nonzero((g.view(bits) != w.view(bits)).any(1))[0]
        assert len(bad) == 0, f'{what}: {k} differs in {len(bad)} of {len(g)} rows, first {bad[0]}: {g[bad[0]]} / {w[bad[0]]}'


def _check(blocks, tsdf, weight, voxel, block, min_weight=1, what=''):
    got = _run(blocks, tsdf, weight, voxel, block, min_weight)
    want = ref.tsdf_mesh(blocks, tsdf, weight, voxel, block, min_weight)
    _same(got, want, what)
    return got


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,block', [('small', 8), ('small', 16), ('large', 8), ('large', 16)])
def test_fixture_equals_statement(size, block):
    from deepglobalregistration_amd import ops
    s = tsdf_cases.SIZES[size]
    depth, K, poses, _ = tsdf_cases.sequence(size)
    vol = ops.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=4, return_volume=True)
    r = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], s['voxel'], block=block)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    want = ref.tsdf_mesh(vol['blocks'].cpu().numpy(), vol['tsdf'].cpu().numpy(), vol['weight'].cpu().numpy(), s['voxel'], block, 1)
    assert len(want[0]) > 1000 and len(want[2]) > len(want[0])
    _same(got, want, f'{size} block {block}')
    # vertex k of the mesh is point k of the fragment
    assert np.array_equal(got['xyz'].view(np.int64), vol['xyz'].cpu().numpy().view(np.int64))


# ---- 2. hand-made volumes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('min_weight', [1, 2])
def test_noise_volume_with_random_weights(min_weight):
    blocks, tsdf, _ = ref.noise_volume()
    # weights 0, 1, 2 with shares 5 / 10 / 85 %: with min_weight 2 a quarter of the cells still have eight usable corners
    weight = np.random.default_rng(5).choice(3, tsdf.shape, p=[0.05, 0.1, 0.85]).astype(np.int32)
    got = _check(blocks, tsdf, weight, 0.01, 8, min_weight, f'noise, min_weight {min_weight}')
    assert len(got['triangles']) > 1000 and not ref.is_closed(got['triangles'])


def test_noise_volume_all_valid_is_closed():
    blocks, tsdf, weight = ref.noise_volume()
    got = _check(blocks, tsdf, weight, 0.01, 8, 1, 'noise')
    assert ref.is_closed(got['triangles'])


def test_sphere_whole_with_a_block_removed_and_shuffled():
    blocks, tsdf, weight = ref.sphere_volume()
    whole = _check(blocks, tsdf, weight, 1.0, 8, 1, 'sphere')
    assert ref.is_closed(whole['triangles'])
    keep = np.arange(8) != 5
    part = _check(blocks[keep], tsdf[keep], weight[keep], 1.0, 8, 1, 'sphere without block 5')
    assert 0 < len(part['triangles']) < len(whole['triangles'])
    perm = np.random.default_rng(1).permutation(8)
    mixed = _check(blocks[perm], tsdf[perm], weight[perm], 1.0, 8, 1, 'sphere shuffled')
    assert not np.array_equal(mixed['xyz'], whole['xyz'])

    def as_set(m):
        return sorted(tuple(np.concatenate([m['xyz'][t].reshape(-1), m['normal'][t].reshape(-1)]).tolist()) for t in m['triangles'])
    assert as_set(mixed) == as_set(whole)


def test_sphere_in_blocks_of_16():
    blocks = ref.grid_blocks(2, 2, 2, (-1, -1, -1))
    c, R, tr = np.array([0.31, -0.27, 0.13]), 11.3, 4.0
    tsdf = ref.fill_volume(blocks, 16, lambda i: np.clip((np.linalg.norm(i + 0.5 - c, axis=1) - R) / tr, -1.0, 1.0))
    got = _check(blocks, tsdf, np.ones(tsdf.shape, np.int32), 0.5, 16, 1, 'sphere 16')
    assert ref.is_closed(got['triangles'])


@pytest.mark.parametrize('block', [8, 16])
def test_single_block(block):
    rng = np.random.default_rng(block)
    tsdf = np.clip(rng.standard_normal((1, block ** 3)) * 0.6, -1, 1).astype(np.float32)
    weight = rng.integers(0, 3, tsdf.shape).astype(np.int32)
    got = _check(np.array([[3, -2, 7]], np.int32), tsdf, weight, 0.02, block, 1, 'one block')
    assert len(got['triangles']) > 0


def test_empty_list_and_all_positive_volume():
    for block in (8, 16):
        V = block ** 3
        got = _check(np.zeros((0, 3), np.int32), np.zeros((0, V), np.float32), np.zeros((0, V), np.int32), 0.01, block, 1, 'empty')
        assert got['xyz'].shape == (0, 3) and got['normal'].shape == (0, 3) and got['triangles'].shape == (0, 3)
        blocks = ref.grid_blocks(2, 2, 1)
        got = _check(blocks, np.full((4, V), 0.5, np.float32), np.ones((4, V), np.int32), 0.01, block, 1, 'all positive')
        assert got['xyz'].shape == (0, 3) and got['triangles'].shape == (0, 3)


@pytest.mark.parametrize('block', [8, 16])
def test_planted_limits_and_zeros_on_both_sides_of_block_borders(block):
    """0.98f and -0.98f (the one unusable, the other usable), -0.0f and 0.0f (neither negative) in the first and the last
    layer of every block on every axis, so that they meet across the borders"""
    rng = np.random.default_rng(11)
    blocks = ref.grid_blocks(2, 2, 2, (-1, 0, 3))
    tsdf = np.clip(rng.standard_normal((8, block ** 3)) * 0.5, -0.97, 0.97).astype(np.float32)
    lc = np.stack([np.arange(block ** 3) % block, (np.arange(block ** 3) // block) % block, np.arange(block ** 3) // block ** 2], 1)
    border = ((lc == 0) | (lc == block - 1)).any(1)
    planted = np.array([0.98, -0.98, -0.0, 0.0, np.nextafter(np.float32(0.98), np.float32(0)), np.nextafter(np.float32(-0.98), np.float32(-1))],
                       np.float32)
    pick = rng.integers(0, 2 * len(planted), (8, int(border.sum())))
    tsdf[:, border] = np.where(pick < len(planted), planted[pick % len(planted)], tsdf[:, border])
    assert (np.signbit(tsdf) & (tsdf == 0)).any() and (tsdf == np.float32(0.98)).any() and (tsdf == np.float32(-0.98)).any()
    weight = np.ones(tsdf.shape, np.int32)
    got = _check(blocks, tsdf, weight, 0.01, block, 1, 'planted')
    assert len(got['triangles']) > 100


def test_negative_block_coordinates_and_the_largest_ones():
    L = 2 ** 26
    blocks = np.array([[L - 2, -L, 5], [L - 1, -L, 5], [L - 1, -L + 1, 5], [-3, -4, -5], [-2, -4, -5], [-2, -4, -6]], np.int32)
    rng = np.random.default_rng(3)
    for block in (8, 16):
        tsdf = np.clip(rng.standard_normal((len(blocks), block ** 3)) * 0.5, -0.97, 0.97).astype(np.float32)
        got = _check(blocks, tsdf, np.ones(tsdf.shape, np.int32), 0.008, block, 1, 'far blocks')
        assert len(got['triangles']) > 100


# ---- 3. calls -------------------------------------------------------------------------------------------------------------
def test_without_normals_and_two_calls_agree():
    blocks, tsdf, _ = ref.noise_volume(seed=2)
    weight = np.random.default_rng(6).integers(0, 3, tsdf.shape).astype(np.int32)
    a = _run(blocks, tsdf, weight, 0.01, 8, 1)
    b = _run(blocks, tsdf, weight, 0.01, 8, 1)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = _run(blocks, tsdf, weight, 0.01, 8, 1, normals=False)
    assert c['xyz'].tobytes() == a['xyz'].tobytes() and c['triangles'].tobytes() == a['triangles'].tobytes()


def _raw_call(lib, ctx, blocks, tsdf, weight, block, voxel, min_weight, xyz, normal, max_v, tri, max_t):
    from deepglobalregistration_amd import _lib
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    rc = lib.dgr_tsdf_mesh(ctx, _lib.ptr(blocks), 0 if blocks is None else len(blocks), _lib.ptr(tsdf), _lib.ptr(weight), block,
                           voxel, min_weight, _lib.ptr(xyz), _lib.ptr(normal), max_v, _lib.ptr(tri), max_t, C.byref(nv),
                           C.byref(nt), _lib.stream_ptr(0))
    torch.cuda.synchronize()
    return rc, nv.value, nt.value


def test_enomem_protocol_writes_nothing_past_either_array_and_the_wrapper_regrows(monkeypatch):
    from deepglobalregistration_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    ctx = _lib.get_ctx(dev)
    b, t, w = ref.sphere_volume()
    want = ref.tsdf_mesh(b, t, w, 1.0, 8, 1)
    P, T = len(want[0]), len(want[2])
    blocks, tsdf, weight = (torch.from_numpy(a).to(dev) for a in (b, t, w))
    PAD = 16

    def buffers():
        return (torch.full((P + PAD, 3), -77.0, dtype=torch.float64, device=dev),
                torch.full((P + PAD, 3), -77.0, dtype=torch.float64, device=dev),
                torch.full((T + PAD, 3), -77, dtype=torch.int32, device=dev))
    for max_v, max_t in ((P - 1, T), (P, T - 1), (0, 0)):
        xyz, normal, tri = buffers()
        rc, nv, nt = _raw_call(lib, ctx, blocks, tsdf, weight, 8, 1.0, 1, xyz, normal, max_v, tri, max_t)
        assert rc == _lib.DGR_ENOMEM and (nv, nt) == (P, T), (rc, nv, nt)
        assert b'vertices' in lib.dgr_last_error()
        assert (xyz == -77).all() and (normal == -77).all() and (tri == -77).all()      # nothing written at all
    xyz, normal, tri = buffers()
    rc, nv, nt = _raw_call(lib, ctx, blocks, tsdf, weight, 8, 1.0, 1, xyz, normal, P, tri, T)
    assert rc == _lib.DGR_OK and (nv, nt) == (P, T)
    assert (xyz[P:] == -77).all() and (normal[P:] == -77).all() and (tri[T:] == -77).all()  # the canaries behind both arrays
    _same({'xyz': xyz[:P].cpu().numpy(), 'normal': normal[:P].cpu().numpy(), 'triangles': tri[:T].cpu().numpy()}, want, 'exact fit')
    # the wrapper: first arrays too small for both, one more call
    monkeypatch.setattr(ops, 'TSDF_MESH_FIRST_VERTICES', 100)
    monkeypatch.setattr(ops, 'TSDF_MESH_FIRST_TRIANGLES', 100)
    _same(_run(b, t, w, 1.0, 8, 1), want, 'regrown')
    monkeypatch.setattr(ops, 'TSDF_MESH_FIRST_VERTICES', 1 << 20)
    _same(_run(b, t, w, 1.0, 8, 1), want, 'triangles regrown')


def test_argument_errors_are_reported_not_launched():
    from deepglobalregistration_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device('cuda:0')
    ctx = _lib.get_ctx(dev)
    b, t, w = ref.sphere_volume()
    blocks, tsdf, weight = (torch.from_numpy(a).to(dev) for a in (b, t, w))
    xyz = torch.zeros((4096, 3), dtype=torch.float64, device=dev)
    tri = torch.zeros((8192, 3), dtype=torch.int32, device=dev)
    good = dict(blocks=blocks, tsdf=tsdf, weight=weight, block=8, voxel=1.0, min_weight=1, xyz=xyz, normal=None, max_v=4096,
                tri=tri, max_t=8192)
    assert _raw_call(lib, ctx, **good)[0] == _lib.DGR_OK
    bad = [dict(tsdf=None), dict(weight=None), dict(xyz=None), dict(tri=None), dict(block=4), dict(block=12), dict(block=32),
           dict(min_weight=0), dict(min_weight=-1), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float('inf')),
           dict(voxel=float('nan')), dict(max_v=-1), dict(max_t=-1)]
    for change in bad:
        rc, _, _ = _raw_call(lib, ctx, **dict(good, **change))
        assert rc == _lib.DGR_EINVAL, change
        assert lib.dgr_last_error().startswith(b'dgr_tsdf_mesh:'), change
    nv, nt = C.c_int64(0), C.c_int64(0)
    args = (_lib.ptr(blocks), 8, _lib.ptr(tsdf), _lib.ptr(weight), 8, 1.0, 1, _lib.ptr(xyz), None, 4096, _lib.ptr(tri), 8192)
    assert lib.dgr_tsdf_mesh(None, *args, C.byref(nv), C.byref(nt), None) == _lib.DGR_EINVAL
    assert lib.dgr_tsdf_mesh(ctx, *args, None, C.byref(nt), None) == _lib.DGR_EINVAL
    assert lib.dgr_tsdf_mesh(ctx, *args, C.byref(nv), None, None) == _lib.DGR_EINVAL
    assert lib.dgr_tsdf_mesh(ctx, None, 8, *args[2:], C.byref(nv), C.byref(nt), None) == _lib.DGR_EINVAL
    assert lib.dgr_tsdf_mesh(ctx, _lib.ptr(blocks), -1, *args[2:], C.byref(nv), C.byref(nt), None) == _lib.DGR_EINVAL
    # found on the device, reported at the synchronisation as an error with nothing written
    for coords, word in ((2 ** 26, b'outside'), (-2 ** 26 - 1, b'outside')):
        far = blocks.clone()
        far[3, 1] = coords
        xyz.fill_(-5.0)
        rc, _, _ = _raw_call(lib, ctx, **dict(good, blocks=far))
        assert rc == _lib.DGR_EINVAL and word in lib.dgr_last_error()
        assert (xyz == -5).all()
    twice = blocks.clone()
    twice[6] = twice[2]
    rc, _, _ = _raw_call(lib, ctx, **dict(good, blocks=twice))
    assert rc == _lib.DGR_EINVAL and b'twice' in lib.dgr_last_error()
    with pytest.raises(ValueError, match='twice'):
        ops.tsdf_mesh(twice, tsdf, weight, 1.0, block=8)
    # ... also when the two copies lie in different workgroups of the insertion (256 list entries each): 320 unobserved
    # blocks along x are an empty mesh, the same list with entry 300 = entry 0 is an error
    row = torch.zeros((320, 3), dtype=torch.int32, device=dev)
    row[:, 0] = torch.arange(320, dtype=torch.int32, device=dev)
    empty = dict(good, blocks=row, tsdf=torch.zeros((320, 8, 8, 8), dtype=torch.float32, device=dev),
                 weight=torch.zeros((320, 8, 8, 8), dtype=torch.int32, device=dev))
    assert _raw_call(lib, ctx, **empty) == (_lib.DGR_OK, 0, 0)
    row[300] = row[0]
    rc, _, _ = _raw_call(lib, ctx, **empty)
    assert rc == _lib.DGR_EINVAL and b'twice' in lib.dgr_last_error()
    # the wrapper's own checks: nothing reaches the library
    for kw, args3 in ((dict(block=4), None), (dict(min_weight=0), None), (dict(voxel_length=0.0), None),
                      (dict(voxel_length=float('nan')), None), (dict(block=16), None), ({}, (blocks.long(), tsdf, weight)),
                      ({}, (blocks, tsdf.double(), weight)), ({}, (blocks, tsdf, weight.long())),
                      ({}, (blocks[:4], tsdf, weight)), ({}, (blocks.cpu(), tsdf, weight)), ({}, (b, t, w))):
        a = args3 or (blocks, tsdf, weight)
        call = dict(dict(voxel_length=1.0, block=8), **kw)
        with pytest.raises(ValueError):
            ops.check_tsdf_mesh_args(*a, **call)
        with pytest.raises(ValueError):
            ops.tsdf_mesh(*a, **call)


# ---- 4. the layers above --------------------------------------------------------------------------------------------------
def test_process_seq_writes_meshes_on_the_points_only_vertices(tmp_path):
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.eval.formats import read_ply, read_ply_mesh
    from deepglobalregistration_amd.util import integration
    from helpers import harness_dgr
    depth, K, poses, _ = synth.synth_rgbd(4, 8, 80, 60, 70, sweep_deg=80.0)
    seq = tmp_path / 'scene' / 'seq-01'
    synth.write_rgbd_sequence(str(seq), depth, K, poses)
    args = dict(n_frames_per_fragment=4, voxel_length=0.04, sdf_trunc=0.16)
    plain = integration.process_seq(str(seq), str(tmp_path / 'points'), **args)
    files = integration.process_seq(str(seq), str(tmp_path / 'mesh'), mesh=True, **args)
    assert [f.rsplit('/', 1)[1] for f in files] == ['fragment-0.ply', 'fragment-1.ply']
    clouds = []
    for k, (f, p) in enumerate(zip(files, plain)):
        m = read_ply_mesh(f)
        assert len(m['xyz']) > 1000 and m['xyz'].tobytes() == read_ply(p).tobytes() and read_ply(f).tobytes() == m['xyz'].tobytes()
        vol =ops.tsdf_fragment(depth[4 * k:4 * k + 4], K, poses[4 * k:4 * k + 4], 0.04, 0.16, return_volume=True)
        want = ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], 0.04)
        assert np.array_equal(m['triangles'], want['triangles'].cpu().numpy()) and len(m['triangles']) > 1000
        assert m['normals'].tobytes() == want['normal'].cpu().numpy().tobytes()
        clouds.append(read_ply(f))
    integration.main([str(tmp_path / 'scene'), str(tmp_path / 'cli'), '--frames', '4', '--voxel', '0.04', '--mesh'])
    cli = tmp_path / 'cli' / 'scene' / 'seq-01'
    assert sorted(p.name for p in cli.iterdir()) == ['fragment-0.ply', 'fragment-1.ply']
    assert 'element face' in open(cli / 'fragment-0.ply', 'rb').read(400).decode('latin1')
    ck = synth.synth_checkpoint(seed=0, voxel_size=0.05, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))
    bank = dgr.extract_fragments(clouds)
    assert len(bank) == 2 and all(len(bank.xyz_of(i)) > 100 for i in range(2))
