"""What the GPU tests of `ops.tsdf_fragment` share (tests/test_gpu_tsdf.py, tests/test_gpu_tsdf_edges.py): one call with the
volume returned, and the comparison with the numpy statement (tests/tsdf_ref.py) -- EXACT equality of `blocks` and `weight`
and of the bits of `tsdf` and `xyz`.  No tolerance."""
import numpy as np
import torch

import tsdf_ref


def run(depth, K, poses, voxel, trunc, **kw):
    from deepglobalregistration_amd import ops
    r = ops.tsdf_fragment(depth, K, poses, voxel, trunc, return_volume=True, **kw)
    assert r['xyz'].is_cuda and r['xyz'].dtype == torch.float64 and r['blocks'].dtype == torch.int32
    assert r['tsdf'].dtype == torch.float32 and r['weight'].dtype == torch.int32
    B = kw.get('block', 16)
    assert r['xyz'].shape[1:] == (3,) and r['blocks'].shape[1:] == (3,)
    assert r['tsdf'].shape == (len(r['blocks']), B ** 3) and r['weight'].shape == r['tsdf'].shape
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in r.items()}      # (`kept`, `n_blocks`: integers)


def same(got, want, what=''):
    for k, bits in (('blocks', np.int32), ('weight', np.int32), ('tsdf', np.int32), ('xyz', np.int64)):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f'{what}: {k} is {g.dtype}{g.shape}, statement {w.dtype}{w.shape}'
        bad = np.nonzero((g.view(bits) != w.view(bits)).reshape(len(g), int(np.prod(g.shape[1:]))).any(1))[0]
        assert len(bad) == 0, f'{what}: {k} differs in {len(bad)} of {len(g)} rows, first {bad[0]}: {g[bad[0]]} / {w[bad[0]]}'


def check(depth, K, poses, voxel, trunc, what='', **kw):
    got = run(depth, K, poses, voxel, trunc, **kw)
    want = tsdf_ref.tsdf_fragment(depth, K, poses, voxel, trunc, **kw)
    same(got, want, what)
    return got
