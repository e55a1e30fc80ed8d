"""Helper of tests/test_gpu_layer_trace.py: in ONE arithmetic mode (fixed per process: DGR_EXACT_F32, DGR_OS_LISTS) run
every net of tests/aux/layer_trace_inputs.py over its clouds and write, per forward, every named tensor in every
representation the forward wrote (NetHandle.tensor) and the kernel that ran each of the 23 layers, to an .npz.

Keys: '<net>/<cloud>/<tensor>/<repr>' arrays, '<net>/<cloud>/kinds', '<net>/<cloud>/missing' (the '<tensor>/<repr>'
pairs the library refused with "did not write").  With a second argument 'wide', the wide-range checkpoint of
tests/aux/split_f64_inputs.py instead (nets 'wr3', 'wr6', cloud 'W')."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import layer_trace_inputs as inp   # noqa: E402
from deepglobalregistration_amd import ops   # noqa: E402

TENSORS = ('T1', 'Y1', 'S1', 'T2', 'Y2', 'S2', 'T4', 'Y4', 'S4', 'T8', 'Y8', 'S8', 'U4', 'V4', 'S4T', 'U2', 'V2', 'S2T',
           'U1', 'V1', 'S1T', 'H', 'CAT4', 'CAT2', 'CAT1')
REPRS = ('f32', 'amax', 'split_planes', 'split_scale', 'dense_split')


def trace(net, coords, feats, res, prefix):
    ops.set_profiling('cuda', True)
    out = net.forward(torch.from_numpy(coords).cuda(), torch.from_numpy(feats).cuda())
    res[prefix + 'kinds'] = np.array(ops.conv_launch_kinds('cuda'))
    ops.set_profiling('cuda', False)
    res[prefix + 'OUT/f32'] = out.cpu().numpy()
    missing = []
    for t in TENSORS:
        for r in REPRS:
            try:
                res[prefix + f'{t}/{r}'] = net.tensor(t, r)
            except (RuntimeError, ValueError) as e:
                if 'did not write' not in str(e):
                    raise
                missing.append(f'{t}/{r}')
    res[prefix + 'missing'] = np.array(missing)
    # what the entry hands back for the output buffer is what the forward returned
    assert np.array_equal(net.tensor('OUT', 'f32'), res[prefix + 'OUT/f32'])


def main(path, what):
    res = {}
    if what == 'wide':
        import split_f64_inputs as wr_inp
        wr = wr_inp.wide_range_case()
        net = ops.NetHandle(wr['sd3'], 3, 1, 32, 5, True)
        trace(net, wr['c3'], np.ones((len(wr['c3']), 1), np.float32), res, 'wr3/W/')
        net = ops.NetHandle(wr['sd6'], 6, 6, 1, 3, False)
        trace(net, wr['c6'], wr['f6'], res, 'wr6/W/')
    else:
        clouds = inp.clouds()
        for name, (D, cin, cout, ks, norm, _, cl) in inp.NETS.items():
            net = ops.NetHandle(inp.state_dict(name), D, cin, cout, ks, norm)   # once per process, reused over the clouds
            for c in cl:
                trace(net, clouds[c], inp.feats(name, c, len(clouds[c])), res, f'{name}/{c}/')
            # a later call on the context reuses the workspace: the read-back refuses instead of returning stale rows
            other = ops.NetHandle(inp.state_dict(name), D, cin, cout, ks, norm)
            c = cl[0]
            other.forward(torch.from_numpy(clouds[c]).cuda(), torch.from_numpy(inp.feats(name, c, len(clouds[c]))).cuda())
            try:
                net.tensor('T1', 'f32')
                raise AssertionError('stale read-back was not refused')
            except (RuntimeError, ValueError) as e:
                assert 'gone' in str(e), e
    np.savez(path, **res)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else 'trace')
