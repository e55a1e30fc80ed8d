"""Helper of tests/test_gpu_fcgf_wide.py: the FCGF net over every case of tests/fcgf_wide_cases.py in ONE dispatch mode
(fixed per process: DGR_NO_WIDE3), every named tensor in every representation the forward wrote and the kernel of each
of the 23 layers (the keys of tests/aux/layer_trace_dump.py, prefix '<case>/'), to an .npz.

    python tests/aux/fcgf_wide_dump.py OUT.npz [repro]

With `repro` also, as 0 / 1 flags, '<case>/again': a second forward returned the same bytes in OUT and in every tensor;
'<case>/share': so did a forward on a CU-masked stream of a quarter of the compute units (the persistent grid of the
wide kernel is then the share's)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import fcgf_wide_cases as fc   # noqa: E402
from layer_trace_dump import trace   # noqa: E402
from deepglobalregistration_amd import ops, synth   # noqa: E402


def main(path, repro):
    net = ops.NetHandle(synth.synth_state_dict(3, 1, 32, fc.CONV1_KS, fc.SEED), 3, 1, 32, fc.CONV1_KS, True, wide_coarse=True)
    res = {}
    for case in fc.CASES:
        feats = np.ones((len(case.coords), 1), np.float32)
        p = case.name + '/'
        trace(net, case.coords, feats, res, p)
        if not repro:
            continue

        def same_bytes():
            got = {}
            trace(net, case.coords, feats, got, p)
            first = {k for k in res if k.startswith(p) and not k.endswith(('/again', '/share'))}
            return int(got.keys() == first and all(got[k].tobytes() == res[k].tobytes() for k in got))

        res[p + 'again'] = np.array(same_bytes())
        share = ops.partition_stream('cuda', 0, 4)
        assert share is not None
        try:
            with torch.cuda.stream(share):
                res[p + 'share'] = np.array(same_bytes())
        finally:
            torch.cuda.synchronize()
            ops.partition_stream('cuda', 0, 1)
    np.savez(path, **res)


if __name__ == '__main__':
    main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == 'repro')
