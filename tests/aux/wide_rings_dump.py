"""Helper of tests/test_gpu_wide_rings.py: every case of tests/wide_rings_cases.py through every shape of the wide conv
kernel (dgr_debug_conv_layer), in ONE arithmetic mode (fixed when the library builds a net: DGR_EXACT_F32), to an .npz.

    python tests/aux/wide_rings_dump.py OUT.npz [repro]

`<case>/<cin>x<cout>`: the layer's output on the plain stream (the whole GPU).  With `repro` also, as 0 / 1 flags,
`.../again`: a second run on the plain stream returned the same bytes; `.../share`: so did a run on a CU-masked stream of a
quarter of the compute units (the context's persistent kernels then size themselves for 64 compute units)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import wide_rings_cases as wc   # noqa: E402
from deepglobalregistration_amd import ops, synth   # noqa: E402


def main(path, repro):
    net = ops.NetHandle(synth.synth_state_dict(6, 6, 1, 3, wc.SEED), 6, 6, 1, 3, False)
    res = {}

    def run_all(store):
        for case in wc.CASES:
            for cin, cout, layer, _, _ in wc.SHAPES:
                y = net.debug_conv_layer(layer, case.coords, case.features(cin), 0).cpu().numpy()
                store(f'{case.name}/{cin}x{cout}', y)

    run_all(lambda k, y: res.__setitem__(k, y))
    if repro:
        run_all(lambda k, y: res.__setitem__(k + '/again', np.array(int(y.tobytes() == res[k].tobytes()))))
        share = ops.partition_stream('cuda', 0, 4)
        assert share is not None
        try:
            with torch.cuda.stream(share):
                run_all(lambda k, y: res.__setitem__(k + '/share', np.array(int(y.tobytes() == res[k].tobytes()))))
        finally:
            torch.cuda.synchronize()
            ops.partition_stream('cuda', 0, 1)
    np.savez(path, **res)


if __name__ == '__main__':
    main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == 'repro')
