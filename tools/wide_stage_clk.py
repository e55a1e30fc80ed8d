"""Where a phase of the wide 6-D conv kernel (conv_wide.hip) goes, per shape and role: a build with -DDGR_WIDE_STAGE_CLK
(make EXTRA=-DDGR_WIDE_STAGE_CLK, library given by DGR_HIP_LIB) sums, per wave, the time spent between reaching and
leaving the phase barrier, the compute waves' wait for their weight fragments and the requesters' time inside land() and
rings().

    python tools/wide_stage_clk.py layers [SHARES]   every wide layer of one 6-D forward (the workload of layer_bench.py),
                                                     re-run alone on share 0 of SHARES (1, 2, 4) shares of the CUs
    python tools/wide_stage_clk.py bench [ARGS...]   inside one run of bench.py (default arguments: the timed configuration,
                                                     --full --no-parity --no-cpu-baseline --no-exact-leg): all contexts
                                                     and all launches of the run summed per shape
"""
import contextlib, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from deepglobalregistration_amd import ops, synth, _lib

SHAPES = ['<64,1,2>', '<64,1,1>', '<128,1,1>', '<256,1,1>', '<128,2,1>', '<256,2,1>']   # dgr_wide_shape_id
HEAD = ('shape      launches-x-wgs  phases/wg  us/phase | compute: barrier  weights | requesters: barrier  land  rings | '
        'storers: barrier | shader MHz')


def table(reset):
    buf = (C.c_ulonglong * 96)()
    if _lib.load().dgr_debug_wide_stage_clk(buf, int(reset)) != 0:
        raise RuntimeError('dgr_debug_wide_stage_clk failed')
    return [[int(buf[16 * i + j]) for j in range(16)] for i in range(6)]


def rows(tab, only=None):
    for name, c in zip(SHAPES, tab):
        if not c[3] or (only and name != only):
            continue
        wgs = c[3] // 4                       # four compute waves per workgroup
        mhz = c[13] / max(c[14], 1) * 100.0   # shader clock ticks per 10-ns wall tick
        pct = lambda x, life: 100.0 * x / max(life, 1)
        print(f'{name:10s} {wgs:14d} {c[12] / max(wgs, 1):10.1f} {c[14] * 0.01 / max(c[12], 1):9.3f} | '
              f'{pct(c[0], c[2]):15.1f}% {pct(c[1], c[2]):7.1f}% | {pct(c[4], c[7]):18.1f}% {pct(c[5], c[7]):4.1f}% '
              f'{pct(c[6], c[7]):5.1f}% | {pct(c[9], c[10]):15.1f}% | {mhz:8.0f}')


def layers(shares):
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    share = ops.partition_stream('cuda', 0, shares)
    with (torch.cuda.stream(share) if share is not None else contextlib.nullcontext()):
        dgr = DeepGlobalRegistration({'weights': synth.synth_checkpoint(0)}, torch.device('cuda'))
        x0, x1, T = synth.synth_pair(0, 50000)
        p0, c0, f0 = dgr.preprocess(x0); p1, c1, f1 = dgr.preprocess(x1)
        gt = torch.from_numpy(synth.gt_correspondences(p0.cpu().numpy(), p1.cpu().numpy(), T, 0.05)).cuda()
        idx1 = torch.where(gt >= 0, gt, (torch.arange(len(gt), device=gt.device) * 7919) % len(p1))
        c6, f6 = ops.inlier_inputs(c0, p0, c1, p1, idx1, 'coords')
        net = dgr.inlier_model._handle()
        ops.set_profiling('cuda', True)
        net.forward(c6, f6)
        kinds = ops.conv_launch_kinds('cuda')
        ops.set_profiling('cuda', False)
        st = net.layer_stats()
        print(f'# one 50k-point pair, every wide layer re-run 5 times alone on share 0 of {shares}; percentages = of the role\'s life')
        print('layer cin cout   pairs  gemm_us | ' + HEAD)
        for li, k in enumerate(kinds):
            if not k.startswith('sparse_conv_wide'):
                continue
            table(True)
            g, _ = net.rerun_layer(li, 5)
            torch.cuda.synchronize()
            print(f"L{li:2d} {st[li]['cin']:4d} {st[li]['cout']:4d} {st[li]['pairs']:8d} {g * 1e3:8.1f} | ", end='')
            rows(table(False), k[len('sparse_conv_wide_f16x2'):].replace(' ', ''))


def bench(args):
    import bench as bench_py
    sys.argv = ['bench.py'] + (args or ['--gpus', '1', '--full', '--no-parity', '--no-cpu-baseline', '--no-exact-leg'])
    table(True)
    try:
        bench_py.main()
    except SystemExit:
        pass
    torch.cuda.synchronize()
    print('# inside bench.py ' + ' '.join(sys.argv[1:]) + ': all contexts, all launches')
    print(HEAD)
    rows(table(False))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'bench':
        bench(sys.argv[2:])
    else:
        layers(int(sys.argv[2]) if len(sys.argv) > 2 else 4)
