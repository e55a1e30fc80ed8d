"""Device-event times of `ops.tsdf_fragment` (csrc/tsdf.hip) on a fragment-sized input beside the numpy statement of the
same arithmetic on the host (tests/tsdf_ref.py): a `synth_rgbd(0)` sequence of 50 frames at 640 x 480 (focal 525) in which
the camera turns through 120 degrees, 8-mm voxels, 4-cm truncation, stride 4, with blocks of 8^3 and of 16^3 voxels.

Per block size: median / min / max of `--reps` whole calls after 3 warm-up calls (everything between the two events:
upload of the poses, tables, allocation, integration, extraction and both host synchronisations; the depth frames are on
the device already, as they would be after one upload per fragment).  Beside the times: blocks, voxels, points; the (block,
frame) pairs the cull kept; voxel-frame updates per second counting every pair (`updates_per_s_nominal`: what the
statement visits) and counting the kept pairs only (`updates_per_s_kept`: what the kernel visits); the compulsory bytes
(depth in, volume out: 2 F H W + 8 voxels, + 24 per point) and those bytes per second as a share of the 8 TB/s HBM peak.

The numpy statement is run ONCE per block size on the host's wall clock (a single, cold run: an order of magnitude, not a
median) on the first `--ref-frames` frames (default: all 50; fewer where the host is slow -- the library is then timed on
the same frames too), and the two results are compared for exact equality.  The one condition: on those frames the
library's call is not slower than the statement on the same box.

    python tools/tsdf_bench.py [--reps 20] [--ref-frames 50] [--out profiles/tsdf_bench.json] [--commit HASH]
    python tools/tsdf_bench.py --profile-only     # three calls per block size and nothing else: what a kernel trace wraps
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
HBM_PEAK = 8e12   # bytes / s
WIDTH, HEIGHT, FOCAL, FRAMES, SWEEP, VOXEL, TRUNC, STRIDE = 640, 480, 525.0, 50, 120.0, 0.008, 0.04, 4


def measure(ops, depth_dev, K, poses, block, reps):
    F = len(poses)
    r = ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE, return_stats=True)
    nb, P, kept = r['n_blocks'], len(r['xyz']), r['kept']
    del r
    from voxel_mean_bench import timed
    ms = timed(lambda: ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE), reps)
    voxels = nb * block ** 3
    nbytes = 2 * F * HEIGHT * WIDTH + 8 * voxels + 24 * P
    s = ms['median_ms'] * 1e-3
    return {'frames': F, 'block': block, 'blocks': nb, 'voxels': voxels, 'points': P, 'block_frames': nb * F,
            'block_frames_kept': kept, 'kept_share': kept / max(nb * F, 1), 'ms': ms,
            'updates_per_s_nominal': voxels * F / s, 'updates_per_s_kept': kept * block ** 3 / s,
            'compulsory_bytes': nbytes, 'compulsory_bytes_per_s': nbytes / s, 'share_of_hbm_peak': nbytes / s / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ref-frames', type=int, default=FRAMES)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--profile-only', action='store_true')
    a = ap.parse_args()
    from deepglobalregistration_amd import ops, synth
    import tsdf_ref
    from voxel_mean_bench import commit_stamp
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_bench measures on the GPU; there is nothing to time without one')
    depth, K, poses, _ = synth.synth_rgbd(0, FRAMES, WIDTH, HEIGHT, FOCAL, sweep_deg=SWEEP)
    depth_dev = torch.from_numpy(depth).cuda()
    if a.profile_only:
        for block in (8, 16):
            for _ in range(3):
                ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE)
        torch.cuda.synchronize()
        return
    out = {'commit': a.commit or commit_stamp(), 'device': torch.cuda.get_device_name(0), 'reps': a.reps,
           'input': {'width': WIDTH, 'height': HEIGHT, 'focal': FOCAL, 'frames': FRAMES, 'sweep_deg': SWEEP, 'voxel_length': VOXEL, 'sdf_trunc': TRUNC,
                     'stride': STRIDE, 'valid_pixels_share': float((depth > 0).mean())},
           'hbm_peak_bytes_per_s': HBM_PEAK, 'ref_frames': a.ref_frames}
    ok = True
    for block in (8, 16):
        full = measure(ops, depth_dev, K, poses, block, a.reps)
        n = a.ref_frames
        t0 = time.perf_counter()
        want = tsdf_ref.tsdf_fragment(depth[:n], K, poses[:n], VOXEL, TRUNC, block=block, stride=STRIDE)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = ops.tsdf_fragment(depth_dev[:n], K, poses[:n], VOXEL, TRUNC, block=block, stride=STRIDE, return_volume=True)
        for key in ('blocks', 'tsdf', 'weight', 'xyz'):
            if not np.array_equal(got[key].cpu().numpy(), want[key]):
                raise SystemExit(f'block {block}: the library and the numpy statement disagree on {key}')
        del got
        part = dict(full) if n == FRAMES else measure(ops, depth_dev[:n], K, poses[:n], block, a.reps)
        part.update(numpy_statement_host_ms=host_ms, numpy_statement_runs=1, numpy_over_device=host_ms / part['ms']['median_ms'])
        out[f'block{block}'] = {'fragment': full, 'statement_frames': part}
        ok &= part['ms']['median_ms'] <= host_ms
    out['not_slower_than_numpy'] = bool(ok)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit('the library is slower on the device than the numpy statement on the host')


if __name__ == '__main__':
    main()
