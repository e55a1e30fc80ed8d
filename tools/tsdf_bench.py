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

The colour leg (`--color`) times, per block size and in one process, the depth-only call and the call with
`color=` on the same frames with `synth_color` images (on the device already), and records the cost of colour over depth
only and the median / maximum |point colour - texture at the point| in levels of 255 (information: colour bleeds at
occlusion edges by design).  The run adds its record to the output file as `fetch_bytes`, after how `ts_integrate` fetches
a pixel's colour: three byte loads.  (The recorded file also holds `fetch_words`, written by this leg when the library
could still be switched to one packed 32-bit word per pixel, the variant that lost and left.)  With `--baseline FILE`, a record this tool wrote for the parent commit in the same session on the same
machine, the depth-only medians are compared with the parent's: not slower by more than the parent's own run-to-run spread
(max - min of its repeats, at least five).

    python tools/tsdf_bench.py --color [--reps 20] [--baseline parent.json] [--out profiles/tsdf_color_bench.json]
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


def color_leg(a, ops, synth, depth, depth_dev, K, poses):
    """the record of the colour leg"""
    from voxel_mean_bench import commit_stamp, timed
    color = synth.synth_color(depth, K, poses, seed=0)
    color_dev = torch.from_numpy(color).cuda()
    fetch = 'bytes'
    rec = {'commit': a.commit or commit_stamp(), 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'fetch': fetch}
    baseline = json.load(open(a.baseline)) if a.baseline else None
    ok = True
    for block in (8, 16):
        def plain():
            return ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE)

        def colored():
            return ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE, color=color_dev)
        r = colored()
        if not torch.equal(r['xyz'], plain()):
            raise SystemExit(f'block {block}: colour changed the points')
        xyz, c = r['xyz'].cpu().numpy(), r['color'].cpu().numpy()
        err = np.abs(255.0 * c - synth.color_texture(xyz, 0).astype(np.float64))
        del r
        e = {'points': len(xyz), 'depth_only_ms': timed(plain, a.reps), 'color_ms': timed(colored, a.reps),
             'texture_error_levels': {'median': float(np.median(err)), 'max': float(err.max())}}
        e['color_over_depth_only'] = e['color_ms']['median_ms'] / e['depth_only_ms']['median_ms']
        if baseline:
            b = baseline[f'block{block}']['fragment']['ms']
            spread = b['max_ms'] - b['min_ms']
            e['parent'] = {'commit': baseline['commit'], 'reps': baseline['reps'], 'ms': b, 'spread_ms': spread}
            e['depth_only_minus_parent_ms'] = e['depth_only_ms']['median_ms'] - b['median_ms']
            e['depth_only_not_slower'] = bool(baseline['reps'] >= 5 and e['depth_only_minus_parent_ms'] <= spread)
            ok &= e['depth_only_not_slower']
        rec[f'block{block}'] = e
    out = {}
    if a.out and os.path.exists(a.out):
        out = json.load(open(a.out))
    out.setdefault('input', {'width': WIDTH, 'height': HEIGHT, 'focal': FOCAL, 'frames': FRAMES, 'sweep_deg': SWEEP,
                             'voxel_length': VOXEL, 'sdf_trunc': TRUNC, 'stride': STRIDE, 'color': 'synth_color(seed=0)'})
    out[f'fetch_{fetch}'] = rec
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit("the depth-only call is slower than the parent's by more than the parent's run-to-run spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ref-frames', type=int, default=FRAMES)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--profile-only', action='store_true')
    ap.add_argument('--color', action='store_true', help='the colour leg instead (see the module docstring)')
    ap.add_argument('--baseline', default=None, help="colour leg: the parent commit's record of this tool, same session")
    a = ap.parse_args()
    from deepglobalregistration_amd import ops, synth
    import tsdf_ref
    from voxel_mean_bench import commit_stamp
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_bench measures on the GPU; there is nothing to time without one')
    depth, K, poses, _ = synth.synth_rgbd(0, FRAMES, WIDTH, HEIGHT, FOCAL, sweep_deg=SWEEP)
    depth_dev = torch.from_numpy(depth).cuda()
    if a.color:
        return color_leg(a, ops, synth, depth, depth_dev, K, poses)
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
