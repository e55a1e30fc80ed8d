"""Device-event times of `ops.voxel_mean` (csrc/voxelmean.hip) beside the numpy statement of the same arithmetic on the
host (tests/voxel_mean_ref.py), at 5-cm voxels:

  * `cloud`: one raw `synth_pair(0)` cloud of 50 k points (float64), no pose -- the down-sample of one cloud;
  * `scene`: the bank of `synth_scene(0, 30)` at 50 k raw points per fragment, voxelised at 5 cm (float32), all 30
             fragments fused under their ground-truth poses -- the fused scene.

Median / min / max of `--reps` calls after 3 warm-up calls.  The numpy statement is timed ONCE per input on the host's
wall clock (`numpy_statement_host_ms`: a single, cold run -- the one that also checks the result), so that figure is an
order of magnitude, not a median.  The two results are compared for exact equality before anything is timed.  Beside
the times: the compulsory bytes of a call (rows x 12 in, V x (8 + 12 + 4 + 24) out) and those bytes per second as a share
of the 8 TB/s HBM peak.

`atomics`: what the integer atomics of the accumulate pass cost.  The same 2^21 float32 rows (4 atomics per row: one
int32, three uint64; 28 bytes added per row) laid out three ways -- every row its own voxel, ~50 rows per voxel at random
(a fused scene), ALL rows in one voxel -- through the same call; the passes in front of the accumulation do the same
work per row in all three, so the differences are the atomics' (and the hash's: one voxel is also one slot).

Recorded, not asserted, except the one condition the feature was accepted under: the fused scene is not slower on the
device than the numpy statement on the same box.

The JSON is stamped with the commit: `--commit`, else the file tools/COMMIT (written beside a copy of the tree that has no
history), else `git rev-parse --short HEAD` with "+dirty" when the tree differs from it.

    python tools/voxel_mean_bench.py [--reps 20] [--out profiles/voxel_mean_bench.json] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
VOXEL = 0.05
HBM_PEAK = 8e12   # bytes / s


def timed(fn, reps, warmup=3):
    """Median / min / max device-event time (ms) of fn() after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}


def commit_stamp():
    try:
        with open(os.path.join(ROOT, 'tools', 'COMMIT')) as f:
            return f.read().replace('\n', '')
    except OSError:
        pass
    try:
        head = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True, check=True)
        dirty = subprocess.run(['git', '-C', ROOT, 'diff', '--quiet']).returncode != 0
        return head.stdout.strip() + ('+dirty' if dirty else '')
    except (OSError, subprocess.CalledProcessError):
        return 'unknown'


def atomics_cost(ops, reps, rows=1 << 21):
    """Device-event time of the whole call on `rows` float32 rows at three contention levels (see the module docstring)."""
    rng = np.random.default_rng(0)
    side = int(np.ceil(rows ** (1 / 3)))
    i = rng.permutation(side ** 3)[:rows]
    cells = np.stack((i % side, i // side % side, i // side // side), 1)
    frac = rng.uniform(0.05, 0.95, (rows, 3))
    v50 = int(round((rows / 50) ** (1 / 3)))
    layouts = {'distinct_voxels': (cells + frac) * VOXEL,
               'about_50_per_voxel': (rng.integers(0, v50, (rows, 3)) + frac) * VOXEL,
               'one_voxel': (1 + frac) * VOXEL}
    out = {'rows': rows, 'atomics_per_row': 4, 'bytes_added_per_row': 28}
    for name, x in layouts.items():
        xd = torch.from_numpy(x.astype(np.float32)).cuda()
        r = ops.voxel_mean(xd, VOXEL)
        assert int(r['count'].sum()) == rows and r['dropped'] == 0
        ms = timed(lambda: ops.voxel_mean(xd, VOXEL), reps)
        out[name] = {'voxels': len(r['count']), 'max_per_voxel': int(r['count'].max()), 'ms': ms}
        del r
    base = out['distinct_voxels']['ms']['median_ms']
    for name in ('about_50_per_voxel', 'one_voxel'):
        out[name]['ms_over_distinct'] = out[name]['ms']['median_ms'] - base
    out['one_voxel']['atomics_per_us_on_one_address'] = rows / (out['one_voxel']['ms']['median_ms'] * 1e3)
    return out


def measure(ops, ref, name, x, off, T, reps):
    xd = torch.from_numpy(x).cuda()
    t0 = time.perf_counter()
    want = ref(x, VOXEL, off, None, T)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = ops.voxel_mean(xd, VOXEL, off, None, T, return_sums=True)
    for key, k2 in (('first', 'first'), ('coords', 'coords'), ('count', 'count'), ('sums', 'sums'), ('xyz', 'mean')):
        if not np.array_equal(got[key].cpu().numpy(), want[k2]):
            raise SystemExit(f'{name}: the library and the numpy statement disagree on {key}')
    del got
    ms = timed(lambda: ops.voxel_mean(xd, VOXEL, off, None, T), reps)
    rows, V = len(x), len(want['first'])
    nbytes = rows * 12 + V * (8 + 12 + 4 + 24)
    return {'rows': rows, 'dtype': str(x.dtype), 'fragments': 1 if off is None else len(off) - 1, 'voxels': V,
            'points_per_voxel_mean': rows / V, 'points_per_voxel_max': int(want['count'].max()), 'dropped': want['dropped'],
            'ms': ms, 'numpy_statement_host_ms': host_ms, 'numpy_statement_runs': 1, 'numpy_over_device': host_ms / ms['median_ms'],
            'compulsory_bytes': nbytes, 'compulsory_bytes_per_s': nbytes / (ms['median_ms'] * 1e-3),
            'share_of_hbm_peak': nbytes / (ms['median_ms'] * 1e-3) / HBM_PEAK,
            'us_per_1e6_rows': ms['median_ms'] * 1e3 / (rows / 1e6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n-raw', type=int, default=50000)
    ap.add_argument('--fragments', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    from deepglobalregistration_amd import ops, synth
    from voxel_mean_ref import voxel_mean_ref
    if not torch.cuda.is_available():
        raise SystemExit('voxel_mean_bench measures on the GPU; there is nothing to time without one')
    out = {'commit': a.commit or commit_stamp(), 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'n_raw': a.n_raw, 'voxel': VOXEL,
           'hbm_peak_bytes_per_s': HBM_PEAK}
    cloud = np.ascontiguousarray(synth.synth_pair(0, n_raw=a.n_raw)[0])
    out['cloud'] = measure(ops, voxel_mean_ref, 'cloud', cloud, None, None, a.reps)
    clouds, poses, _ = synth.synth_scene(0, a.fragments, n_raw=a.n_raw)
    frags = [ops.voxelize(c, VOXEL)[0].cpu().numpy() for c in clouds]
    off = np.cumsum([0] + [len(f) for f in frags])
    out['scene'] = measure(ops, voxel_mean_ref, 'scene', np.concatenate(frags), off, np.linalg.inv(poses), a.reps)
    out['atomics'] = atomics_cost(ops, a.reps)
    out['scene_not_slower_than_numpy'] = bool(out['scene']['ms']['median_ms'] <= out['scene']['numpy_statement_host_ms'])
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['scene_not_slower_than_numpy']:
        raise SystemExit('the fused scene is slower on the device than the numpy statement on the host')


if __name__ == '__main__':
    main()
