"""Device-event times of the ground-truth matching group (csrc/gtmatch.hip) at the BASELINE configs[1] size: 6 pairs
of `synth_pair` clouds (50 k raw points, 5-cm voxels, ~27 k rows per side), radius = 2 voxels under the ground-truth pose:

  * `ops.radius_pairs_batch` (count call + fill call, all pairs in the same launches),
  * `ops.pairs_isin` of one predicted match per row against those pairs, `ops.validation_counts`,

beside `scipy.spatial.cKDTree.query_ball_point` on the same inputs (tree build + query per pair, all host cores the run
may use: `--workers`), the host loop these calls replace.  Recorded, not asserted: there is no target.

    python tools/gt_match_bench.py [--pairs 6] [--reps 20] [--workers 16] [--out profiles/gt_match_bench.json] [--commit HASH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
VOXEL = 0.05


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--n-raw', type=int, default=50000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    from deepglobalregistration_amd import ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('gt_match_bench measures on the GPU; there is nothing to time without one')
    radius = 2 * VOXEL
    x0s, x1s, Ts = [], [], []
    for s in range(a.pairs):
        xyz0, xyz1, T = synth.synth_pair(s, n_raw=a.n_raw)
        x0s.append(ops.voxelize(xyz0, VOXEL)[0])
        x1s.append(ops.voxelize(xyz1, VOXEL)[0])
        Ts.append(T)
    off0 = np.cumsum([0] + [len(x) for x in x0s])
    off1 = np.cumsum([0] + [len(x) for x in x1s])
    X0, X1, Ts = torch.cat(x0s), torch.cat(x1s), np.stack(Ts)

    pairs, pair_off = ops.radius_pairs_batch(X0, off0, X1, off1, Ts, radius)
    res = {'radius_pairs_batch': timed(lambda: ops.radius_pairs_batch(X0, off0, X1, off1, Ts, radius), a.reps),
           'radius_pairs_batch_K1': timed(lambda: ops.radius_pairs_batch(X0, off0, X1, off1, Ts, radius, 1), a.reps)}
    # one predicted match per row (half of them a ground-truth partner), as validate_collated labels them
    rng = np.random.default_rng(0)
    pred = []
    for p in range(a.pairs):
        n0, n1 = int(off0[p + 1] - off0[p]), int(off1[p + 1] - off1[p])
        j = rng.integers(0, n1, n0)
        own = pairs[pair_off[p]:pair_off[p + 1]].cpu().numpy()
        first = np.unique(own[:, 0], return_index=True)
        take = rng.random(len(first[0])) < 0.5
        j[first[0][take]] = own[first[1][take], 1]
        pred.append(np.stack((np.arange(n0), j), 1))
    pred = torch.from_numpy(np.concatenate(pred)).cuda()
    seeds = [max(int(off0[p + 1] - off0[p]), int(off1[p + 1] - off1[p])) for p in range(a.pairs)]
    label = ops.pairs_isin(pairs, pair_off, pred, off0, seeds)
    weights = torch.from_numpy(rng.random(len(label)).astype(np.float32)).cuda()
    res['pairs_isin'] = timed(lambda: ops.pairs_isin(pairs, pair_off, pred, off0, seeds), a.reps)
    res['validation_counts'] = timed(lambda: ops.validation_counts(label, weights, off0), a.reps)

    # the host loop: KD-tree radius queries per pair (the reference: Open3D's KD-tree from a Python loop per point)
    h0 = [x.cpu().numpy().astype(np.float64) @ T[:3, :3].T + T[:3, 3] for x, T in zip(x0s, Ts)]
    h1 = [x.cpu().numpy().astype(np.float64) for x in x1s]
    host_ms, host_pairs = [], 0
    for rep in range(1 + min(a.reps, 5)):
        t = time.perf_counter()
        host_pairs = 0
        for p0, p1 in zip(h0, h1):
            host_pairs += sum(len(v) for v in cKDTree(p1).query_ball_point(p0, radius, workers=a.workers))
        if rep:
            host_ms.append(1e3 * (time.perf_counter() - t))
    res['scipy_cKDTree_query_ball_point'] = {'median_ms': float(np.median(host_ms)), 'min_ms': float(np.min(host_ms)),
                                             'max_ms': float(np.max(host_ms)), 'workers': a.workers}
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'reps': a.reps, 'n_raw': a.n_raw,
           'voxel': VOXEL, 'radius': radius, 'n0': np.diff(off0).tolist(), 'n1': np.diff(off1).tolist(),
           'gt_pairs': int(len(pairs)), 'host_pairs_closed_ball': int(host_pairs), 'label_share': float(label.float().mean()),
           'ms': res,
           'host_over_device_radius_pairs': res['scipy_cKDTree_query_ball_point']['median_ms'] / res['radius_pairs_batch']['median_ms']}
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
