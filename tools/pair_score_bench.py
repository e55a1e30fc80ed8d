"""Device-event times of `ops.score_pairs` (csrc/pairscore.hip) beside the only way the code before it can compute the
same eleven sums per directed pair: `ops.radius_pairs_batch(K=1)` on the pairs in its batch layout (every pair's source
and target rows copied out of the bank), then a torch gather of the partners and per-pair sums on the device.

Two inputs, both at 5-cm voxels with radius = 2 voxels:

  * `pairs6`:  the 6 pairs of `tools/gt_match_bench.py` (`synth_pair(s, 50000)`, ~27 k / ~21 k rows), a 12-fragment bank,
               every pair scored in both directions under its ground-truth pose: 12 directed pairs;
  * `scene12`: the 12 fragments of `synth_scene(0, 12, 50000)` with all 132 directed pairs under the poses that relate
               them (windows of one room: the farthest two still share a sixth of their width).

Median / min / max of `--reps` calls after 3 warm-up calls.  The composition's time EXCLUDES building its batch layout
(`layout_ms`, reported beside it), and `radius_pairs_batch_K1_alone` is the library call without any of the torch work
behind it -- a floor under every way of writing that part.  The two results are compared before anything is timed (same
n, sums to 1e-9).  Recorded, not asserted: there is no target ratio.

    python tools/pair_score_bench.py [--reps 20] [--out profiles/pair_score_bench.json] [--commit HASH]
"""
import argparse
import json
import os
import sys

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


def batch_layout(xyz, off, ids):
    """The directed pairs in the layout `radius_pairs_batch` takes: (X0, off0, X1, off1), rows copied on the device."""
    dev = xyz.device
    rows0 = torch.cat([torch.arange(int(off[i]), int(off[i + 1]), device=dev) for i, _ in ids])
    rows1 = torch.cat([torch.arange(int(off[j]), int(off[j + 1]), device=dev) for _, j in ids])
    n0 = [int(off[i + 1] - off[i]) for i, _ in ids]
    n1 = [int(off[j + 1] - off[j]) for _, j in ids]
    return xyz[rows0].contiguous(), np.cumsum([0] + n0), xyz[rows1].contiguous(), np.cumsum([0] + n1)


def composition(ops, X0, off0, X1, off1, Ts, Ts_dev, radius):
    """The eleven sums per pair from the K = 1 pair list: float64 [n,11] on the host."""
    dev = X0.device
    pairs, pair_off = ops.radius_pairs_batch(X0, off0, X1, off1, Ts, radius, K=1)
    n = len(off0) - 1
    seg = torch.repeat_interleave(torch.arange(n, device=dev), torch.from_numpy(np.diff(pair_off)).to(dev))
    o0, o1 = torch.from_numpy(off0).to(dev), torch.from_numpy(off1).to(dev)
    x = X0[pairs[:, 0] + o0[seg]].double()
    q = X1[pairs[:, 1] + o1[seg]].double()
    T = Ts_dev[seg]
    p = torch.einsum('nrc,nc->nr', T[:, :3, :3], x) + T[:, :3, 3]
    d2 = ((p - q) ** 2).sum(1, keepdim=True)
    terms = torch.cat((torch.ones_like(d2), d2, q, q[:, :1] * q, q[:, 1:2] * q[:, 1:], q[:, 2:] * q[:, 2:]), 1)
    # a pair's entries are contiguous: one slice sum per pair (a float64 index_add_ over them was many times slower)
    return torch.stack([terms[int(pair_off[k]):int(pair_off[k + 1])].sum(0) for k in range(n)]).cpu().numpy()


def measure(ops, name, xyz, off, ids, Ts, radius, reps):
    ids = np.asarray(ids, np.int32)
    Ts = np.ascontiguousarray(Ts, np.float64)
    Ts_dev = torch.from_numpy(Ts).to(xyz.device)
    new = ops.score_pairs(xyz, off, ids, Ts, radius)
    X0, off0, X1, off1 = batch_layout(xyz, off, ids)
    old = composition(ops, X0, off0, X1, off1, Ts, Ts_dev, radius)
    if not np.array_equal(new[:, 0], old[:, 0]):
        raise SystemExit(f'{name}: the two ways disagree on n: {new[:, 0]} / {old[:, 0]}')
    # (the composition's d^2 comes from an einsum, not the kernel's fixed operation order: 1e-9 relative covers it)
    scale = np.abs(old).max(0) + 1e-300
    if (np.abs(new - old) / scale).max() > 1e-9:
        raise SystemExit(f'{name}: the two ways disagree on the sums')
    res = {'score_pairs': timed(lambda: ops.score_pairs(xyz, off, ids, Ts, radius), reps),
           'radius_pairs_batch_K1_gather_sums': timed(lambda: composition(ops, X0, off0, X1, off1, Ts, Ts_dev, radius), reps),
           'radius_pairs_batch_K1_alone': timed(lambda: ops.radius_pairs_batch(X0, off0, X1, off1, Ts, radius, K=1), reps),
           'layout_ms': timed(lambda: batch_layout(xyz, off, ids), reps)}
    rows = np.diff(off)
    return {'fragments': int(len(off) - 1), 'rows_per_fragment': rows.tolist(), 'directed_pairs': int(len(ids)),
            'target_fragments': int(len(np.unique(ids[:, 1]))), 'source_rows_scored': int(rows[ids[:, 0]].sum()),
            'n_corr_total': int(new[:, 0].sum()), 'pairs_with_fitness_ge_0.3': int((new[:, 0] / rows[ids[:, 0]] >= 0.3).sum()),
            'ms': res,
            'composition_over_score_pairs': res['radius_pairs_batch_K1_gather_sums']['median_ms'] / res['score_pairs']['median_ms'],
            'radius_pairs_alone_over_score_pairs': res['radius_pairs_batch_K1_alone']['median_ms'] / res['score_pairs']['median_ms']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n-raw', type=int, default=50000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    a = ap.parse_args()
    from deepglobalregistration_amd import ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('pair_score_bench measures on the GPU; there is nothing to time without one')
    radius = 2 * VOXEL
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'n_raw': a.n_raw, 'voxel': VOXEL,
           'radius': radius}

    frags, ids, Ts = [], [], []
    for s in range(6):
        xyz0, xyz1, T = synth.synth_pair(s, n_raw=a.n_raw)
        frags += [ops.voxelize(xyz0, VOXEL)[0], ops.voxelize(xyz1, VOXEL)[0]]
        ids += [(2 * s, 2 * s + 1), (2 * s + 1, 2 * s)]
        Ts += [T, np.linalg.inv(T)]
    off = np.cumsum([0] + [len(f) for f in frags])
    out['pairs6'] = measure(ops, 'pairs6', torch.cat(frags), off, ids, np.stack(Ts), radius, a.reps)

    clouds, poses, _ = synth.synth_scene(0, 12, n_raw=a.n_raw)
    frags = [ops.voxelize(c, VOXEL)[0] for c in clouds]
    ids = [(i, j) for i in range(12) for j in range(12) if i != j]
    Ts = np.stack([poses[j] @ np.linalg.inv(poses[i]) for i, j in ids])
    off = np.cumsum([0] + [len(f) for f in frags])
    out['scene12'] = measure(ops, 'scene12', torch.cat(frags), off, ids, Ts, radius, a.reps)

    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
