"""Scene workload: every overlapping pair of a 12-fragment synthetic scene (BASELINE configs[1] shape: 50 k raw points
per fragment, 5 cm voxels, conv1 k = 7), in batches of 6, registered three ways in one process:

  (a) `register_batch` from the raw clouds           (voxelises and featurises both clouds of every pair),
  (b) `register_voxelized` on pre-voxelised tensors  (featurises both clouds of every pair; bench.py's timed call),
  (c) `extract_fragments` + `register_pairs`         (voxelises and featurises every fragment ONCE; extraction is timed).

Matches and logits are teacher-forced like bench.py's (untrained weights): a share of the 1-NN results replaced by
ground-truth matches, logits from `synth.gt_forced_logits` on the final matches of an untimed run of (b).  After every
shape has run once, the three methods alternate, `--reps` times each; a repetition is a host clock around all batches
of the scene, ending in a stream synchronise.  Writes profiles/scene_bench.json.  Needs the GPU.

    python tools/scene_bench.py [--reps 5] [--fragments 12] [--n-raw 50000] [--out profiles/scene_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--fragments', type=int, default=12)
    ap.add_argument('--n-raw', type=int, default=50000)
    ap.add_argument('--batch-pairs', type=int, default=6)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_bench.json'))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('at least five repetitions')
    import torch
    if not torch.cuda.is_available():
        sys.exit('scene_bench.py needs a GPU')
    from deepglobalregistration_amd import ops, synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    voxel, dev = 0.05, torch.device('cuda')
    ck = synth.synth_checkpoint(seed=0, voxel_size=voxel, feat_conv1_kernel_size=7)
    dgr = DeepGlobalRegistration({'weights': ck, 'clip_weight_thresh': 0.05}, dev)
    clouds, _, scene_pairs = synth.synth_scene(args.seed, args.fragments, n_raw=args.n_raw)
    pairs = [(i, j) for i, j, _ in scene_pairs]
    B = args.batch_pairs
    groups = [list(range(k, min(k + B, len(pairs)))) for k in range(0, len(pairs), B)]
    vox = [dgr.preprocess(c)[:2] for c in clouds]
    host = [x.cpu().numpy() for x, _ in vox]

    # per pair: planted matches (pair-local, -1 = keep the search's) and, from an untimed run of (b), forced logits
    ovr = [synth.gt_correspondences(host[i], host[j], T, voxel, seed=k) for k, (i, j, T) in enumerate(scene_pairs)]
    batches = []
    for g in groups:
        c0, x0, c1, x1, off0, off1 = [], [], [], [], [0], [0]
        for q, k in enumerate(g):
            for f, cs, xs, off in ((pairs[k][0], c0, x0, off0), (pairs[k][1], c1, x1, off1)):
                x, c = vox[f]
                c = c.clone()
                c[:, 0] = q
                cs.append(c); xs.append(x); off.append(off[-1] + len(x))
        bt = dict(C0=torch.cat(c0), X0=torch.cat(x0), off0=off0, C1=torch.cat(c1), X1=torch.cat(x1), off1=off1,
                  ovr=torch.from_numpy(np.concatenate([np.where(ovr[k] >= 0, ovr[k] + off1[q], -1)
                                                       for q, k in enumerate(g)])).to(dev))
        dgr.register_voxelized(bt['C0'], bt['X0'], off0, bt['C1'], bt['X1'], off1, override_idx1=bt['ovr'])
        idx1 = ops.batch_output(dev, 'idx1').cpu().numpy()
        X1h = bt['X1'].cpu().numpy()
        bt['fl'] = [synth.gt_forced_logits(host[pairs[k][0]], X1h[idx1[off0[q]:off0[q + 1]]], scene_pairs[k][2], voxel)
                    for q, k in enumerate(g)]
        bt['forced'] = torch.from_numpy(np.concatenate(bt['fl'])).to(dev)
        batches.append(bt)
    forced = [f for bt in batches for f in bt['fl']]

    def run_a():
        out = []
        for g, bt in zip(groups, batches):
            # (register_batch has no match hook: its matches are the search's; the logits stay forced)
            out.append(dgr.register_batch([(clouds[pairs[k][0]], clouds[pairs[k][1]]) for k in g],
                                          forced_logits=bt['forced'])[1])
        return np.concatenate(out)

    def run_b():
        return np.concatenate([dgr.register_voxelized(bt['C0'], bt['X0'], bt['off0'], bt['C1'], bt['X1'], bt['off1'],
                                                      forced_logits=bt['forced'], override_idx1=bt['ovr'])[1]
                               for bt in batches])

    def run_c():
        bank = dgr.extract_fragments(clouds)
        return dgr.register_pairs(bank, pairs, batch_pairs=B, forced_logits=forced, override_idx1=ovr)[1]
    methods = {'a_register_batch_raw': run_a, 'b_register_voxelized': run_b, 'c_extract_register_pairs': run_c}
    status = {}
    for name, fn in methods.items():      # every shape once, untimed
        status[name] = fn().tolist()
        torch.cuda.synchronize()
    times = {name: [] for name in methods}
    for _ in range(args.reps):
        for name, fn in methods.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            times[name].append(time.perf_counter() - t0)

    def summary(ts):
        ts = np.asarray(ts)
        return {'median_s': float(np.median(ts)), 'min_s': float(ts.min()), 'max_s': float(ts.max()),
                'spread_rel': float((ts.max() - ts.min()) / np.median(ts)),
                'pairs_per_s': float(len(pairs) / np.median(ts)), 'times_s': [float(t) for t in ts]}
    res = {name: summary(ts) for name, ts in times.items()}
    try:
        commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                                check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = open(os.path.join(ROOT, 'tools', 'COMMIT')).read().strip() if \
            os.path.exists(os.path.join(ROOT, 'tools', 'COMMIT')) else 'unknown'
    b, c = res['b_register_voxelized'], res['c_extract_register_pairs']
    doc = {'what': 'tools/scene_bench.py: all overlapping pairs of one synthetic scene, three ways (see its docstring)',
           'commit_parent': commit, 'device': torch.cuda.get_device_name(0),
           'fragments': args.fragments, 'n_raw': args.n_raw, 'voxel_size': voxel, 'batch_pairs': B,
           'pairs': len(pairs), 'voxels_per_fragment': [len(h) for h in host],
           'fragment_multiplicity': {'mean': float(2 * len(pairs) / args.fragments),
                                     'per_fragment': np.bincount(np.asarray(pairs).reshape(-1),
                                                                 minlength=args.fragments).tolist()},
           'reps': args.reps, 'methods': res,
           'ratio_c_over_b_time': float(c['median_s'] / b['median_s']),
           'c_not_slower_than_b_beyond_spread_of_b': bool(c['median_s'] <= b['max_s']),
           'status_counts': {name: np.bincount(np.asarray(s) & 0xff, minlength=4).tolist() for name, s in status.items()}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in doc.items() if k != 'methods'}))
    for name, r in res.items():
        print(f'{name:28s} median {r["median_s"] * 1e3:8.2f} ms  [{r["min_s"] * 1e3:.2f}, {r["max_s"] * 1e3:.2f}]  '
              f'{r["pairs_per_s"]:7.1f} pairs/s')
    return 0 if doc['c_not_slower_than_b_beyond_spread_of_b'] else 1


if __name__ == '__main__':
    sys.exit(main())
