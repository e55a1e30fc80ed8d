"""Device-event times of the batched k-NN search (`ops.knn_batch`, dgr_knn_l2_batch; k = 1: `ops.knn1_batch`) at the
BASELINE configs[1] shapes: 6 pairs of ~27k x 27k FCGF descriptors (C = 32) of `synth_pair` clouds under
`synth_checkpoint` weights, k in {1, 2, 4, 8, 16, 32}, the prefiltered search against DGR_KNN_BRUTE=1 (read once per
process: each mode runs in a child process of its own).

    python tools/knn_topk_bench.py [--pairs 6] [--reps 10] [--out profiles/knn_topk_bench.json] [--commit HASH]
    rocprofv3 --kernel-trace --stats -- python tools/knn_topk_bench.py --in-process --reps 3   # per-kernel times
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
KS = (1, 2, 4, 8, 16, 32)


def features(pairs):
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    ck = synth.synth_checkpoint(seed=0, voxel_size=0.05, feat_conv1_kernel_size=7)
    dgr = DeepGlobalRegistration({'weights': ck}, torch.device('cuda:0'))
    F0, F1, n0, n1 = [], [], [], []
    for s in range(pairs):
        xyz0, xyz1, _ = synth.synth_pair(s, n_raw=50000)
        for xyz, F, n in ((xyz0, F0, n0), (xyz1, F1, n1)):
            _, c, f = dgr.preprocess(xyz)
            F.append(dgr.fcgf_feature_extraction(f, c).cpu().numpy())
            n.append(len(F[-1]))
    return np.concatenate(F0), np.concatenate(F1), np.array(n0), np.array(n1)


def time_search(F0, F1, n0, n1, reps):
    """Device-event times of the batched search for every k of KS (the mode this process runs in)."""
    from deepglobalregistration_amd import ops
    F0, F1 = torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda()
    off0 = np.concatenate([[0], np.cumsum(n0)])
    off1 = np.concatenate([[0], np.cumsum(n1)])
    res = {}
    for k in KS:
        def run():
            if k == 1:
                return ops.knn1_batch(F0, F1, off0, off1, return_distance=True)
            return ops.knn_batch(F0, F1, off0, off1, k, return_distance=True)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res[str(k)] = {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}
    return res


def child(path, reps):
    d = np.load(path)
    print(json.dumps(time_search(d['F0'], d['F1'], d['n0'], d['n1'], reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--child', default=None)
    ap.add_argument('--in-process', action='store_true',
                    help='one process, the mode of the environment (for a profiler that follows no child process)')
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return
    F0, F1, n0, n1 = features(a.pairs)
    if a.in_process:
        mode = 'brute' if os.environ.get('DGR_KNN_BRUTE') else 'prefilter'
        print(json.dumps({mode: time_search(F0, F1, n0, n1, a.reps)}, indent=1))
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'feats.npz')
        np.savez(path, F0=F0, F1=F1, n0=n0, n1=n1)
        modes = {}
        for mode in ('prefilter', 'brute'):
            env = dict(os.environ)
            env.pop('DGR_KNN_BRUTE', None)
            if mode == 'brute':
                env['DGR_KNN_BRUTE'] = '1'
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, '--reps', str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f'{mode} child failed with status {r.returncode}')
            modes[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'pairs': a.pairs, 'reps': a.reps,
           'n0': n0.tolist(), 'n1': n1.tolist(), 'C': int(F0.shape[1]), 'ms': modes,
           'prefilter_k_over_k1': {k: modes['prefilter'][k]['median_ms'] / modes['prefilter']['1']['median_ms']
                                   for k in modes['prefilter']}}
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
