"""Device-event times of `ops.pose_graph_optimize` (csrc/posegraph.hip) beside the float64 numpy solver of
tests/posegraph_ref.py (the same Levenberg-Marquardt with frozen line processes, numpy's LAPACK Cholesky) on the same box.

Three sizes:

  * `n12`:     one 12-node graph, chain + closures at distance 2 and 3 + 10 outliers (40 edges);
  * `n60_all`: one 60-node graph with all 1770 pairs, 10 % of them outliers (a 3DMatch-sized scene, all-pairs);
  * `n60_x8`:  eight such graphs (different seeds) in one call.

Median / min / max of `--reps` calls after 3 warm-up calls; a call includes its host side (argument checks, adjacency,
copies in and out).  The numpy solver is timed with `time.perf_counter` over `--ref-reps` runs; `cpu_count` and
`numpy_threads` say what it had.  Before anything is timed the two are compared (F* to 1e-9 relative).  The one condition:
the 60-node call is not slower than the numpy solver (`n60_all.hip_not_slower`); no ratio is fixed in advance.

`--timing-lib PATH`: a second build of the library with the kernel's stage clocks compiled in
(`make -C deepglobalregistration_amd/csrc OUT=PATH BUILD=build_pgtiming EXTRA=-DDGR_PG_TIMING`); each size is then run once
more in a child process under that library, and the kernel's own report -- time per factorisation attempt and the share of
it spent assembling, factorising, substituting and in the edge passes -- is added as `kernel_stages`.

    python tools/pose_graph_bench.py [--reps 20] [--out profiles/pose_graph_bench.json] [--commit HASH] [--timing-lib PATH]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def all_pairs_graph(seed, n=60, outlier_share=0.1):
    """Every pair (i, j), i < j, of `n` random poses: (i, i+1) certain, the rest uncertain; `outlier_share` of all pairs,
    drawn among the uncertain ones, carry a random X.  Noise and information matrices as in posegraph_ref.make_graph."""
    import posegraph_ref as R
    from deepglobalregistration_amd.core import pose_graph as pg
    rng = np.random.default_rng(seed)
    P = np.stack([R.random_pose(rng) for _ in range(n)])
    edges = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int64)
    unc = edges[:, 1] - edges[:, 0] != 1
    outlier = np.zeros(len(edges), bool)
    outlier[rng.choice(np.nonzero(unc)[0], int(round(outlier_share * len(edges))), replace=False)] = True
    X = pg.rigid_inverse(P[edges[:, 1]]) @ P[edges[:, 0]]
    X = R.retract(rng.normal(scale=np.where(unc, 1e-2, 1e-3)[:, None], size=(len(edges), 6)), X)
    X[outlier] = np.stack([R.random_pose(rng) for _ in range(int(outlier.sum()))])
    info = np.stack([R.random_information(rng) for _ in range(len(edges))])
    P_init, reached = pg.spanning_tree_poses(n, edges[~unc], X[~unc], info[~unc, 3, 3], 0)
    assert reached.all()
    return {'n': n, 'edges': edges, 'X': X, 'info': info, 'uncertain': unc, 'outlier': outlier, 'P_true': P,
            'P_init': P[0] @ P_init, 'mu': pg.default_mu(info, 0.1), 'reference_node': 0}


def sizes():
    import posegraph_ref as R
    return {'n12': [R.make_graph(25, 12, 10)], 'n60_all': [all_pairs_graph(100)],
            'n60_x8': [all_pairs_graph(100 + k) for k in range(8)]}


def hip_call(ops, graphs):
    noff = np.cumsum([0] + [g['n'] for g in graphs])
    eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
    cat = lambda k: np.concatenate([g[k] for g in graphs])
    args = (noff, eoff, cat('edges'), cat('X'), cat('info'), cat('uncertain'), cat('P_init'),
            [(g['mu'], g['reference_node']) for g in graphs])
    return lambda: ops.pose_graph_optimize(*args)


def timed(fn, reps, warmup=3):
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


def timing_child():
    """Under a library built with -DDGR_PG_TIMING: one call per size; the kernel prints its stage clocks."""
    from deepglobalregistration_amd import ops
    for name, graphs in sizes().items():
        print(f'size {name}', flush=True)
        hip_call(ops, graphs)()
        torch.cuda.synchronize()


def kernel_stages(lib):
    env = dict(os.environ, DGR_HIP_LIB=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--timing-child'], env=env, capture_output=True, text=True,
                         timeout=600)
    if out.returncode != 0:
        raise SystemExit('the timing child failed:\n' + out.stdout + out.stderr)
    res, name = {}, None
    for line in out.stdout.splitlines():
        if line.startswith('size '):
            name = line.split()[1]
        m = re.match(r'pg timing: graph (\d+) n (\d+) edges (\d+) steps (\d+) factorisations (\d+) total_us ([\d.]+) assemble_us '
                     r'([\d.]+) cholesky_us ([\d.]+) solve_us ([\d.]+) edges_us ([\d.]+)', line)
        if m and name:
            v = [float(x) for x in m.groups()]
            res.setdefault(name, []).append({
                'graph': int(v[0]), 'nodes': int(v[1]), 'edges': int(v[2]), 'accepted_steps': int(v[3]), 'factorisations': int(v[4]),
                'loop_us': v[5], 'us_per_factorisation_attempt': v[5] / max(v[4], 1), 'share_assemble': v[6] / v[5],
                'share_cholesky': v[7] / v[5], 'share_substitution': v[8] / v[5], 'share_edge_passes_and_update': v[9] / v[5]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ref-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--timing-lib', default=None)
    ap.add_argument('--timing-child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pose_graph_bench measures on the GPU; there is nothing to time without one')
    if a.timing_child:
        return timing_child()
    import posegraph_ref as R
    from deepglobalregistration_amd import ops
    from deepglobalregistration_amd.core import pose_graph as pg
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'ref_reps': a.ref_reps,
           'cpu_count': os.cpu_count(), 'numpy_threads': os.environ.get('OMP_NUM_THREADS'),
           'timer': 'device events around the whole call (3 warm-up calls); numpy solver: perf_counter'}
    for name, graphs in sizes().items():
        call = hip_call(ops, graphs)
        P, line, stats = call()
        noff = np.cumsum([0] + [g['n'] for g in graphs])
        eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
        ref_s, worst, steps_ref, true_pruned = [], 0.0, [], 0
        for k, g in enumerate(graphs):
            ts = []
            for _ in range(a.ref_reps):
                t0 = time.perf_counter()
                ref = R.lm_solve(*R.solve_args(g))
                ts.append(time.perf_counter() - t0)
            ref_s.append(float(np.median(ts)))
            steps_ref.append(ref['iterations'])
            F = pg.robust_objective(P[noff[k]:noff[k + 1]], g['edges'], g['X'], g['info'], g['uncertain'], g['mu'])
            worst = max(worst, (F - ref['objective_final']) / ref['objective_final'])
            l = line[eoff[k]:eoff[k + 1]]
            if not (l[g['outlier']] < 0.25).all():
                raise SystemExit(f'{name}: graph {k}: a planted outlier was kept')
            true_pruned += int((l[~g['outlier']] < 0.25).sum())
        if worst > 1e-9:
            raise SystemExit(f'{name}: F* of the kernel is {worst:.3e} (relative) above the numpy solver\'s')
        hip = timed(call, a.reps)
        numpy_ms = 1e3 * float(np.sum(ref_s))
        out[name] = {'graphs': len(graphs), 'nodes': [g['n'] for g in graphs], 'edges': [len(g['edges']) for g in graphs],
                     'outliers': [int(g['outlier'].sum()) for g in graphs], 'true_edges_below_0.25': true_pruned, 'accepted_steps': stats[:, 2].astype(int).tolist(),
                     'accepted_steps_numpy': steps_ref, 'F_rel_above_numpy_worst': worst, 'hip_ms': hip,
                     'numpy_ms_sum_over_graphs': numpy_ms, 'numpy_over_hip': numpy_ms / hip['median_ms'],
                     'hip_not_slower': bool(hip['median_ms'] <= numpy_ms)}
    if a.timing_lib:
        out['kernel_stages'] = kernel_stages(a.timing_lib)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['n60_all']['hip_not_slower']:
        raise SystemExit('the 60-node call is slower than the numpy solver')


if __name__ == '__main__':
    main()
