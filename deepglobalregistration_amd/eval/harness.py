"""Evaluation loop in the spirit of scripts/test_3dmatch.py:87-156: every pair of a trajectory dataset is
registered by each method, and success / RTE / RRE / time are accumulated per pair and per scene."""
import os
import time

import numpy as np

from .formats import load_cloud, read_trajectory, write_ply, write_trajectory
from .metrics import rte_rre


class ThreeDMatchTrajectory:
    """The test split layout read by `ThreeDMatchTrajectoryDataset` (dataloader/threedmatch_loader.py:144-196):
    `<root>/<scene>/cloud_bin_<i>.ply` fragments and `<root>/<scene>-evaluation/gt.log` with one record per
    overlapping pair (i, j) whose pose maps fragment j into fragment i.  Items are (scene, xyz_i, xyz_j, T_gt)."""

    def __init__(self, root, scenes=None):
        self.root = root
        if scenes is None:
            scenes = sorted(d[:-len('-evaluation')] for d in os.listdir(root) if d.endswith('-evaluation'))
        self.scenes = list(scenes)
        self.files = []
        for s in self.scenes:
            traj = os.path.join(root, s + '-evaluation', 'gt.log')
            if not os.path.exists(traj):
                raise FileNotFoundError(traj)
            for meta, pose in read_trajectory(traj):
                self.files.append((s, meta[0], meta[1], pose))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, k):
        s, i, j, T = self.files[k]
        return (s, load_cloud(os.path.join(self.root, s, f'cloud_bin_{i}.ply')),
                load_cloud(os.path.join(self.root, s, f'cloud_bin_{j}.ply')), T)

    def fragment(self, scene, i):
        """The cloud of fragment i of `scene`."""
        return load_cloud(os.path.join(self.root, scene, f'cloud_bin_{i}.ply'))

    def records(self, scene):
        """The (i, j, pose) triples of `scene` in file order (the order its items have in the dataset)."""
        return [(i, j, T) for s, i, j, T in self.files if s == scene]


def analyze_stats(stats, mask, method_names, out=print):
    """Mean [success, RTE, RRE, time, scene id] over the evaluated pairs, and over the successful ones."""
    mask = np.asarray(mask).reshape(-1) > 0
    summary = {}
    for m, name in enumerate(method_names):
        s = stats[m][mask]
        ok = s[s[:, 0] > 0]
        summary[name] = {'pairs': int(len(s)), 'recall': float(s[:, 0].mean()) if len(s) else 0.0,
                         'mean': s.mean(0) if len(s) else np.zeros(stats.shape[2]),
                         'mean_successful': ok.mean(0) if len(ok) else np.zeros(stats.shape[2])}
        out(f'{name}: recall {summary[name]["recall"]:.4f} over {len(s)} pairs; successful pairs: '
            f'RTE {summary[name]["mean_successful"][1]:.4f} m, RRE {summary[name]["mean_successful"][2]:.3f} deg, '
            f'{summary[name]["mean_successful"][3]:.4f} s')
    return summary


def evaluate(methods, method_names, dataset, success_rte_thresh=0.3, success_rre_thresh=15.0, out=print,
             summary_every=0):
    """`methods` expose `.register(xyz0, xyz1) -> T [4,4]`.  The ground truth of a gt.log record maps the
    second fragment into the first, and `register` estimates first -> second, hence `T_gt = inv(pose)`
    (scripts/test_3dmatch.py:106).  Returns (stats [methods, pairs, 5], per-scene means, summary)."""
    n = len(dataset)
    scenes = list(getattr(dataset, 'scenes', []))
    stats = np.zeros((len(methods), n, 5))
    mask = np.zeros((n, 1), int)
    for k in range(n):
        sname, xyz0, xyz1, pose = dataset[k]
        if sname not in scenes:
            scenes.append(sname)
        T_gt = np.linalg.inv(pose)
        for m, method in enumerate(methods):
            t0 = time.time()
            T = method.register(xyz0, xyz1)
            stats[m, k, :3] = rte_rre(T, T_gt, success_rte_thresh, success_rre_thresh)
            stats[m, k, 3] = time.time() - t0
            stats[m, k, 4] = scenes.index(sname)
        mask[k] = 1
        if summary_every and k % summary_every == summary_every - 1:
            analyze_stats(stats, mask, method_names, out)
    summary = analyze_stats(stats, mask, method_names, out)
    scene_means = np.zeros((len(methods), len(scenes), 3))
    for m in range(len(methods)):
        for sid in range(len(scenes)):
            sel = stats[m, :, 4] == sid
            if sel.any():
                scene_means[m, sid] = stats[m, sel, :3].mean(0)
    return stats, scene_means, summary


def evaluate_batched(method, dataset, success_rte_thresh=0.3, success_rre_thresh=15.0, batch_pairs=6, out=print):
    """`evaluate` for one method that can register a scene's pair list from features computed once per fragment:
    per scene, every fragment that occurs in a record is loaded once, `method.extract_fragments(clouds)` featurises
    them, and `method.register_pairs(bank, pairs, batch_pairs, safeguard=True, icp=method.use_icp)` registers all
    records (the flags give the branch structure of `register()`: gate, safeguard RANSAC, final ICP).  Metrics as in
    `evaluate` (T_gt = inv(pose)); returns the same (stats [1, pairs, 5], per-scene means [1, scenes, 3], summary).
    The time column is NOT the per-call time `evaluate` records: it is the scene's wall time, from the first load to a
    device synchronisation behind the last batch, divided by the scene's records."""
    scenes = list(dataset.scenes)
    stats = np.zeros((1, len(dataset), 5))
    k = 0
    for sid, sname in enumerate(scenes):      # (dataset.files lists the scenes in this order)
        recs = dataset.records(sname)
        if not recs:
            continue
        t0 = time.time()
        frags = sorted({f for i, j, _ in recs for f in (i, j)})
        slot = {f: n for n, f in enumerate(frags)}
        bank = method.extract_fragments([dataset.fragment(sname, f) for f in frags])
        T, _, _ = method.register_pairs(bank, [(slot[i], slot[j]) for i, j, _ in recs], batch_pairs,
                                        safeguard=True, icp=method.use_icp)
        dev = getattr(method, 'device', None)
        if dev is not None and getattr(dev, 'type', None) == 'cuda':
            import torch
            torch.cuda.synchronize(dev)
        dt = (time.time() - t0) / len(recs)
        for r, (_, _, pose) in enumerate(recs):
            stats[0, k, :3] = rte_rre(T[r], np.linalg.inv(pose), success_rte_thresh, success_rre_thresh)
            stats[0, k, 3] = dt
            stats[0, k, 4] = sid
            k += 1
    assert k == len(dataset)
    summary = analyze_stats(stats, np.ones((len(dataset), 1), int), ['DGR'], out)
    scene_means = np.zeros((1, len(scenes), 3))
    for sid in range(len(scenes)):
        sel = stats[0, :, 4] == sid
        if sel.any():
            scene_means[0, sid] = stats[0, sel, :3].mean(0)
    return stats, scene_means, summary


def optimize_scenes(method, dataset, out_dir, success_rte_thresh=0.3, success_rre_thresh=15.0, batch_pairs=6, out=print,
                    fused_dir=None, fused_voxel=None):
    """The scene mode: per scene, the fragments of its records are featurised once, the records registered
    (`register_pairs` as in `evaluate_batched`), scored and handed to `method.optimize_scene` -- robust pose-graph
    optimisation over the scored pairs (csrc/posegraph.hip).  Writes `<out_dir>/<scene>.log`: one record
    "k k n_fragments" + the 4x4 pose of fragment k in the frame of the scene's first fragment (`write_trajectory`; the
    trajectory format of the Redwood reconstruction pipeline), for the fragments the kept edges connect to it.
    With `fused_dir`, also `<fused_dir>/<scene>.ply`: the scene itself, the reachable fragments of the bank under their
    optimised poses averaged per voxel of `fused_voxel` (default: the method's voxel size) by `method.fuse_scene`.
    Returns (stats [2, pairs, 5], rows): stats[0] judges the pairwise poses as `evaluate_batched` does, stats[1] the
    poses the optimised trajectory implies for the same records, inv(P_j) P_i (a record with an unreachable fragment
    counts as a failure); the time column of stats[1] is the optimisation's wall time per record.  rows: per scene
    (name, fragments, reachable fragments, pairs, kept pairs, objective_initial, objective_final, iterations)."""
    os.makedirs(out_dir, exist_ok=True)
    scenes = list(dataset.scenes)
    stats = np.zeros((2, len(dataset), 5))
    rows = []
    k = 0
    for sid, sname in enumerate(scenes):
        recs = dataset.records(sname)
        if not recs:
            continue
        t0 = time.time()
        frags = sorted({f for i, j, _ in recs for f in (i, j)})
        slot = {f: n for n, f in enumerate(frags)}
        bank = method.extract_fragments([dataset.fragment(sname, f) for f in frags])
        pairs = [(slot[i], slot[j]) for i, j, _ in recs]
        T, _, _ = method.register_pairs(bank, pairs, batch_pairs, safeguard=True, icp=method.use_icp)
        t1 = time.time()
        res = method.optimize_scene(bank, pairs, T)
        t2 = time.time()
        P, reach = res['poses'], res['reachable']
        write_trajectory(os.path.join(out_dir, f'{sname}.log'),
                         [((f, f, len(frags)), P[slot[f]]) for f in frags if reach[slot[f]]])
        if fused_dir is not None:
            os.makedirs(fused_dir, exist_ok=True)
            fused = method.fuse_scene(bank, P, voxel_size=fused_voxel, fragments=reach)
            write_ply(os.path.join(fused_dir, f'{sname}.ply'), fused['xyz'].cpu().numpy())
        for r, (i, j, pose) in enumerate(recs):
            T_gt = np.linalg.inv(pose)
            stats[0, k, :3] = rte_rre(T[r], T_gt, success_rte_thresh, success_rre_thresh)
            both = reach[slot[i]] and reach[slot[j]]
            stats[1, k, :3] = rte_rre(np.linalg.inv(P[slot[j]]) @ P[slot[i]] if both else None, T_gt, success_rte_thresh,
                                      success_rre_thresh)
            stats[:, k, 3] = ((t1 - t0) / len(recs), (t2 - t1) / len(recs))
            stats[:, k, 4] = sid
            k += 1
        rows.append((sname, len(frags), int(reach.sum()), len(recs), int(res['kept'].sum()), res['objective_initial'],
                     res['objective_final'], res['iterations']))
        out(f'{sname}: {len(frags)} fragments ({int(reach.sum())} reachable), {len(recs)} pairs ({int(res["kept"].sum())} kept), '
            f'F* {res["objective_initial"]:.6g} -> {res["objective_final"]:.6g} in {res["iterations"]} steps')
    assert k == len(dataset)
    analyze_stats(stats, np.ones((len(dataset), 1), int), ['pairwise', 'pose graph'], out)
    return stats, rows
