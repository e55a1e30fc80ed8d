"""Golden vectors of the ground-truth matching and labelling (csrc/gtmatch.hip).

Run where the reference is importable (DGR_REFERENCE, as for make_golden.py):

    python tests/golden/make_golden_gt_match.py

* Labels: the REFERENCE's own `core.correspondence.find_correct_correspondence`, unchanged (it imports with
  tests/golden/me_stub ahead of the reference on sys.path: its `import open3d` finds the stub), for the default
  `len_batch` seeding, an explicit small `hash_seed` that collides, predicted pairs in the k = 3 layout of
  `trainer.find_pairs` (core/trainer.py:660-679) and a batch of three pairs.
* Radius pairs: Open3D is not available, so the expected lists come from `brute_radius_pairs` below, a float64 brute
  force that RESTATES `util.pointcloud.get_matching_indices` (util/pointcloud.py:83-96; KDTreeFlann.search_radius_vector_3d:
  squared distance strictly below radius^2, ascending by distance) -- recorded as a restatement, not as reference output.
  tests/test_gpu_gt_match.py imports the same function for its larger cases.
"""
import os
import sys

import numpy as np

REF = os.environ.get('DGR_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'gt_match.npz')


def transformed_f64(x0, T):
    """T . x0 in float64 on the f32 points widened exactly, in the operation order the kernel fixes:
    ((T0 x + T1 y) + T2 z) + T3 per row of T, products and sums rounded one by one (numpy's elementwise arithmetic)."""
    x0 = np.asarray(x0, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = x0[:, 0], x0[:, 1], x0[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def sqdist_f64(p, x1):
    """[N0,N1] float64 squared distances (ex^2 + ey^2) + ez^2, e = p - x1 (no fused multiply-add anywhere)."""
    x1 = np.asarray(x1, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        e = p[:, None, :] - x1[None, :, :]
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def pairs_from_sqdist(d2, radius, K=None):
    """The ordered pair list from a squared-distance matrix: rows by i, within a row ascending by (d^2, j), first K.
    A NaN or infinite distance (a non-finite coordinate on either side) is no hit.  Also returns, for the checks the GPU
    test asserts, the smallest relative distance of any d^2 to radius^2 and the smallest relative gap between the K-th
    and the (K+1)-th d^2 of a row that has more than K hits."""
    r2 = float(radius) * float(radius)
    with np.errstate(invalid='ignore'):
        hit = d2 < r2
    out, gap = [], np.inf
    for i in np.nonzero(hit.any(1))[0]:
        js = np.nonzero(hit[i])[0]
        order = np.lexsort((js, d2[i, js]))
        js = js[order]
        if K is not None and len(js) > K:
            a, b = d2[i, js[K - 1]], d2[i, js[K]]
            gap = min(gap, (b - a) / b if b > 0 else 0.0)
            js = js[:K]
        out.append(np.stack((np.full(len(js), i, np.int64), js.astype(np.int64)), 1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    finite = d2[np.isfinite(d2)]
    margin = float(np.abs(finite - r2).min() / r2) if finite.size else np.inf
    return pairs, margin, float(gap)


def brute_radius_pairs(x0, x1, T, radius, K=None):
    """int64 [P,2]: every (i, j) with |T x0[i] - x1[j]|^2 < radius^2 (float64), by i and then by (d^2, j), first K per i."""
    return pairs_from_sqdist(sqdist_f64(transformed_f64(x0, T), x1), radius, K)[0]


def find_pairs_layout(nns):
    """`trainer.find_pairs` (core/trainer.py:669-678) for one batch entry: nns [N0,k] -> [k N0, 2], column j of the
    neighbours stacked below column j - 1."""
    n0, k = nns.shape
    return np.concatenate([np.stack((np.arange(n0), nns[:, j]), 1) for j in range(k)]).astype(np.int64)


def label_inputs():
    rng = np.random.default_rng(7)
    cases = {}

    def entry(n0, n1, n_pos, k):
        pos = np.unique(np.stack((rng.integers(0, n0, n_pos), rng.integers(0, n1, n_pos)), 1), axis=0).astype(np.int64)
        nns = rng.integers(0, n1, (n0, k))
        take = rng.random(n0) < 0.5                 # half of the rows: the first neighbour is a positive partner of the row
        for i in np.nonzero(take)[0]:
            js = pos[pos[:, 0] == i, 1]
            if len(js):
                nns[i, 0] = js[0]
        return pos, find_pairs_layout(nns), (n0, n1)
    cases['default'] = [entry(120, 150, 300, 1)]
    cases['k3'] = [entry(90, 70, 250, 3)]
    cases['batch3'] = [entry(60, 80, 150, 1), entry(40, 30, 60, 3), entry(100, 100, 400, 1)]
    cases['collide'] = [entry(200, 180, 500, 1)]    # hash_seed = 7 << N1: i + 7 j takes 1460 values for 36000 pairs
    return cases


LABEL_SEED = {'default': None, 'k3': None, 'batch3': None, 'collide': 7}


def radius_inputs():
    rng = np.random.default_rng(11)
    x0 = rng.uniform(-1, 1, (150, 3)).astype(np.float32)
    x1 = np.concatenate([x0[:100] + rng.normal(scale=0.05, size=(100, 3)), rng.uniform(-1, 1, (70, 3))]).astype(np.float32)
    ang = 0.7
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    T[:3, 3] = [0.3, -0.2, 0.1]
    x1 = (x1.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return x0, x1[rng.permutation(len(x1))], T, 0.2


def compute(ref=REF):
    for p in (ref, os.path.join(HERE, 'me_stub')):    # the stub first: the reference imports open3d
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    from core.correspondence import find_correct_correspondence
    out = {}
    for name, entries in label_inputs().items():
        pos = [e[0] for e in entries]
        pred = [e[1] for e in entries]
        lens = [list(e[2]) for e in entries]
        seed = LABEL_SEED[name]
        lab = find_correct_correspondence(pos, pred, hash_seed=seed, len_batch=None if seed is not None else lens)
        out[f'label_{name}'] = np.asarray(lab, bool)
        out[f'label_{name}_len_batch'] = np.asarray(lens, np.int64)
        for p, (a, b, _) in enumerate(entries):
            out[f'label_{name}_pos{p}'] = a
            out[f'label_{name}_pred{p}'] = b
    # the colliding seed must really collide: some pair is labelled correct that is no positive pair
    e = label_inputs()['collide'][0]
    exact = np.isin(e[1][:, 0] + e[1][:, 1] * 10 ** 6, e[0][:, 0] + e[0][:, 1] * 10 ** 6)
    assert (out['label_collide'] & ~exact).any()
    x0, x1, T, r = radius_inputs()
    out.update(radius_x0=x0, radius_x1=x1, radius_T=T, radius_r=np.float64(r))
    d2 = sqdist_f64(transformed_f64(x0, T), x1)
    for K in (None, 2):
        pairs, margin, gap = pairs_from_sqdist(d2, r, K)
        assert margin > 1e-9 and gap > 1e-9, (margin, gap)
        out[f'radius_pairs_K{K or 0}_restated'] = pairs
    return out


def main():
    out = compute()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
