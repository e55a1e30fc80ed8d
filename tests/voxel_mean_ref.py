"""The numpy statement of `dgr_voxel_mean` (include/dgr_hip.h): the averaging voxel down-sample of selected fragments under
their poses on one lattice.  Not a test: the helper the voxel-mean tests compare the library against, for EXACT equality --
every floating-point operation below is one correctly rounded float64 operation in the order the header fixes (numpy's
elementwise arithmetic never fuses a multiply and an add), and the sums are int64."""
import numpy as np

FRAC_BITS = 40   # DGR_VM_FRAC_BITS


def transformed_f64(x, T):
    """T . x in float64 on the rows widened exactly: ((T0 x + T1 y) + T2 z) + T3 per row of T, products and sums rounded
    one by one (tests/golden/make_golden_gt_match.py::transformed_f64, for f32 or f64 rows)."""
    x = np.asarray(x).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([((T[r, 0] * a + T[r, 1] * b) + T[r, 2] * c) + T[r, 3] for r in range(3)], 1)


def voxel_mean_ref(xyz, voxel_size, off=None, frag_ids=None, T=None, origin=None):
    """dict(first int64 [V], coords int32 [V,3], count int32 [V], sums int64 [V,3], mean float64 [V,3], dropped int) of
    xyz [N,3] (float32 or float64: widened exactly), fragment f in rows off[f]:off[f+1] (default: one fragment), the
    distinct fragments `frag_ids` (default: all) under the poses T[k] (default: none) on the lattice (origin, voxel_size).
    Voxels in ascending order of their first row, a row's number being its row in xyz."""
    xyz = np.asarray(xyz)
    assert xyz.dtype in (np.float32, np.float64) and xyz.ndim == 2 and xyz.shape[1] == 3
    off = np.array([0, len(xyz)], np.int64) if off is None else np.asarray(off, np.int64)
    ids = np.arange(len(off) - 1) if frag_ids is None else np.asarray(frag_ids, np.int64)
    assert len(set(ids.tolist())) == len(ids)
    origin = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    voxel = np.float64(voxel_size)
    rows, pts = [], []
    for k in np.argsort(ids, kind='stable'):            # ascending fragment = ascending row of xyz
        a, b = int(off[ids[k]]), int(off[ids[k] + 1])
        rows.append(np.arange(a, b, dtype=np.int64))
        pts.append(xyz[a:b].astype(np.float64) if T is None else transformed_f64(xyz[a:b], np.asarray(T, np.float64)[k]))
    rows, p = np.concatenate(rows), np.concatenate(pts)
    with np.errstate(invalid='ignore', over='ignore'):
        u = (p - origin) / voxel
        keep = (np.isfinite(u) & (u >= -2.0 ** 31) & (u < 2.0 ** 31)).all(1)
    rows, u = rows[keep], u[keep]
    c = np.floor(u)
    k = np.floor((u - c) * 2.0 ** FRAC_BITS).astype(np.int64)
    c = c.astype(np.int64)
    if len(c):
        _, first_idx, inv = np.unique(c, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        order = np.argsort(first_idx, kind='stable')   # voxels by their first row (rows ascend already)
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        v = rank[inv]
        first_idx = first_idx[order]
    else:
        v, first_idx = np.zeros(0, np.int64), np.zeros(0, np.int64)
    V = len(first_idx)
    count = np.zeros(V, np.int64)
    sums = np.zeros((V, 3), np.int64)
    np.add.at(count, v, 1)
    np.add.at(sums, v, k)
    coords = c[first_idx].reshape(V, 3)
    mean = origin + (coords.astype(np.float64) + sums.astype(np.float64) / (count.astype(np.float64) * 2.0 ** FRAC_BITS)[:, None]) * voxel
    return dict(first=rows[first_idx], coords=coords.astype(np.int32), count=count.astype(np.int32), sums=sums, mean=mean,
                dropped=int((~keep).sum()))
