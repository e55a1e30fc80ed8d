"""`util/pointcloud.py` of the reference: the ground-truth correspondence set of a pair, the overlap ratio and the
averaging voxel down-sample in front of it, on the GPU."""
import numpy as np
import torch

from .. import ops


def _points(x):
    if hasattr(x, 'points') and not isinstance(x, np.ndarray) and not torch.is_tensor(x):   # o3d.geometry.PointCloud
        return np.asarray(x.points)
    return x


def get_matching_indices(source, target, trans, search_voxel_size, K=None):
    """util/pointcloud.py:83-96: every (i, j) with |trans . source[i] - target[j]| < search_voxel_size, in the reference's
    order (by i; within one i by distance, as Open3D's radius search returns them, equal distances by the smaller j; the
    first K of every i).  `source` / `target`: [N,3] arrays, tensors or objects with `.points`.  Returns an int64 [P,2]
    device tensor where the reference returns a list of tuples (`.tolist()` gives that list).  Points are searched as
    float32 -- what the voxelised clouds of this package are -- with the distances in float64 (csrc/gtmatch.hip)."""
    trans = trans.detach().cpu().numpy() if torch.is_tensor(trans) else np.asarray(trans)
    return ops.radius_pairs(_points(source), _points(target), trans, search_voxel_size, K)


def voxel_down_sample(pcd, voxel_size, origin=None):
    """Open3D's `pcd.voxel_down_sample(voxel_size)` as the reference calls it (util/pointcloud.py:74-75): every occupied
    voxel is replaced by the MEAN of its points (`ops.voxel_mean`, csrc/voxelmean.hip).  `pcd`: an [N,3] float32 / float64
    array or tensor (other dtypes are taken as float64) or an object with `.points`.  Returns the means as a float64 [V,3]
    device tensor, voxels in the order of their first point.
    `origin=None` puts the lattice where Open3D puts it: the cloud's minimum bound minus half a voxel, here the per-axis
    minimum over the points whose three coordinates are finite, widened to float64, minus 0.5 * voxel_size in float64.
    Open3D is absent, so this lattice is a restatement that is NOT pinned against it; the arithmetic of
    the means is this library's fixed-point definition (include/dgr_hip.h at dgr_voxel_mean), not Open3D's float sums:
    the two agree to rounding, not bit for bit."""
    x = _points(pcd)
    if not torch.is_tensor(x):
        x = np.asarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
    elif x.dtype not in (torch.float32, torch.float64):
        x = x.double()
    ops.check_voxel_mean_args(x, voxel_size, origin=origin)      # fail before anything is moved to the device
    if origin is None:
        x = ops._xyz_any_dev(x)
        finite = x[torch.isfinite(x).all(1)]
        if len(finite) == 0:
            raise ValueError('the cloud has no finite point')
        origin = (finite.min(0).values.double() - 0.5 * float(voxel_size)).cpu().numpy()
    return ops.voxel_mean(x, voxel_size, origin=origin)['xyz']


def compute_overlap_ratio(pcd0, pcd1, trans, voxel_size, downsample=True):
    """util/pointcloud.py:72-80: the larger of the two shares of points that have a partner strictly within `voxel_size`
    -- points of `pcd0` under `trans` against `pcd1`, points of `pcd1` under inv(trans) against `pcd0` -- the quantity
    behind the `@0.30` 3DMatch pair lists.  `pcd0` / `pcd1`: [N,3] arrays, tensors or objects with `.points`.
    `downsample=True` voxelises both clouds at `voxel_size` first, as the reference does, but with `ops.voxelize`, which
    KEEPS THE FIRST POINT of every voxel; Open3D's `voxel_down_sample` AVERAGES the points of a voxel, so the two
    down-sampled clouds differ by up to a voxel diagonal per point and the ratio is close to, not equal to, the
    reference's.  `downsample='mean'` averages instead, as the reference does (`voxel_down_sample` above, then float32).
    `downsample=False` takes the clouds as they are (already voxelised clouds, a bank's fragments).
    Both directions are one `ops.score_pairs` call on a two-fragment bank."""
    trans = trans.detach().cpu().numpy() if torch.is_tensor(trans) else np.asarray(trans)
    if trans.shape != (4, 4):
        raise ValueError(f'trans must be [4,4], got {trans.shape}')
    trans = np.array(trans, np.float64)
    ops.check_radius_args(voxel_size, None, trans, 1)          # fail before anything is moved to the device
    clouds = []
    for x in (_points(pcd0), _points(pcd1)):
        if isinstance(downsample, str) and downsample == 'mean':
            x = voxel_down_sample(x, voxel_size)
        elif downsample:
            x = ops.voxelize(x, voxel_size)[0]
        elif not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, np.float32))
        if x.dim() != 2 or x.shape[1] != 3 or len(x) == 0:
            raise ValueError(f'expected non-empty [N,3] points, got {tuple(x.shape)}')
        clouds.append(x.float())
    clouds[1] = clouds[1].to(clouds[0].device)
    trans[3] = (0, 0, 0, 1)
    sums = ops.score_pairs(torch.cat(clouds), [0, len(clouds[0]), len(clouds[0]) + len(clouds[1])], [[0, 1], [1, 0]],
                           np.stack((trans, np.linalg.inv(trans))), voxel_size)
    return max(float(sums[0, 0]) / len(clouds[0]), float(sums[1, 0]) / len(clouds[1]))
