"""`util/pointcloud.py` of the reference: the ground-truth correspondence set of a pair, on the GPU."""
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
