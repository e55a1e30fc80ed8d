"""What the eleven sums of `ops.score_pairs` (csrc/pairscore.hip) say about a registered pair: Open3D's `fitness` and
`inlier_rmse` (RegistrationResult) and its 6x6 information matrix (`get_information_matrix_from_point_clouds`, the record
of a 3DMatch / Redwood `.info` file).  Host arithmetic on [n,11] float64 arrays.

Open3D is not available here: the information matrix restates `GetInformationMatrixFromPointClouds` -- the sum of
G^T G over the correspondences with the rows

    G = [[ 0,  z, -y, 1, 0, 0],
         [-z,  0,  x, 0, 1, 0],
         [ y, -x,  0, 0, 0, 1]]        (x, y, z) = the TARGET point of the correspondence

in Open3D's order, rotation then translation -- in closed form from the first and second moments of the partners.  It is
not pinned against Open3D's output."""
import numpy as np


def _sums(sums):
    s = np.asarray(sums, np.float64)
    if s.ndim == 1:
        s = s[None]
    if s.ndim != 2 or s.shape[1] != 11:
        raise ValueError(f'sums must be [n,11], got {s.shape}')
    return s


def information_from_sums(sums):
    """[n,6,6]: Lambda = [[tr(M) I - M, [s]x], [[s]x^T, n I]] with M = sum q q^T, s = sum q and
    [s]x = [[0, -sz, sy], [sz, 0, -sx], [-sy, sx, 0]] -- the sum of G^T G above."""
    s = _sums(sums)
    n = len(s)
    xx, xy, xz, yy, yz, zz = (s[:, 5 + k] for k in range(6))
    M = np.stack((xx, xy, xz, xy, yy, yz, xz, yz, zz), 1).reshape(n, 3, 3)
    sx, sy, sz = s[:, 2], s[:, 3], s[:, 4]
    zero = np.zeros(n)
    S = np.stack((zero, -sz, sy, sz, zero, -sx, -sy, sx, zero), 1).reshape(n, 3, 3)
    eye = np.eye(3)[None]
    info = np.zeros((n, 6, 6))
    info[:, :3, :3] = (xx + yy + zz)[:, None, None] * eye - M
    info[:, :3, 3:] = S
    info[:, 3:, :3] = S.transpose(0, 2, 1)
    info[:, 3:, 3:] = s[:, 0, None, None] * eye
    return info


def scores_from_sums(sums, n_source_rows):
    """dict of per-pair arrays: `n_corr` int64 (source rows with a partner), `fitness` = n_corr / source rows,
    `inlier_rmse` = sqrt(sum d^2 / n_corr), 0 where n_corr = 0 (the ICP's convention, as is fitness 0 there),
    `information` [n,6,6]."""
    s = _sums(sums)
    rows = np.asarray(n_source_rows, np.float64).reshape(-1)
    if rows.shape != (len(s),):
        raise ValueError('one source row count per pair expected')
    n = s[:, 0]
    has = n > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        fitness = np.where(rows > 0, n / rows, 0.0)
        rmse = np.where(has, np.sqrt(s[:, 1] / np.where(has, n, 1.0)), 0.0)
    return {'n_corr': np.rint(n).astype(np.int64), 'fitness': fitness, 'inlier_rmse': rmse,
            'information': information_from_sums(s)}
