"""Registration error metrics of the reference's evaluation scripts."""
import numpy as np


def rte_rre(T_pred, T_gt, rte_thresh, rre_thresh, eps=1e-16):
    """scripts/test_3dmatch.py:38-46 (same in scripts/test_kitti.py): returns [success, RTE (m), RRE (deg)];
    a missing estimate counts as a failure with infinite errors."""
    if T_pred is None:
        return np.array([0, np.inf, np.inf])
    T_pred, T_gt = np.asarray(T_pred, np.float64), np.asarray(T_gt, np.float64)
    rte = float(np.linalg.norm(T_pred[:3, 3] - T_gt[:3, 3]))
    cos = (np.trace(T_pred[:3, :3].T @ T_gt[:3, :3]) - 1.0) / 2.0
    rre = float(np.degrees(np.arccos(np.clip(cos, -1 + eps, 1 - eps))))
    return np.array([float(rte < rte_thresh and rre < rre_thresh), rte, rre])


VALID_EPS = float(np.finfo(float).eps)   # core/trainer.py:34


def validation_statistics(counts, eps=VALID_EPS):
    """The inlier statistics of core/trainer.py:395, 443-448 (`_valid_epoch`) from validation counts [..., 6] =
    (n, hits, tp, fp, tn, fn) per batch entry (ops.validation_counts), summed over the entries like the reference's
    running tp / fp / tn / fn: hit_ratio = hits / n, precision, recall, f1, tpr, tnr, balanced_accuracy, with the
    reference's eps in every denominator."""
    c = np.asarray(counts, np.int64).reshape(-1, 6).sum(0)
    n, hits, tp, fp, tn, fn = (int(v) for v in c)
    precision = tp / (tp + fp + eps)
    recall = tp / (tp + fn + eps)
    f1 = 2 * (precision * recall) / (precision + recall + eps)
    tpr = tp / (tp + fn + eps)
    tnr = tn / (tn + fp + eps)
    return {'hit_ratio': hits / n if n else 0.0, 'precision': precision, 'recall': recall, 'f1': f1, 'tpr': tpr, 'tnr': tnr,
            'balanced_accuracy': (tpr + tnr) / 2}


def batch_rte_rre(R_pred, t_pred, T_gt):
    """core/metrics.py:25-43 as `_valid_epoch` uses them (core/trainer.py:418-420): per batch entry the translation error
    |t_pred - t_gt| and the rotation error arccos(clamp((tr(R_pred^T R_gt) - 1) / 2, -0.999, 0.999)) in degrees -- the
    reference's clamp, so a perfect rotation reads 2.56 degrees, not 0.  The ground truth is rounded to float32 as there."""
    R_pred, t_pred = np.asarray(R_pred, np.float64).reshape(-1, 3, 3), np.asarray(t_pred, np.float64).reshape(-1, 3)
    T_gt = np.asarray(T_gt, np.float32).astype(np.float64).reshape(-1, 4, 4)
    side = ((R_pred * T_gt[:, :3, :3]).sum((1, 2)) - 1) / 2
    rre = np.degrees(np.arccos(np.clip(side, -0.999, 0.999)))
    rte = np.linalg.norm(t_pred - T_gt[:, :3, 3], axis=1)
    return rte, rre


def rotation_vector(R):
    """The rotation vector (axis times angle, angle in [0, pi]) of a 3x3 rotation matrix."""
    R = np.asarray(R, np.float64)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # sin(angle) * axis
    s, c = float(np.linalg.norm(w)), (float(np.trace(R)) - 1.0) / 2.0
    angle = float(np.arctan2(s, c))
    if s > 1e-6:
        return w * (angle / s)
    if c > 0:                                   # angle -> 0: angle / sin(angle) -> 1
        return w
    # angle -> pi: the axis from the symmetric part R + R^T = 2 cos I + 2 (1 - cos) a a^T, which knows it up to its sign;
    # the sign is the antisymmetric part's (w = sin(angle) a, tiny here but not noise: |w| >~ 1e-9 against 1e-16), and
    # where w is exactly zero the angle is pi and both signs are logarithms
    A = (R + R.T) / 2.0 - c * np.eye(3)
    k = int(np.argmax(np.diag(A)))
    a = A[k] / np.sqrt(max(A[k, k] * (1.0 - c), 1e-300))
    if float(a @ w) < 0.0:
        a = -a
    return a / np.linalg.norm(a) * angle


def information_rmse(T_a, T_b, info):
    """The RMSE between the poses T_a and T_b over the correspondences that the 6x6 information matrix `info`
    summarises (`core.pair_score.information_from_sums`; a record of a `.info` file): sqrt(xi^T info xi / info[3,3]) with
    xi = (omega, v), omega the rotation vector of E = T_a T_b^-1 and v its translation; info[3,3] is the number of
    correspondences, `inf` when it is 0.  To first order in the rotation, xi^T info xi = sum |E q - q|^2 over the
    correspondences' target points q.  The 3DMatch / Redwood benchmark thresholds the same quantity (0.2 m) in its
    Matlab evaluation, which is not available here: the formula is derived from the definition of the information matrix,
    not copied from that code."""
    info = np.asarray(info, np.float64)
    if info.shape != (6, 6):
        raise ValueError(f'info must be [6,6], got {info.shape}')
    n = info[3, 3]
    if not n > 0:
        return float('inf')
    E = np.asarray(T_a, np.float64).reshape(4, 4) @ np.linalg.inv(np.asarray(T_b, np.float64).reshape(4, 4))
    xi = np.concatenate((rotation_vector(E[:3, :3]), E[:3, 3]))
    return float(np.sqrt(max(float(xi @ info @ xi), 0.0) / n))
