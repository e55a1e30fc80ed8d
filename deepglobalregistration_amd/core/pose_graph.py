"""Host arithmetic around the pose-graph optimiser (`ops.pose_graph_optimize`, csrc/posegraph.hip): the edge residual
and the robust objective the solver minimises, the default line-process weight, the spanning-tree start, pruning and
connectivity.  float64 numpy throughout; nothing here touches the device.

Nodes are fragments with poses P_i (4x4, fragment i -> common frame).  Edge e = (s, t, X, Lambda, uncertain): X the pose of
s in t's frame (`register_pairs`' T for the pair (s, t)), Lambda the pair's 6x6 information matrix (`core.pair_score`,
rotation block first, accumulated over TARGET points).  With E = inv(P_t) P_s inv(X) and xi = (rotation vector of E,
translation of E), chi2 = xi^T Lambda xi = Lambda[3,3] * `eval.metrics.information_rmse`(inv(P_t) P_s, X, Lambda)^2.

    F*(P) = sum_certain chi2 + sum_uncertain mu chi2 / (mu + chi2)

is the objective of Choi, Zhou, Koltun (2015) with the line processes l = (mu / (mu + chi2))^2 eliminated.  `edge_residuals`
is the ONE Python statement of the residual (its device twin is `pg_residual` in csrc/posegraph.hip).  X and the poses are
taken as rigid: their inverse is [R^T | -R^T t] and their last row is ignored."""
import numpy as np


def _poses(P, name='P'):
    P = np.asarray(P, np.float64)
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError(f'{name} must be [n,4,4], got {P.shape}')
    return P


def _edges(edges, n=None):
    e = np.asarray(edges)
    if e.size == 0:
        return np.zeros((0, 2), np.int64)
    if e.ndim != 2 or e.shape[1] != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError('edges must be an [m,2] integer array')
    if n is not None and (bool((e < 0).any()) or bool((e >= n).any())):
        raise ValueError(f'edge id outside [0, {n})')
    return e.astype(np.int64)


def rigid_inverse(T):
    """[..., 4, 4]: [R^T | -R^T t] with the last row (0, 0, 0, 1)."""
    T = np.asarray(T, np.float64)
    out = np.zeros(T.shape)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def rotation_vectors(R):
    """`eval.metrics.rotation_vector` for a stack [m,3,3]: axis times angle, angle in [0, pi], with its care near 0 (the
    antisymmetric part is the vector) and near pi (the axis from the symmetric part, its sign from the antisymmetric
    one)."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    w = 0.5 * np.stack((R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]), 1)
    s = np.linalg.norm(w, axis=1)
    c = (np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0
    angle = np.arctan2(s, c)
    out = w.copy()
    big = s > 1e-6
    out[big] = w[big] * (angle[big] / s[big])[:, None]
    for k in np.nonzero(~big & (c <= 0))[0]:
        A = (R[k] + R[k].T) / 2.0 - c[k] * np.eye(3)
        j = int(np.argmax(np.diag(A)))
        a = A[j] / np.sqrt(max(A[j, j] * (1.0 - c[k]), 1e-300))
        if float(a @ w[k]) < 0.0:      # the symmetric part knows the axis up to its sign: that is the antisymmetric part's
            a = -a
        out[k] = a / np.linalg.norm(a) * angle[k]
    return out


def edge_residuals(P, edges, X):
    """(E [m,4,4], xi [m,6]) of every edge: E = inv(P_t) P_s inv(X), xi = (rotation vector of E, translation of E)."""
    P, X = _poses(P), _poses(X, 'X')
    edges = _edges(edges, len(P))
    if len(X) != len(edges):
        raise ValueError('one X per edge expected')
    E = rigid_inverse(P[edges[:, 1]]) @ P[edges[:, 0]] @ rigid_inverse(X)
    E[:, 3] = (0.0, 0.0, 0.0, 1.0)
    return E, np.concatenate((rotation_vectors(E[:, :3, :3]), E[:, :3, 3]), 1)


def edge_chi2(P, edges, X, info):
    """chi2 [m] = xi^T Lambda xi."""
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    _, xi = edge_residuals(P, edges, X)
    if len(info) != len(xi):
        raise ValueError('one information matrix per edge expected')
    return np.einsum('ea,eab,eb->e', xi, info, xi)


def line_process(chi2, uncertain, mu):
    """The closed-form minimiser l = (mu / (mu + chi2))^2 on the uncertain edges, 1 on the certain ones."""
    chi2 = np.asarray(chi2, np.float64)
    return np.where(np.asarray(uncertain, bool), (mu / (mu + chi2)) ** 2, 1.0)


def robust_objective(P, edges, X, info, uncertain, mu):
    """F*(P): sum of chi2 over the certain edges plus mu chi2 / (mu + chi2) over the uncertain ones."""
    if not mu > 0:
        raise ValueError('mu must be positive')
    chi2 = edge_chi2(P, edges, X, info)
    unc = np.asarray(uncertain, bool).reshape(-1)
    if unc.shape != chi2.shape:
        raise ValueError('one uncertain flag per edge expected')
    return float(np.where(unc, mu * chi2 / (mu + chi2), chi2).sum())


def default_mu(info, radius, preference_loop_closure=1.0):
    """preference_loop_closure * radius^2 * mean over the edges of Lambda[3,3] (the number of correspondences): an edge
    whose correspondences have RMSE `radius` under the graph's poses has chi2 ~ mu and l = 1/4.  An unpinned restatement
    of Open3D's ComputeLineProcessWeight."""
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    if len(info) == 0:
        raise ValueError('no edges')
    if not (radius > 0 and np.isfinite(radius)) or not (preference_loop_closure > 0 and np.isfinite(preference_loop_closure)):
        raise ValueError('radius and preference_loop_closure must be positive and finite')
    return float(preference_loop_closure * radius * radius * info[:, 3, 3].mean())


def prune_edges(line, uncertain, threshold=0.25):
    """kept [m] bool: every certain edge, and the uncertain ones with l >= threshold."""
    line, unc = np.asarray(line, np.float64).reshape(-1), np.asarray(uncertain, bool).reshape(-1)
    if line.shape != unc.shape:
        raise ValueError('one line-process value per edge expected')
    return ~unc | (line >= threshold)


def reachable_nodes(n, edges, kept=None, reference_node=0):
    """[n] bool: the nodes connected to `reference_node` through the kept edges."""
    edges = _edges(edges, n)
    if not 0 <= reference_node < n:
        raise ValueError(f'reference node outside [0, {n})')
    kept = np.ones(len(edges), bool) if kept is None else np.asarray(kept, bool).reshape(-1)
    adj = [[] for _ in range(n)]
    for (s, t), k in zip(edges, kept):
        if k:
            adj[s].append(t)
            adj[t].append(s)
    seen = np.zeros(n, bool)
    seen[reference_node] = True
    stack = [reference_node]
    while stack:
        for j in adj[stack.pop()]:
            if not seen[j]:
                seen[j] = True
                stack.append(j)
    return seen


def spanning_tree_poses(n, edges, X, weight, reference_node=0, uncertain=None):
    """(poses [n,4,4], reached [n] bool): the poses composed along a maximum spanning tree -- Kruskal over the edges
    ordered by (certain before uncertain when `uncertain` is given, larger `weight` first (Lambda[3,3], the number of
    correspondences), smaller index first) -- from P[reference_node] = I: P_s = P_t X along an edge (s, t, X).  Nodes the
    tree does not reach from the reference are reported in `reached` and keep the identity."""
    edges, X = _edges(edges, n), np.asarray(X, np.float64).reshape(-1, 4, 4)
    weight = np.asarray(weight, np.float64).reshape(-1)
    if not 0 <= reference_node < n:
        raise ValueError(f'reference node outside [0, {n})')
    if not len(edges) == len(X) == len(weight):
        raise ValueError('one X and one weight per edge expected')
    unc = np.zeros(len(edges), bool) if uncertain is None else np.asarray(uncertain, bool).reshape(-1)
    order = sorted(range(len(edges)), key=lambda k: (bool(unc[k]), -weight[k], k))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    adj = [[] for _ in range(n)]
    for k in order:
        s, t = int(edges[k, 0]), int(edges[k, 1])
        a, b = find(s), find(t)
        if a != b:
            parent[a] = b
            adj[s].append((t, k, True))     # from s, the far node is t
            adj[t].append((s, k, False))
    poses = np.tile(np.eye(4), (n, 1, 1))
    reached = np.zeros(n, bool)
    reached[reference_node] = True
    stack = [reference_node]
    while stack:
        i = stack.pop()
        for j, k, i_is_source in adj[i]:
            if reached[j]:
                continue
            # i = s, j = t: P_t = P_s inv(X);   i = t, j = s: P_s = P_t X
            poses[j] = poses[i] @ (rigid_inverse(X[k]) if i_is_source else X[k])
            poses[j, 3] = (0.0, 0.0, 0.0, 1.0)
            reached[j] = True
            stack.append(j)
    return poses, reached
