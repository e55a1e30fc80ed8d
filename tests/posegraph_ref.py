"""The yardstick of the pose-graph tests (a helper module, not a conftest): a float64 numpy Levenberg-Marquardt of the
definition in `deepglobalregistration_amd.core.pose_graph` with analytic Jacobians -- the algorithm csrc/posegraph.hip
runs, restated on the host --, `scipy.optimize.least_squares` on the robust objective F* as the arbiter of that solver, and
a seeded generator of graphs with planted outliers.

Conventions.  Left perturbations P_i <- retract(delta_i) P_i with retract(omega, v) = [exp([omega]x) | v] (first-order
equal to the SE(3) exponential).  With E = inv(P_t) P_s inv(X), a perturbation of node s multiplies E from the left by
retract(Ad(inv(P_t)) delta_s), one of node t by the inverse of that, so d xi / d delta_s = D A = -d xi / d delta_t with
    A = [[R_t^T, 0], [[t']x R_t^T, R_t^T]],  t' = -R_t^T t_t          (the adjoint of inv(P_t), rotation rows first)
    D = [[Jl^-1(omega), 0], [-[t_E]x, I]]                             (Jl^-1: inverse left Jacobian of SO(3))."""
import numpy as np

from deepglobalregistration_amd.core import pose_graph as pg
from deepglobalregistration_amd.core.pair_score import information_from_sums

LAMBDA_INIT, LAMBDA_MIN, LAMBDA_MAX, STEP_TOL = 1e-6, 1e-12, 1e8, 1e-13   # the constants of csrc/posegraph.hip


def hat(w):
    w = np.asarray(w, np.float64)
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    return K


def so3_exp(w):
    """Rodrigues for a stack [..., 3]."""
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(-1)
    th = np.sqrt(th2)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    K = hat(w)
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def retract(delta, P):
    """[exp([omega]x) | v] . P for stacks delta [n,6], P [n,4,4]."""
    delta, P = np.asarray(delta, np.float64), np.asarray(P, np.float64)
    out = P.copy()
    R = so3_exp(delta[:, :3])
    out[:, :3, :3] = R @ P[:, :3, :3]
    out[:, :3, 3] = (R @ P[:, :3, 3:4])[..., 0] + delta[:, 3:]
    return out


def left_jacobian_inverse(w):
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(-1)
    th = np.sqrt(th2)
    small = th < 1e-3
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0 + th2 / 720.0, 1.0 / (ths * ths) - np.cos(ths / 2) / (2.0 * ths * np.sin(ths / 2)))
    K = hat(w)
    return np.eye(3) - 0.5 * K + c[..., None, None] * (K @ K)


def edge_jacobians(P, edges, X):
    """(xi [m,6], J [m,6,6]) with J = d xi / d delta_s; d xi / d delta_t = -J."""
    P = np.asarray(P, np.float64)
    edges = np.asarray(edges)
    E, xi = pg.edge_residuals(P, edges, X)
    Pt = P[edges[:, 1]]
    Rtt = np.swapaxes(Pt[:, :3, :3], 1, 2)
    tp = -(Rtt @ Pt[:, :3, 3:4])[..., 0]
    J = np.zeros((len(edges), 6, 6))
    J[:, :3, :3] = left_jacobian_inverse(xi[:, :3]) @ Rtt
    J[:, 3:, :3] = hat(tp - E[:, :3, 3]) @ Rtt
    J[:, 3:, 3:] = Rtt
    return xi, J


def _slots(n, ref):
    slot = np.arange(n)
    slot[ref + 1:] -= 1
    slot[ref] = -1
    return slot


MUTANTS = ('damp_identity', 'weight_not_squared', 'offdiag_half')


def _solve_normal(W, g, factor):
    """-W^-1 g through a triangular factor of W; LinAlgError where W is not positive definite.  'cholesky': LAPACK's.
    'eigh_qr': W = V diag(e) V^T = M^T M with M = diag(sqrt(e)) V^T, and M = Q R gives W = R^T R -- the same
    mathematical step by another road in float64, whose distance from the first is the rounding noise of a step."""
    if factor == 'cholesky':
        L = np.linalg.cholesky(W)
        return -np.linalg.solve(L.T, np.linalg.solve(L, g))
    if factor != 'eigh_qr':
        raise ValueError(f'unknown factor {factor!r}')
    e, V = np.linalg.eigh(W)
    if not (e > 0).all():
        raise np.linalg.LinAlgError('not positive definite')
    Rf = np.linalg.qr(np.sqrt(e)[:, None] * V.T, mode='r')
    return -np.linalg.solve(Rf, np.linalg.solve(Rf.T, g))


def lm_solve(n, edges, X, info, uncertain, P0, mu, reference_node=0, max_iter=100, rel_tol=1e-13, factor='cholesky',
             mutant=None):
    """Levenberg-Marquardt on F* with the line-process weights frozen inside an outer iteration (IRLS).  Returns a dict:
    poses, line_process, objective_initial, objective_final, iterations, converged, factorisations (attempted trial
    steps: accepted, rejected and failed ones), rejections (the trial steps that were not accepted) and decrease_ratio
    (the last accepted step's decrease of F* over the stopping threshold rel_tol F*; None without a step: `steps_check`
    reads from it whether `converged` was decided by more than rounding).
    `factor`: how the damped normal matrix is factored ('cholesky' | 'eigh_qr', `_solve_normal`).  `mutant`: None, or one
    deliberate error a test must notice -- 'damp_identity' (lambda I for lambda diag(H)), 'weight_not_squared' (sqrt(l)
    for l as the weight of B = l J^T Lambda J), 'offdiag_half' (the off-diagonal blocks of H halved)."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f'unknown mutant {mutant!r}')
    edges = np.asarray(edges, np.int64)
    X, info = np.asarray(X, np.float64), np.asarray(info, np.float64).reshape(-1, 6, 6)
    unc = np.asarray(uncertain, bool)
    P = np.asarray(P0, np.float64).copy()
    slot = _slots(n, reference_node)
    m = 6 * (n - 1)
    s_, t_ = edges[:, 0], edges[:, 1]

    def fstar(chi2):
        return float(np.where(unc, mu * chi2 / (mu + chi2), chi2).sum())

    def linearise(P):
        xi, J = edge_jacobians(P, edges, X)
        chi2 = np.einsum('ea,eab,eb->e', xi, info, xi)
        return xi, J, chi2

    xi, J, chi2 = linearise(P)
    F = F0 = fstar(chi2)
    lam, iterations, converged, factorisations, margin = LAMBDA_INIT, 0, False, 0, None
    off = 0.5 if mutant == 'offdiag_half' else 1.0
    for _ in range(max_iter):
        w = np.where(unc, mu / (mu + chi2), 1.0)           # sqrt(l)
        lw = w * w
        LJ = info @ J
        B = (w if mutant == 'weight_not_squared' else lw)[:, None, None] * (np.swapaxes(J, 1, 2) @ LJ)
        c = lw[:, None] * np.einsum('eba,eb->ea', LJ, xi)   # l J^T Lambda xi
        H, g = np.zeros((m, m)), np.zeros(m)
        for e in range(len(edges)):
            a, b = slot[s_[e]], slot[t_[e]]
            if a >= 0:
                H[6 * a:6 * a + 6, 6 * a:6 * a + 6] += B[e]
                g[6 * a:6 * a + 6] += c[e]
            if b >= 0:
                H[6 * b:6 * b + 6, 6 * b:6 * b + 6] += B[e]
                g[6 * b:6 * b + 6] -= c[e]
            if a >= 0 and b >= 0:
                H[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= off * B[e]
                H[6 * b:6 * b + 6, 6 * a:6 * a + 6] -= off * B[e]
        d = np.diag(H).copy()
        d[~(d > 0)] = 1.0
        const = float(np.where(unc, mu * (w - 1.0) ** 2, 0.0).sum())
        accepted = False
        while True:
            ok = True
            factorisations += 1
            try:
                delta = _solve_normal(H + lam * (np.eye(m) if mutant == 'damp_identity' else np.diag(d)), g, factor)
            except np.linalg.LinAlgError:
                ok = False
            if ok and np.isfinite(delta).all():
                full = np.zeros((n, 6))
                full[slot >= 0] = delta.reshape(n - 1, 6)[slot[slot >= 0]]
                Pt = retract(full, P)
                Pt[reference_node] = P[reference_node]
                chi2_t = pg.edge_chi2(Pt, edges, X, info)
                Ft = float((lw * chi2_t).sum()) + const
                if Ft <= F:
                    accepted = True
                    break
            lam *= 10.0
            if lam > LAMBDA_MAX:
                break
        if not accepted:
            converged = True      # no descent left at any damping: the numerical floor
            break
        P = Pt
        xi, J, chi2 = linearise(P)
        F_new = fstar(chi2)
        dec, F_old, F = F - F_new, F, F_new
        iterations += 1
        lam = max(lam * 0.1, LAMBDA_MIN)
        margin = dec / (rel_tol * F_old) if rel_tol * F_old > 0 else None
        if dec <= rel_tol * F_old or float(np.abs(delta).max()) <= STEP_TOL:
            converged = True
            break
    return {'poses': P, 'line_process': pg.line_process(chi2, unc, mu), 'objective_initial': F0, 'objective_final': F,
            'iterations': iterations, 'converged': converged, 'factorisations': factorisations,
            'rejections': factorisations - iterations, 'decrease_ratio': margin}


def scipy_solve(n, edges, X, info, uncertain, P0, mu, reference_node=0):
    """The arbiter: scipy's trust-region least squares on F* itself (residuals sqrt(w) L^T xi with Lambda = L L^T and
    w = mu / (mu + chi2) on the uncertain edges, 1 on the others), parametrised by left perturbations of P0."""
    from scipy.optimize import least_squares
    edges = np.asarray(edges, np.int64)
    info = np.asarray(info, np.float64).reshape(-1, 6, 6)
    unc = np.asarray(uncertain, bool)
    P0 = np.asarray(P0, np.float64)
    slot = _slots(n, reference_node)
    Lc = np.linalg.cholesky(info + 1e-12 * np.trace(info, axis1=1, axis2=2)[:, None, None] * np.eye(6) / 6)

    def poses(x):
        full = np.zeros((n, 6))
        full[slot >= 0] = x.reshape(n - 1, 6)[slot[slot >= 0]]
        P = retract(full, P0)
        P[reference_node] = P0[reference_node]
        return P

    def fun(x):
        _, xi = pg.edge_residuals(poses(x), edges, X)
        chi2 = np.einsum('ea,eab,eb->e', xi, info, xi)
        w = np.where(unc, mu / (mu + chi2), 1.0)
        return (np.sqrt(w)[:, None] * np.einsum('eba,eb->ea', Lc, xi)).reshape(-1)
    r = least_squares(fun, np.zeros(6 * (n - 1)), jac='3-point', method='trf', ftol=1e-15, xtol=1e-15, gtol=1e-15,
                      max_nfev=2000)
    P = poses(r.x)
    return {'poses': P, 'objective_final': pg.robust_objective(P, edges, X, info, unc, mu)}


# ----------------------------------------------------------------------------------------------------------------------
def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return so3_exp(axis * rng.uniform(0, max_angle))


def random_pose(rng, extent=3.0):
    T = np.eye(4)
    T[:3, :3] = random_rotation(rng)
    T[:3, 3] = rng.uniform(-extent, extent, size=3)
    return T


def random_information(rng, n_points=3000):
    """Lambda of about `n_points` correspondences whose target points are spread over a room-sized box."""
    k = int(n_points * rng.uniform(0.7, 1.3))
    q = rng.uniform((-3.0, -2.0, 0.0), (3.0, 2.0, 3.0), size=(k, 3)) * rng.uniform(0.5, 1.0) + rng.uniform(-0.5, 0.5, size=3)
    s = np.zeros(11)
    s[0] = k
    s[2:5] = q.sum(0)
    s[5:] = [(q[:, a] * q[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return information_from_sums(s)[0]


def make_graph(seed, n, n_outliers=0, closures=(2, 3), pose_noise=1e-2, chain_noise=1e-3, radius=0.1, ring=False,
               all_certain=False, reference_node=0, extra_edges=()):
    """A graph of `n` random poses: certain chain edges (i, i+1) with noise `chain_noise`, uncertain true closures
    (i, i+d) for d in `closures` with noise `pose_noise` (rotation rad and translation m, normal), `n_outliers` uncertain
    closures between random non-adjacent nodes with a random X, optionally the ring closure (n-1, 0).  `extra_edges`:
    (s, t) true closures appended last.  The initial poses are the chain of certain edges from the reference node.
    Returns a dict: n, edges, X, info, uncertain, outlier [m] bool, P_true, P_init, mu, reference_node."""
    rng = np.random.default_rng(seed)
    P_true = np.stack([random_pose(rng) for _ in range(n)])
    edges, X, unc, outlier = [], [], [], []

    def measured(s, t, noise):
        T = pg.rigid_inverse(P_true[t]) @ P_true[s]
        return retract(rng.normal(scale=noise, size=(1, 6)), T[None])[0]
    for i in range(n - 1):
        edges.append((i, i + 1)); X.append(measured(i, i + 1, chain_noise)); unc.append(False); outlier.append(False)
    true_closures = [(i, i + d) for d in closures for i in range(n - d)]
    if ring and n > 2:
        true_closures.append((n - 1, 0))
    true_closures += [tuple(e) for e in extra_edges]
    for s, t in true_closures:
        edges.append((s, t)); X.append(measured(s, t, pose_noise)); unc.append(not all_certain); outlier.append(False)
    for _ in range(n_outliers):
        while True:
            s, t = (int(v) for v in rng.integers(0, n, size=2))
            if abs(s - t) >= 2:
                break
        edges.append((s, t)); X.append(random_pose(rng)); unc.append(True); outlier.append(True)
    edges, X = np.asarray(edges, np.int64), np.stack(X)
    unc, outlier = np.asarray(unc, bool), np.asarray(outlier, bool)
    info = np.stack([random_information(rng) for _ in range(len(edges))])
    chain = ~unc if not all_certain else (np.arange(len(edges)) < n - 1)
    P_init, reached = pg.spanning_tree_poses(n, edges[chain], X[chain], info[chain, 3, 3], reference_node)
    assert reached.all()
    P_init = P_true[reference_node] @ P_init      # the gauge node sits at its true pose: a non-trivial fixed value
    return {'n': n, 'edges': edges, 'X': X, 'info': info, 'uncertain': unc, 'outlier': outlier, 'P_true': P_true,
            'P_init': P_init, 'mu': pg.default_mu(info, radius), 'reference_node': reference_node}


def solve_args(g):
    return (g['n'], g['edges'], g['X'], g['info'], g['uncertain'], g['P_init'], g['mu'], g['reference_node'])


def with_pi_edge(g, angle=np.pi - 1e-8, axis=(0.6, -0.48, 0.64)):
    """`g` plus one planted outlier whose residual rotation at the initial poses is `angle` about the unit vector `axis`:
    the rotation vector's branch next to pi.  (The default axis has a positive largest entry; (0.6, -0.64, 0.48) has a
    negative one, which is where a logarithm that signs the axis without looking at the antisymmetric part goes wrong.)"""
    s, t = 0, g['n'] - 1
    flip = np.eye(4)
    flip[:3, :3] = so3_exp(np.array(axis, np.float64) * angle)
    X = pg.rigid_inverse(flip) @ pg.rigid_inverse(g['P_init'][t]) @ g['P_init'][s]
    rng = np.random.default_rng(99)
    out = dict(g)
    out['edges'] = np.concatenate((g['edges'], [[s, t]]))
    out['X'] = np.concatenate((g['X'], X[None]))
    out['info'] = np.concatenate((g['info'], random_information(rng)[None]))
    out['uncertain'] = np.append(g['uncertain'], True)
    out['outlier'] = np.append(g['outlier'], True)
    return out


def with_perturbed_start(g, seed, scale=0.1):
    """`g` started `scale` (rad, m; normal) away from the chain of certain edges at every node but the reference: for graphs
    whose chain start is already the minimum."""
    out = dict(g)
    d = np.random.default_rng(seed).normal(scale=scale, size=(g['n'], 6))
    d[g['reference_node']] = 0.0
    out['P_init'] = retract(d, g['P_init'])
    return out


def suite_graphs():
    """name -> graph: the solvable cases of tests/test_gpu_pose_graph.py.  6 (n - 1) unknowns against the Cholesky panel
    width 8 and the 4x4 tiles of its trailing update: 6 (below one panel), 12, 18 (two above a multiple), 24, 48, 72 (at
    one), 66 (two above), 762 (the cap: 95 panels and a last one of two columns)."""
    return {
        'n2_one_edge': with_perturbed_start(make_graph(20, 2, 0, closures=()), 40),   # (F* = 0 at the chain start itself)
        'n3_triangle': make_graph(21, 3, 0, closures=(2,)),
        'n4': make_graph(22, 4, 1),
        'n5': make_graph(23, 5, 2),
        'n9': make_graph(24, 9, 5),
        'n12_10_outliers': make_graph(25, 12, 10),
        'n13': make_graph(26, 13, 6),
        'reference_node_5': make_graph(27, 8, 4, reference_node=5),
        'duplicate_edges': make_graph(28, 7, 3, extra_edges=((2, 4), (4, 2), (0, 1))),
        'all_certain': make_graph(29, 8, 0, all_certain=True),
        'rotation_near_pi': with_pi_edge(make_graph(30, 6, 2)),
        'n128_ring_with_chords': make_graph(31, 128, 40, ring=True),
    }


def side_by_side(a, b):
    """The graphs `a` and `b` as ONE graph: b's nodes after a's, no edge between the two, the reference node a's.  Nothing
    ties b's component to the gauge, so the normal matrix is singular but for the damping."""
    cat = lambda k: np.concatenate((a[k], b[k]))
    out = {k: cat(k) for k in ('X', 'info', 'uncertain', 'outlier', 'P_true', 'P_init')}
    out.update(n=a['n'] + b['n'], edges=np.concatenate((a['edges'], b['edges'] + a['n'])), reference_node=a['reference_node'],
               mu=pg.default_mu(out['info'], 0.1))
    return out


def with_isolated_node(g, seed):
    """`g` plus one node without an edge (degree 0: its rows of H are zero, its damping falls back to lambda * 1)."""
    out = dict(g)
    T = random_pose(np.random.default_rng(seed))[None]
    out.update(n=g['n'] + 1, P_true=np.concatenate((g['P_true'], T)), P_init=np.concatenate((g['P_init'], T)))
    return out


def with_rank1_information(g, weight=300.0, axis=3):
    """`g` with Lambda = weight * e e^T on every edge (e the unit vector `axis`; 3 is the first translation, so
    Lambda[3,3], the number of correspondences, stays positive): five of an edge's six residual directions cost nothing."""
    out = dict(g)
    out['info'] = np.zeros_like(g['info'])
    out['info'][:, axis, axis] = weight
    return out


NEGATIVE_AXIS = (0.6, -0.64, 0.48)      # a unit vector whose largest-magnitude entry is negative


def step_graphs():
    """name -> graph: what the k-step comparison adds to `suite_graphs` -- starts far enough from the chain for the
    reject / re-damp loop to run, nodes the reference node cannot reach, rank-deficient information, the reference node
    last, a residual rotation next to pi about an axis whose largest entry is negative."""
    n9, n13, two = make_graph(24, 9, 5), make_graph(26, 13, 6), side_by_side(make_graph(33, 5, 2), make_graph(34, 4, 1))
    return {
        'far_n9': with_perturbed_start(n9, 7, scale=1.0),
        'far_n13': with_perturbed_start(n13, 8, scale=2.0),
        'two_components': two,
        'two_components_far': with_perturbed_start(two, 9, scale=0.5),
        'isolated_node': with_isolated_node(make_graph(35, 6, 2), 36),
        'rank1_info': with_rank1_information(make_graph(23, 5, 2)),
        'reference_last': make_graph(32, 8, 4, reference_node=7),
        'pi_negative_axis_5e-7': with_pi_edge(make_graph(30, 6, 2), np.pi - 5e-7, NEGATIVE_AXIS),
        'pi_negative_axis_1e-8': with_pi_edge(make_graph(30, 6, 2), np.pi - 1e-8, NEGATIVE_AXIS),
    }


def step_class(name, g):
    """The noise class of a graph for the k-step comparison: 'n128' above 20 nodes, 'far' for the far or singular starts
    of `step_graphs`, 'suite' for the rest."""
    if g['n'] > 20:
        return 'n128'
    return 'far' if name.startswith(('far_', 'two_components', 'isolated_node', 'rank1_info', 'pi_')) else 'suite'


def ulp64(x):
    """64 ulp of |x|: the floor of a noise class whose measured maximum is only an ulp or two."""
    return 64 * float(np.spacing(abs(float(x))))


STEP_KS = (1, 2, 3, 5)
UNDECIDED = (0.25, 4.0)      # decrease / (rel_tol F*) of a step whose stopping decision is left to rounding


def objective_slack(g, P, ulps=4):
    """What F*(P) can differ by between two float64 evaluations, to first order: xi comes out of sums of products of
    matrix entries of order 1 and is known to a few ulp of 1 ABSOLUTELY, however small it is, so
    |d F*| <= sum_e l_e |d chi2_e| <= sum_e l_e 2 sqrt(chi2_e lambda_max(Lambda_e)) |d xi|, with |d xi| = `ulps` ulp of 1.
    On the graphs of this module it is 0.001 to 0.17 of 1e-12 F* (n3_triangle: a half); it decides where a graph is all but
    solved and a relative bound on F* asks for more digits of xi than float64 has (n2_one_edge after two steps: F* = 2e-11
    from xi ~ 1e-8, where two evaluations agree to 2e-9 relative and this term is 9e-19)."""
    chi2 = pg.edge_chi2(P, g['edges'], g['X'], g['info'])
    lmax = np.linalg.eigvalsh(np.asarray(g['info'], np.float64).reshape(-1, 6, 6))[:, -1]
    l = pg.line_process(chi2, g['uncertain'], g['mu'])
    return float(2.0 * ulps * np.finfo(np.float64).eps * (l * np.sqrt(chi2 * np.maximum(lmax, 0.0))).sum())


def steps_check(solve, g, ks=STEP_KS, tol=None, reference=None):
    """Holds a solver to the reference step by step.  For every k of `ks`: `solve(g, k)` (a dict with poses,
    objective_final, iterations, converged -- the solver under test stopped after at most k accepted steps) against
    `lm_solve(..., max_iter=k)`: the same number of accepted steps, the same `converged`, poses within `tol` (largest
    entry difference), and the reported objective within 1e-12 relative of `robust_objective` of the returned poses, plus
    `objective_slack`.  `reference`: a dict k -> reference result, filled as needed, so that several solvers share one
    reference.  Returns one record per k: (k, got, ref, pose difference).

    One exception, `UNDECIDED`: `converged` is not compared where the reference's last step lowered F* by between a quarter
    of and four times the stopping threshold rel_tol F* = 1e-13 F*.  F* carries relative rounding noise of that order
    itself (a residual rotation of 1e-3 rad read off a matrix with entries of 1 is known to eps / 1e-3 ~ 1e-13), so the
    flag is a coin there: at the fifth step of n3_triangle the two float64 factorisations of `lm_solve` lower F* by 0.51
    and 1.07 thresholds and disagree.  It is the only such case among the graphs of this module at k <= 5 (the next run that goes
    on lowers F* by 31 thresholds), which tests/test_pose_graph_cpu.py asserts; full runs end inside the band more often
    (n4, n5, far_n13: 0.3 .. 0.7), which is why a full run's step count is held to the reference's only within one."""
    if tol is None:
        raise ValueError('steps_check needs a pose tolerance')
    reference = {} if reference is None else reference
    rows = []
    for k in ks:
        if k not in reference:
            reference[k] = lm_solve(*solve_args(g), max_iter=k)
        ref, got = reference[k], solve(g, k)
        dp = float(np.abs(np.asarray(got['poses']) - ref['poses']).max())
        F = pg.robust_objective(got['poses'], g['edges'], g['X'], g['info'], g['uncertain'], g['mu'])
        assert int(got['iterations']) == ref['iterations'], f'k={k}: {int(got["iterations"])} accepted steps, reference {ref["iterations"]}'
        if ref['decrease_ratio'] is None or not UNDECIDED[0] < ref['decrease_ratio'] < UNDECIDED[1]:
            assert bool(got['converged']) == bool(ref['converged']), f'k={k}: converged {got["converged"]}, reference {ref["converged"]}'
        assert dp <= tol, f'k={k}: poses differ by {dp:.3e} > {tol:.3e}'
        assert abs(got['objective_final'] - F) <= 1e-12 * abs(F) + objective_slack(g, got['poses']), \
            f'k={k}: objective {got["objective_final"]!r}, F*(poses) {F!r}'
        rows.append((k, got, ref, dp))
    return rows
