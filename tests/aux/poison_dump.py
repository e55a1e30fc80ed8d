"""Helper of tests/test_gpu_workspace_poison.py: every public entry point once, at the smallest shapes that have
capacity slack and tile tails, every returned array to an .npz under 'family/case/name'.

    [DGR_WORKSPACE_FILL=<32-bit hex word>] python tests/aux/poison_dump.py OUT.npz

With the variable set, the library fills its workspace and private allocations with the word (csrc/ctx.hip), every input
lies between guard bands of the word (`poison.guarded`; checked untouched after each family) and every output `ops` allocates is a guarded view checked when
the call is over (`poison.Outputs`): a damaged band ends the process with its report and a non-zero exit.  Unset: no
guarding and no proxy, the plain product path.  No timings, stage times or kernel names are stored: every key is meant
to be the same bytes in every run."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import poison   # noqa: E402
from deepglobalregistration_amd import _lib, ops, synth   # noqa: E402

FAMILIES = ('peek', 'voxelize', 'nets', 'maps', 'knn', 'glue', 'registration', 'o3d', 'fused', 'grids', 'posegraph',
            'voxelmean', 'tsdf')
_env = os.environ.get('DGR_WORKSPACE_FILL')
WORD = None if _env is None else int(_env, 16)
RES = {}
INPUTS = []     # the guarded inputs of the family that is running
VOXEL = 0.05


def G(a, dtype=None):
    """A host array (or tensor) as a device tensor of `dtype`: between guard bands when a word is set."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    t = t.cuda().contiguous()
    return t if WORD is None else poison.guarded(t, WORD, INPUTS)


def outputs():
    return contextlib.nullcontext() if WORD is None else poison.Outputs(WORD)


def put(key, v):
    assert key not in RES, key
    if torch.is_tensor(v):
        v = v.detach().cpu()
        v = v.view(torch.int16).numpy().view(np.uint16) if v.dtype == torch.uint16 else v.numpy()
    RES[key] = np.ascontiguousarray(v)


def put_all(prefix, names, values):
    for n, v in zip(names, values):
        put(f'{prefix}/{n}', v)


# ----------------------------------------------------------------------------------------------------------------
def peek():
    buf = (C.c_uint32 * 1024)()
    _lib.check(_lib.load().dgr_debug_workspace_peek(_lib.get_ctx('cuda'), 1024, buf))
    put('peek/fresh/words', np.array(buf, np.uint32))          # a new chunk (DgrArena::alloc)
    rng = np.random.default_rng(0)
    ops.knn1(G(rng.standard_normal((70, 32)), torch.float32), G(rng.standard_normal((90, 32)), torch.float32))
    _lib.check(_lib.load().dgr_debug_workspace_peek(_lib.get_ctx('cuda'), 1024, buf))
    put('peek/after_a_call/words', np.array(buf, np.uint32))   # a chunk the arena keeps (DgrArena::reset)


def voxelize():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (1000, 3))
    for name, dt in (('f32', torch.float32), ('f64', torch.float64)):
        with outputs():
            put_all(f'voxelize/{name}', ('xyz', 'coords', 'sel'), ops.voxelize(G(x, dt), VOXEL, batch_index=3))


def _forward(net, coords, feats, prefix):
    with outputs():
        put(prefix + '/OUT', net.forward(G(coords, torch.int32), G(feats, torch.float32)))
    for t in ('S1', 'S8', 'U1'):
        for r in ('f32', 'amax'):
            try:
                put(f'{prefix}/{t}.{r}', net.tensor(t, r))
            except (RuntimeError, ValueError) as e:
                if 'did not write' not in str(e):
                    raise


def nets():
    import fcgf_wide_cases as fc
    import layer_trace_inputs as inp
    clouds = inp.clouds()
    for name, (D, cin, cout, ks, norm, _, cl) in inp.NETS.items():
        net = ops.NetHandle(inp.state_dict(name), D, cin, cout, ks, norm)
        for c in cl:
            _forward(net, clouds[c], inp.feats(name, c, len(clouds[c])), f'nets/{name}.{c}')
    net = ops.NetHandle(synth.synth_state_dict(3, 1, 32, fc.CONV1_KS, fc.SEED), 3, 1, 32, fc.CONV1_KS, True, wide_coarse=True)
    case = next(c for c in fc.CASES if c.name == 'a_two_small')
    _forward(net, case.coords, np.ones((len(case.coords), 1), np.float32), 'nets/fcgf_wide.a_two_small')


def maps():
    import maps_cases as mc
    for case, ks in ((next(c for c in mc.CASES_3D if c.name == 'rows513'), 5),
                     (next(c for c in mc.CASES_6D if c.name == 'replay_strided'), 3)):
        for lean in (False, True):
            p = f'maps/{case.D}d.{case.name}.{"lean" if lean else "full"}'
            m = ops.Maps(G(case.coords, torch.int32), case.D, ks, lean=lean)
            for ts in (1, 2, 4, 8):
                put(f'{p}/coords.{ts}', m.coords(ts))
            kinds = [('same', ts) for ts in (1, 2, 4, 8)] + [('down', ts) for ts in (1, 2, 4)] + [('conv1', 1)]
            if case.D == 3:
                kinds += [('nbr_same', ts) for ts in (1, 2, 4, 8)] + [('nbr_down', ts) for ts in (1, 2, 4)] + \
                         [('nbr_up', ts) for ts in (1, 2, 4)]
            for kind, ts in kinds:
                try:
                    got = m.kernel_map(kind, ts)
                except ValueError:      # a map this build does not make (a lean 3-D object has tables only): in every run
                    continue
                put_all(f'{p}/{kind}.{ts}', ('k', 'in', 'out'), got)
            del m


def _knn_single(name, F0, F1):
    F0, F1 = G(F0), G(F1)
    with outputs():
        put_all(f'knn/{name}/knn1', ('idx', 'dist'), ops.knn1(F0, F1, return_distance=True))
        for k in (1, 8, 32):
            put_all(f'knn/{name}/k{k}', ('idx', 'dist'), ops.knn(F0, F1, k, return_distance=True))
            put(f'knn/{name}/k{k}.sq.idx', ops.knn(F0, F1, k, squared=True))


def knn():
    rng = np.random.default_rng(3)

    def feats(n, c):
        f = rng.standard_normal((n, c)).astype(np.float32)
        return f / np.linalg.norm(f, axis=1, keepdims=True)
    F0, F1 = feats(1200, 32), feats(1500, 32)
    _knn_single('c32.1200x1500', F0, F1)
    # 64 identical reference rows and 300 queries next to them: more exact candidates than a query's slots hold
    F0, F1 = F0.copy(), F1.copy()
    F1[100:164] = F1[100]
    F0[:300] = F1[100] + 1e-3 * rng.standard_normal((300, 32)).astype(np.float32)
    _knn_single('c32.identical_refs', F0, F1)
    _knn_single('c16.120x260', feats(120, 16), feats(260, 16))
    _knn_single('c64.80x200', feats(80, 64), feats(200, 64))
    _knn_single('c32.300x20', feats(300, 32), feats(20, 32))     # k = 32 > N1
    sizes = [(700, 1500), (33, 5), (300, 1025)]
    off0 = np.cumsum([0] + [a for a, _ in sizes])
    off1 = np.cumsum([0] + [b for _, b in sizes])
    F0, F1 = G(feats(off0[-1], 32)), G(feats(off1[-1], 32))
    with outputs():
        put_all('knn/batch/knn1', ('idx', 'dist'), ops.knn1_batch(F0, F1, off0, off1, return_distance=True))
        for k in (1, 8, 32):
            put_all(f'knn/batch/k{k}', ('idx', 'dist'), ops.knn_batch(F0, F1, off0, off1, k, return_distance=True))


def glue():
    rng = np.random.default_rng(4)
    n0, n1 = 300, 257
    c0 = np.concatenate([np.zeros((n0, 1)), rng.integers(-20, 20, (n0, 3))], 1)
    c1 = np.concatenate([np.zeros((n1, 1)), rng.integers(-20, 20, (n1, 3))], 1)
    x0, x1 = rng.uniform(-1, 1, (n0, 3)), rng.uniform(-1, 1, (n1, 3))
    idx1 = rng.integers(0, n1, n0)
    a = (G(c0, torch.int32), G(x0, torch.float32), G(c1, torch.int32), G(x1, torch.float32), G(idx1, torch.int64))
    with outputs():
        for ft in ('coords', 'ones'):
            put_all(f'glue/inlier_inputs.{ft}', ('coords6', 'feats'), ops.inlier_inputs(*a, ft))
        w, s = ops.sigmoid_clip_sum(G(rng.uniform(-4, 4, 200), torch.float32), 0.05)     # one workgroup: one order of the sum
        put('glue/sigmoid_clip_sum/w', w)
        put('glue/sigmoid_clip_sum/sum', np.array(s, np.float64))
        put('glue/gather_rows3/out', ops.gather_rows3(a[3], a[4]))


def registration():
    import reg_checks as rc
    for n in (300, 4097, 16385):          # clusters of 1, 2 and 8 workgroups
        X, Y, outl = rc.geometry(n)
        w = rc.weights('a', n, outl)
        X, Y, w = G(X), G(Y), G(w)
        put_all(f'registration/procrustes.{n}', ('R', 't'), ops.weighted_procrustes(X, Y, w))
        R, t, st = ops.se3_refine(X, Y, w, quantization_size=2 * VOXEL, max_iter=10)
        put_all(f'registration/refine.{n}', ('R', 't', 'iterations', 'loss', 'break_count'),
                (R, t, np.array(st['iterations']), np.array(st['loss'], np.float32), np.array(st['break_count'])))


def o3d():
    import o3d_cases as oc
    for name in ('n0:257', 'cell_doubling'):
        case = oc.icp_case(name)
        T, fit, rmse, it = ops.icp_point_to_point(G(case['src']), G(case['dst']), case['max_dist'], init=case['init'],
                                                  **oc.ops_kw(case))
        put_all(f'o3d/icp.{name.replace(":", "")}', ('T', 'fitness', 'rmse', 'iterations'), (T, np.array(fit), np.array(rmse), np.array(it)))
    X, Y = oc.corr_problem(513)
    T, best, count, rmse = ops.ransac_correspondence(G(X), G(Y), oc.RS_THR, 2000, seed=0)
    put_all('o3d/ransac.513', ('T', 'best', 'count', 'rmse'), (T, np.array(best), np.array(count), np.array(rmse)))


def fused():
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    ck = synth.synth_checkpoint(seed=0, voxel_size=VOXEL, feat_conv1_kernel_size=7)
    dgr = DeepGlobalRegistration({'weights': ck, 'clip_weight_thresh': 0.05, 'ransac_max_iteration': 20000}, torch.device('cuda'))
    # the ragged batch of test_gpu_pipeline.py::test_ragged_and_tiny_batches
    rng = np.random.default_rng(5)
    tiny0, tiny1 = rng.uniform(0, 0.4, (60, 3)), rng.uniform(0, 0.4, (45, 3))
    single = np.array([[0.01, 0.02, 0.03]])
    big0, big1, _ = synth.synth_pair(0, n_raw=6000)
    x0, c0, x1, c1, off0, off1 = [], [], [], [], [0], [0]
    for p, (a, b) in enumerate([(tiny0, tiny1), (big0, single), (big0, big1)]):
        xa, ca, _ = dgr.preprocess(a, batch_index=p)
        xb, cb, _ = dgr.preprocess(b, batch_index=p)
        x0.append(xa); c0.append(ca); x1.append(xb); c1.append(cb)
        off0.append(off0[-1] + len(xa)); off1.append(off1[-1] + len(xb))
    with outputs():
        T, status, _ = dgr.register_voxelized(G(torch.cat(c0)), G(torch.cat(x0)), off0, G(torch.cat(c1)), G(torch.cat(x1)), off1,
                                              safeguard=True, icp=True)
        put_all('fused/ragged', ('T', 'status'), (T, status))
        for which in ('idx1', 'logit', 'F0'):
            put(f'fused/ragged/{which}', ops.batch_output('cuda', which))
    # one register_pairs call over a three-fragment bank
    clouds, _, _ = synth.synth_scene(5, 3, n_raw=3000)
    bank = dgr.extract_fragments(clouds)
    bank = FragmentBank.from_tensors(G(bank.coords), G(bank.xyz), G(bank.F), bank.off)
    with outputs():
        T, status, _ = dgr.register_pairs(bank, [(0, 1), (1, 2), (2, 0)], batch_pairs=3, safeguard=True, icp=True)
        put_all('fused/pairs', ('T', 'status'), (T, status))


def _poses(rng, n, deg=20.0, shift=0.2):
    T = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        a = np.deg2rad(rng.uniform(-deg, deg))
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        T[k, :3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        T[k, :3, 3] = rng.uniform(-shift, shift, 3)
    return T


def grids():
    rng = np.random.default_rng(6)
    for sizes in ([63], [65], [300, 0, 4097, 64]):
        tag = '_'.join(str(s) for s in sizes)
        off0 = np.cumsum([0] + sizes)
        sizes1 = [max(0, s - 3) if s != 64 else 0 for s in sizes]         # other sizes on the other side; one side empty once
        off1 = np.cumsum([0] + sizes1)
        T = _poses(rng, len(sizes))
        x0 = rng.uniform(-0.5, 0.5, (off0[-1], 3)).astype(np.float32)
        x1 = np.zeros((off1[-1], 3), np.float32)
        for p in range(len(sizes)):       # x1 = some rows of x0 under the pose, moved by less than the radius
            src = x0[off0[p]:off0[p + 1]][:sizes1[p]].astype(np.float64)
            x1[off1[p]:off1[p + 1]] = src @ T[p, :3, :3].T + T[p, :3, 3] + rng.normal(0, 0.02, src.shape)
        gx0, gx1 = G(x0), G(x1)
        found = {}
        with outputs():
            for K in (None, 2):
                pairs, pair_off = ops.radius_pairs_batch(gx0, off0, gx1, off1, T, 0.06, K=K)
                put_all(f'grids/radius.{tag}.K{K}', ('pairs', 'pair_off'), (pairs, pair_off))
                found[K] = (pairs, pair_off)
        # predicted pairs: the capped list with every third pair replaced; labels against the full list
        pos, pos_off = found[None]
        pred, pred_off = found[2][0].cpu().numpy().copy(), found[2][1]
        for p in range(len(sizes)):
            seg = pred[pred_off[p]:pred_off[p + 1]]
            if sizes1[p]:
                seg[::3, 1] = rng.integers(0, sizes1[p], len(seg[::3]))
        M = np.maximum(np.array(sizes), np.array(sizes1)) + 1
        with outputs():
            label = ops.pairs_isin(G(pos), pos_off, G(pred), pred_off, M)
            put(f'grids/isin.{tag}/label', label)
            wts = rng.uniform(0, 1, len(pred)).astype(np.float32)
            put(f'grids/validation.{tag}/counts', ops.validation_counts(G(label.clone()), G(wts), pred_off))
    # pair scoring: every ordered pair of a bank of 65, 257 and 1000 points
    off = np.array([0, 65, 322, 1322])
    world = rng.uniform(-0.5, 0.5, (1000, 3))
    pose = _poses(rng, 3)
    inv = np.linalg.inv(pose)
    xyz = np.concatenate([(world[:off[f + 1] - off[f]] @ pose[f, :3, :3].T + pose[f, :3, 3] + rng.normal(0, 0.01, (off[f + 1] - off[f], 3)))
                          for f in range(3)]).astype(np.float32)
    ids = np.array([(i, j) for i in range(3) for j in range(3) if i != j])
    T = np.stack([pose[j] @ inv[i] for i, j in ids])
    put('grids/score_pairs/sums', ops.score_pairs(G(xyz), off, ids, T, 0.06))


def posegraph():
    import posegraph_ref as R
    g = R.suite_graphs()
    graphs = [g[k] for k in ('n2_one_edge', 'n5', 'n13', 'n128_ring_with_chords')]
    noff = np.cumsum([0] + [x['n'] for x in graphs])
    eoff = np.cumsum([0] + [len(x['edges']) for x in graphs])
    cat = lambda k: np.concatenate([x[k] for x in graphs])   # noqa: E731
    P, line, stats = ops.pose_graph_optimize(noff, eoff, cat('edges'), cat('X'), cat('info'), cat('uncertain'), cat('P_init'),
                                             [(x['mu'], x['reference_node']) for x in graphs])
    put_all('posegraph/four_graphs', ('poses', 'line', 'stats'), (P, line, stats))


def voxelmean():
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.4, 0.4, (65 + 4097, 3)).astype(np.float32)
    with outputs():
        r = ops.voxel_mean(G(x), VOXEL, [0, 65, 65 + 4097], None, _poses(rng, 2, 5.0, 0.05), return_sums=True)
        for k in ('xyz', 'coords', 'count', 'first', 'sums'):
            put(f'voxelmean/two_fragments/{k}', r[k])
        put('voxelmean/two_fragments/dropped', np.array(r['dropped']))


def tsdf():
    import tsdf_cases
    s = tsdf_cases.SIZES['small']
    depth, K, poses, _ = tsdf_cases.sequence('small')
    with outputs():
        vol = ops.tsdf_fragment(G(depth.copy()), K, poses, s['voxel'], s['trunc'], block=8, stride=4, return_volume=True)
        for k in ('xyz', 'blocks', 'tsdf', 'weight'):
            put(f'tsdf/small.fragment/{k}', vol[k])
    with outputs():
        r = ops.tsdf_mesh(G(vol['blocks']), G(vol['tsdf']), G(vol['weight']), s['voxel'], block=8)
        for k in ('xyz', 'normal', 'triangles'):
            put(f'tsdf/small.mesh/{k}', r[k])


def main(path):
    for fam in FAMILIES:
        fn = globals()[fam]
        before = len(RES)
        fn()
        torch.cuda.synchronize()
        if WORD is not None:     # no call wrote to an input or next to one
            poison.check_inputs(INPUTS, WORD, fam)
        INPUTS.clear()
        assert len(RES) > before and all(k.startswith(fam + '/') for k in list(RES)[before:]), fam
        print(f'{fam}: {len(RES) - before} keys', flush=True)
    np.savez(path, **RES)


if __name__ == '__main__':
    try:
        main(sys.argv[1])
    except poison.BandDamaged as e:
        print(f'BAND DAMAGED: {e}', file=sys.stderr, flush=True)
        sys.exit(3)
