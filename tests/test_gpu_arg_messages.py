"""The argument checks that only GPU tensors reach (they sit behind the device check of a wrapper, or need a
`DeepGlobalRegistration` object), with the exact exception type and message: the companion of test_arg_messages_cpu.py,
in the same form.  The strings are the ones the code raised before the checks were gathered in `_args.py`.  Every case
raises before a kernel is launched: a handful of rows is enough."""
import numpy as np
import pytest
import torch

from helpers import harness_dgr

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


@pytest.fixture(scope='module')
def world():
    """One object with synthetic weights, a two-fragment bank on its device (rows 0:2 and 2:5) and the same on the CPU."""
    from deepglobalregistration_amd import synth
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    ck = synth.synth_checkpoint(seed=0, voxel_size=0.05, feat_conv1_kernel_size=7)
    dgr = harness_dgr({'weights': ck, 'clip_weight_thresh': 0.05}, torch.device('cuda'))

    def bank(device, width=32):
        return FragmentBank.from_tensors(torch.zeros(5, 4, dtype=torch.int32, device=device), torch.zeros(5, 3, device=device),
                                         torch.zeros(5, width, device=device), np.array([0, 2, 5]))
    return dict(dgr=dgr, bank=bank('cuda'), narrow=bank('cuda', 16), cpu_bank=bank('cpu'))


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device='cuda')


def wrapper_cases():
    from deepglobalregistration_amd import ops
    width = 'F0 [N0,C] and F1 [N1,C] must share the feature width'
    offsets = 'off0 / off1 must be [npairs+1] row offsets covering F0 / F1'
    xyw = 'X, Y must be [N,3] and w [N] / [N,1]'
    nb = 2 ** 31 // (5 * 512) + 1                 # the first block count with 5 nb 8^3 >= 2^31; expanded views, no memory

    def mesh(blocks=z(2, 3, dtype=torch.int32), tsdf=z(2, 512), weight=z(2, 512, dtype=torch.int32)):
        return ops.check_tsdf_mesh_args(blocks, tsdf, weight, 0.01, 8, 1)
    return [
        # ---- the four k-NN wrappers: device, feature width, offsets --------------------------------------------------
        (lambda: ops.knn1(torch.zeros(3, 4), z(3, 4)), ValueError, 'expected a CUDA(ROCm) tensor'),
        (lambda: ops.knn1(z(3, 4), z(3, 5)), ValueError, width),
        (lambda: ops.knn1(z(3, 4), z(12)), ValueError, width),
        (lambda: ops.knn1_batch(z(3, 4), z(3, 5), [0, 3], [0, 3]), ValueError, width),
        (lambda: ops.knn(z(3), z(3, 4), 2), ValueError, width),
        (lambda: ops.knn_batch(z(3, 4), z(3, 5), [0, 3], [0, 3], 2), ValueError, width),
        (lambda: ops.knn_batch(z(3, 4), z(3, 5), [0, 2], [0, 3], 2), ValueError, width),      # the width before the offsets
        (lambda: ops.knn1_batch(z(3, 4), z(3, 4), [0, 2], [0, 3]), ValueError, offsets),
        (lambda: ops.knn1_batch(z(3, 4), z(3, 4), [0, 3], [0, 1, 3]), ValueError, offsets),
        (lambda: ops.knn1_batch(z(3, 4), z(3, 4), [3], [3]), ValueError, offsets),
        (lambda: ops.knn_batch(z(3, 4), z(3, 4), [1, 3], [0, 3], 2), ValueError, offsets),
        (lambda: ops.knn_batch(z(3, 4), z(3, 4), [0, 3], [0, 4], 2), ValueError, offsets),
        # ---- _xyw, inlier_inputs -------------------------------------------------------------------------------------
        (lambda: ops.weighted_procrustes(z(3, 3), z(4, 3), z(3)), ValueError, xyw),
        (lambda: ops.weighted_procrustes(z(3, 2), z(3, 2), z(3)), ValueError, xyw),
        (lambda: ops.se3_refine(z(3, 3), z(3, 3), z(4, 1)), ValueError, xyw),
        (lambda: ops.weighted_procrustes(np.zeros((3, 3)), z(3, 3), z(3)), ValueError, 'expected a CUDA(ROCm) tensor'),
        (lambda: ops.inlier_inputs(z(3, 4, dtype=torch.int32), z(3, 3), z(2, 4, dtype=torch.int32), z(2, 3),
                                   z(2, dtype=torch.int64)), ValueError, 'one correspondence per row of fragment 0 expected'),
        (lambda: ops.inlier_inputs(z(3, 4, dtype=torch.int32), z(3, 3), z(2, 4, dtype=torch.int32), z(2, 3),
                                   z(2, dtype=torch.int64), 'twos'), TypeError, 'Undefined feature type'),
        # ---- check_tsdf_mesh_args behind its device check -----------------------------------------------------------------
        (lambda: mesh(weight=torch.zeros(2, 512, dtype=torch.int32)), ValueError, 'weight must be a tensor on the GPU'),
        (lambda: mesh(blocks=z(2, 3, dtype=torch.int64)), ValueError, 'blocks must be int32 [nb,3], got torch.int64 (2, 3)'),
        (lambda: mesh(blocks=z(2, 4, dtype=torch.int32)), ValueError, 'blocks must be int32 [nb,3], got torch.int32 (2, 4)'),
        (lambda: mesh(tsdf=z(2, 4096)), ValueError, 'tsdf must be float32 [2,512], got torch.float32 (2, 4096)'),
        (lambda: mesh(tsdf=z(2, 512, dtype=torch.float64)), ValueError, 'tsdf must be float32 [2,512], got torch.float64 (2, 512)'),
        (lambda: mesh(weight=z(1, 512, dtype=torch.int32)), ValueError, 'weight must be int32 [2,512], got torch.int32 (1, 512)'),
        (lambda: mesh(weight=z(2, 512)), ValueError, 'weight must be int32 [2,512], got torch.float32 (2, 512)'),
        (lambda: mesh(z(1, 3, dtype=torch.int32).expand(nb, 3), z(1, 512).expand(nb, 512),
                      z(1, 512, dtype=torch.int32).expand(nb, 512)),
         ValueError, '838861 blocks of 8^3 voxels: 2^31 or more possible triangles'),
    ]


WRAPPER_CASES = 26


@pytest.mark.parametrize('k', range(WRAPPER_CASES))
def test_wrapper_checks(k):
    cases = wrapper_cases()
    assert len(cases) == WRAPPER_CASES
    call, kind, message = cases[k]
    with pytest.raises(Exception) as e:
        call()
    assert (type(e.value), str(e.value)) == (kind, message)


def test_register_entry_points(world):
    """The hook lengths and the offsets of `register_batch` / `register_pairs`, on the smallest inputs that reach them."""
    from deepglobalregistration_amd import ops
    dgr, bank = world['dgr'], world['bank']
    fcgf, inlier = dgr.fcgf_model._handle(), dgr.inlier_model._handle()
    c, x = z(3, 4, dtype=torch.int32), z(3, 3)

    def batch(off0=(0, 3), off1=(0, 3), **kw):
        return ops.register_batch(fcgf, inlier, c, x, list(off0), c, x, list(off1), 0.05, **kw)

    def pairs(ids=((0, 1),), off=(0, 2, 5), **kw):
        return ops.register_pairs(inlier, bank.coords, bank.xyz, bank.F, np.array(off), np.array(ids), 0.05, **kw)
    per_row = ' must have one entry per row of fragment 0'
    cases = [
        (lambda: batch(off0=(0, 2)), ValueError, 'offset arrays do not match the coordinate arrays'),
        (lambda: batch(off1=(0, 4)), ValueError, 'offset arrays do not match the coordinate arrays'),
        (lambda: batch(inlier_feature_type='twos'), KeyError, "'twos'"),
        (lambda: batch(forced_logit=z(2)), ValueError, 'forced_logit' + per_row),
        (lambda: batch(forced_logit=np.zeros((4, 1), np.float32)), ValueError, 'forced_logit' + per_row),
        (lambda: batch(override_idx1=z(4, dtype=torch.int64)), ValueError, 'override_idx1' + per_row),
        (lambda: batch(forced_logit=z(2), override_idx1=z(2, dtype=torch.int64)), ValueError, 'forced_logit' + per_row),
        (lambda: batch(forced_logit=z(2), inlier_feature_type='twos'), KeyError, "'twos'"),    # the record before the hooks
        (lambda: pairs(ids=(0, 1)), ValueError, 'pair_ids must be [npairs,2]'),
        (lambda: pairs(ids=((0, 1, 0),)), ValueError, 'pair_ids must be [npairs,2]'),
        (lambda: pairs(off=(0, 2, 4)), ValueError, 'offset array does not match the bank arrays'),
        (lambda: pairs(off=(5,)), ValueError, 'offset array does not match the bank arrays'),
        (lambda: pairs(forced_logit=z(3)), ValueError, 'forced_logit' + per_row),               # fragment 0 has 2 rows
        (lambda: pairs(ids=((1, 0), (0, 1)), forced_logit=z(4)), ValueError, 'forced_logit' + per_row),   # 3 + 2 rows
        (lambda: pairs(override_idx1=[0]), ValueError, 'override_idx1' + per_row),
        (lambda: pairs(forced_logit=z(1), override_idx1=z(1, dtype=torch.int64)), ValueError, 'forced_logit' + per_row),
    ]
    for call, kind, message in cases:
        with pytest.raises(Exception) as e:
            call()
        assert (type(e.value), str(e.value)) == (kind, message)


def test_scene_methods(world):
    """`DeepGlobalRegistration`'s own checks: the bank's device first, then what each method checks next."""
    dgr, bank, cpu_bank = world['dgr'], world['bank'], world['cpu_bank']
    where = 'the bank is on cpu, this object on cuda'
    ids_msg = 'pairs must be an [n,2] integer array'
    poses = np.stack([I4, I4])
    cases = [
        (lambda: dgr.register_pairs(cpu_bank, [[0, 1]]), ValueError, where),
        (lambda: dgr.score_pairs(cpu_bank, [[0, 1]], I4), ValueError, where),
        (lambda: dgr.optimize_scene(cpu_bank, [[0, 1]], I4), ValueError, where),
        (lambda: dgr.fuse_scene(cpu_bank, poses), ValueError, where),
        (lambda: dgr.score_pairs(cpu_bank, [0, 1], np.zeros(3), -1), ValueError, where),      # the device before the rest
        (lambda: dgr.fuse_scene(cpu_bank, I4, min_points=0), ValueError, where),
        (lambda: dgr.register_pairs(world['narrow'], [[0, 1]]), ValueError,
         'the bank holds 16-wide features, the FCGF model writes 32'),
        (lambda: dgr.register_pairs(bank, [[0, 2]]), ValueError, 'pair id outside [0, 2)'),
        (lambda: dgr.register_pairs(bank, [[0, 1]], batch_pairs=0), ValueError, 'batch_pairs must be at least 1'),
        (lambda: dgr.register_pairs(bank, [[0, 1]], forced_logits=[]), ValueError, 'forced_logits must have one entry per pair'),
        (lambda: dgr.score_pairs(bank, [0, 1], I4), ValueError, ids_msg),
        (lambda: dgr.score_pairs(bank, [], I4), ValueError, 'the pair list is empty'),
        (lambda: dgr.score_pairs(bank, [[0, 1]], I4, radius=0), ValueError, 'radius must be a positive finite number, got 0'),
        (lambda: dgr.score_pairs(bank, [[0, 1]], np.zeros((2, 4, 4))), ValueError, 'T must be [1,4,4], got (2, 4, 4)'),
        (lambda: dgr.score_pairs(bank, [[0, 1]], np.full((4, 4), np.nan)), ValueError, 'T must be finite (first three rows)'),
        (lambda: dgr.score_pairs(bank, [[0, 1]], np.zeros((4, 4))), ValueError, 'a pose cannot be inverted: Singular matrix'),
        (lambda: dgr.optimize_scene(bank, [0, 1], I4), ValueError, ids_msg),
        (lambda: dgr.optimize_scene(bank, [[0, 1]], np.zeros((3, 4))), ValueError, 'T must be [1,4,4], got (3, 4)'),
        (lambda: dgr.optimize_scene(bank, [[0, 1]], I4, reference_node=2), ValueError, 'reference node 2 outside [0, 2)'),
        (lambda: dgr.optimize_scene(bank, [[0, 1]], I4, edge_prune_threshold=2), ValueError,
         'edge_prune_threshold must lie in [0, 1]'),
        (lambda: dgr.optimize_scene(bank, [[0, 0]], I4), ValueError, 'a pair joins a fragment to itself'),
        (lambda: dgr.fuse_scene(bank, I4), ValueError, 'poses must be [2,4,4], got (4, 4)'),
        (lambda: dgr.fuse_scene(bank, torch.zeros(2, 4, 4), min_points=0), ValueError, 'min_points must be an integer >= 1, got 0'),
        (lambda: dgr.fuse_scene(bank, poses, min_points=True), ValueError, 'min_points must be an integer >= 1, got True'),
        (lambda: dgr.fuse_scene(bank, poses, min_points=2.0), ValueError, 'min_points must be an integer >= 1, got 2.0'),
        (lambda: dgr.fuse_scene(bank, poses, voxel_size=0), ValueError, 'voxel_size must be a positive finite number, got 0'),
        (lambda: dgr.fuse_scene(bank, poses, fragments=[2]), ValueError, 'fragment id outside [0, 2)'),
    ]
    for call, kind, message in cases:
        with pytest.raises(Exception) as e:
            call()
        assert (type(e.value), str(e.value)) == (kind, message)
