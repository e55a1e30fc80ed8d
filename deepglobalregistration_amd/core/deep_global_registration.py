"""`DeepGlobalRegistration` with the reference's constructor / `register()` / stage-method
surface (core/deep_global_registration.py:67-324), executed on one MI355X by libdgr_hip.so.

Scope: steps 0-5 of `register()` -- voxelisation, FCGF features, feature
matching, 6-D inlier network, confidence gate, weighted Procrustes + robust refinement -- plus the two
Open3D steps around it, re-implemented on the GPU: the safeguard RANSAC from the
putative correspondences (:50-64, 302-315) when the confidence gate fails (an SVD failure leaves T = identity,
exactly like the reference's `except RuntimeError` branch :295-300), and the final point-to-point ICP (:317-322) when `use_icp` is set (the reference's default, :75).  The
`fcgf_feature_matching` safeguard variant (:31-46) is not implemented.
"""
import os

import numpy as np
import torch

from .. import _args, _lib, ops
from ..model import load_model
from ..sparse import SparseTensor
from ..util.timer import Timer
from .knn import find_knn_gpu
from .registration import GlobalRegistration


def _cfg_get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _cfg_has(cfg, key):
    return (key in cfg) if isinstance(cfg, dict) else hasattr(cfg, key)


class DeepGlobalRegistration:
    def __init__(self, config, device=torch.device('cuda')):
        self.config = config
        self.clip_weight_thresh = _cfg_get(config, 'clip_weight_thresh', 0.05)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DeepGlobalRegistration (MI355X build) runs on the GPU only')
        _lib.load()                      # fail loudly here if the HIP extension is missing
        self.safeguard_method = 'correspondence'
        self.use_icp = bool(_cfg_get(config, 'use_icp', True))   # reference: self.use_icp = True (:75)
        self.ransac_seed = int(_cfg_get(config, 'ransac_seed', 0))
        # the reference hard-codes RANSACConvergenceCriteria(4000000, ...) (:61); a config key so that parity tests can
        # give both sides a count the CPU oracle finishes
        self.ransac_max_iteration = int(_cfg_get(config, 'ransac_max_iteration', 4000000))
        # optional runtime key: keep the correspondences and logits of the last register() call (`last_corres_idx1`,
        # `last_logit`: device tensors that stay alive until the next call) for inspection -- tools/check_me_conventions.py
        # and the parity tests read them; off by default
        self.keep_intermediates = bool(_cfg_get(config, 'keep_intermediates', False))
        self.last_corres_idx1 = None
        self.last_logit = None
        self.last_wsum = None
        self.feat_timer = Timer()
        self.reg_timer = Timer()
        self.last_status = None
        self.last_stats = None
        self.last_icp = None

        weights = _cfg_get(config, 'weights')
        if isinstance(weights, (str, os.PathLike)):
            assert os.path.exists(weights), weights
            state = torch.load(weights, map_location='cpu', weights_only=False)
        elif isinstance(weights, dict):
            state = weights              # in-memory checkpoint (synthetic weights, tests)
        else:
            raise ValueError('config.weights must be a checkpoint path or a checkpoint dict')
        network_config = state['config']
        self.network_config = network_config
        self.inlier_feature_type = _cfg_get(network_config, 'inlier_feature_type', 'coords')
        self.voxel_size = _cfg_get(network_config, 'voxel_size')

        # FCGF network (:94-116); legacy checkpoints use un-prefixed keys (:104-112)
        if _cfg_has(network_config, 'feat_model'):
            name, n_out, ks = (_cfg_get(network_config, 'feat_model'), _cfg_get(network_config, 'feat_model_n_out'),
                               _cfg_get(network_config, 'feat_conv1_kernel_size'))
        else:
            name, n_out, ks = (_cfg_get(network_config, 'model'), _cfg_get(network_config, 'model_n_out'),
                               _cfg_get(network_config, 'conv1_kernel_size'))
        FCGFModel = load_model(name)
        if FCGFModel is None:
            raise NotImplementedError(f'feature model {name!r}: only ResUNetBN2C is implemented')
        self.fcgf_model = FCGFModel(1, n_out, bn_momentum=_cfg_get(network_config, 'bn_momentum', 0.05),
                                    conv1_kernel_size=ks,
                                    normalize_feature=_cfg_get(network_config, 'normalize_feature'))
        # optional runtime keys: the MinkowskiEngine conventions the checkpoint was written under (model/me_conventions.py)
        me_conv = {'kernel_order': _cfg_get(config, 'me_kernel_order', 'first_axis_fastest'),
                   'transposed_mirrored': bool(_cfg_get(config, 'me_transposed_mirrored', False))}
        self.fcgf_model.me_conventions = dict(me_conv)
        # optional runtime key `share_weights_with`: another DeepGlobalRegistration of the same checkpoint on this device
        # (one object per HIP stream / library context): its device-resident weights are used, not a second copy
        shared = _cfg_get(config, 'share_weights_with')
        if shared is not None:
            self.fcgf_model.share_weights(shared.fcgf_model)
        else:
            self.fcgf_model.load_state_dict(state['state_dict'])
        self.fcgf_model = self.fcgf_model.to(self.device).eval()

        # inlier network (:118-131)
        num_feats = 6 if self.inlier_feature_type == 'coords' else 1
        InlierModel = load_model(_cfg_get(network_config, 'inlier_model'))
        if InlierModel is None:
            raise NotImplementedError('inlier model: only ResUNetBN2C is implemented')
        self.inlier_model = InlierModel(num_feats, 1, bn_momentum=_cfg_get(network_config, 'bn_momentum', 0.05),
                                        conv1_kernel_size=_cfg_get(network_config, 'inlier_conv1_kernel_size'),
                                        normalize_feature=False, D=6)
        self.inlier_model.me_conventions = dict(me_conv)
        if shared is not None:
            self.inlier_model.share_weights(shared.inlier_model)
        else:
            self.inlier_model.load_state_dict(state['state_dict_inlier'])
        self.inlier_model = self.inlier_model.to(self.device).eval()
        self.nn_max_n = _cfg_get(network_config, 'nn_max_n', 250)

    # ---- stage methods, same names and argument order as the reference -------------------------
    def preprocess(self, pcd, batch_index=0):
        """Stage 0 (:134-161).  Returns xyz f32 [N,3] (device), coords i32 [N,4] (device),
        feats ones [N,1]."""
        if hasattr(pcd, 'points') and not isinstance(pcd, np.ndarray):   # o3d.geometry.PointCloud
            xyz = np.array(pcd.points)
        elif isinstance(pcd, np.ndarray):
            xyz = pcd
        elif torch.is_tensor(pcd):
            xyz = pcd
        else:
            raise Exception('Unrecognized pcd type')
        xyz_sel, coords, _ = ops.voxelize(xyz, self.voxel_size, batch_index, self.device)
        feats = torch.ones(len(xyz_sel), 1, device=self.device)
        return xyz_sel, coords, feats

    def fcgf_feature_extraction(self, feats, coords):
        """Step 1 (:163-169)."""
        sinput = SparseTensor(feats, coordinates=coords, device=self.device)
        return self.fcgf_model(sinput).F

    def fcgf_feature_matching(self, feats0, feats1):
        """Step 2 (:171-183)."""
        nns = find_knn_gpu(feats0, feats1, nn_max_n=self.nn_max_n, knn=1, return_distance=False)
        corres_idx0 = torch.arange(len(nns), device=self.device).long()
        corres_idx1 = nns.long().reshape(-1)
        return corres_idx0, corres_idx1

    def inlier_feature_generation(self, xyz0, xyz1, coords0, coords1, fcgf_feats0, fcgf_feats1,
                                  corres_idx0, corres_idx1):
        """Step 3 (:185-208).  corres_idx0 must be arange(N0), as produced by step 2."""
        assert len(corres_idx0) == len(corres_idx1)
        feat_type = self.inlier_feature_type
        assert feat_type in ['ones', 'feats', 'coords']
        if feat_type == 'feats':
            raise TypeError("inlier_feature_type 'feats' is inconsistent with the network input width "
                            'in the reference (deep_global_registration.py:119) and is not supported')
        _, feat = ops.inlier_inputs(coords0, xyz0, coords1, xyz1, corres_idx1, feat_type)
        return feat

    def inlier_prediction(self, inlier_feats, coords):
        """Step 4 (:210-217)."""
        sinput = SparseTensor(inlier_feats, coordinates=coords, device=self.device)
        return self.inlier_model(sinput).F

    def safeguard_registration(self, pcd0, pcd1, idx0, idx1, feats0, feats1, distance_threshold,
                               num_iterations):
        """Safeguard (:219-236): RANSAC over the putative correspondences.  `pcd0` / `pcd1` are the
        voxelised xyz tensors (the reference wraps them into Open3D clouds).  Like the reference's call
        (RANSACConvergenceCriteria(4000000, num_iterations) with the second argument clamped to
        confidence 1.0), all 4 000 000 hypotheses (`ransac_max_iteration`) are evaluated; `num_iterations` is accepted
        and unused."""
        if self.safeguard_method != 'correspondence':
            # :235.  The reference's other branch, 'fcgf_feature_matching' (:31-46), calls the pre-0.10
            # `o3d.registration` namespace, which does not exist in the pinned open3d==0.17.0: dead code there.
            raise ValueError('Undefined')
        idx0 = torch.as_tensor(idx0, device=self.device).long()
        X = pcd0 if len(idx0) == len(pcd0) and bool((idx0 == torch.arange(len(idx0), device=self.device)).all()) \
            else ops.gather_rows3(pcd0, idx0)
        Y = ops.gather_rows3(pcd1, torch.as_tensor(idx1, device=self.device).long())
        T, h, count, rmse = ops.ransac_correspondence(X, Y, distance_threshold, self.ransac_max_iteration,
                                                      seed=self.ransac_seed)
        self.last_stats = {'ransac_hypothesis': h, 'ransac_inliers': count, 'ransac_rmse': rmse}
        return T

    # ---- extension points of register(): identities here.  The test harness (tests/helpers.py::HarnessDGR) overrides
    #      them to replace matches / logits AFTER the search / the inlier net ran (untrained synthetic weights give
    #      meaningless matches and confidences); nothing in the product does.
    def _post_matching(self, xyz0, xyz1, corres_idx1):
        return corres_idx1

    def _post_inlier_prediction(self, xyz0, xyz1, corres_idx1, logit):
        return logit

    # ---- main entry ------------------------------------------------------------------------------
    def register(self, xyz0, xyz1, inlier_thr=0.00):
        """Main algorithm (:238-324).  Returns a 4x4 float64 numpy transformation."""
        self.reg_timer.tic()
        xyz0, coords0, feats0 = self.preprocess(xyz0)
        xyz1, coords1, feats1 = self.preprocess(xyz1)

        self.feat_timer.tic()
        fcgf_feats0 = self.fcgf_feature_extraction(feats0, coords0)
        fcgf_feats1 = self.fcgf_feature_extraction(feats1, coords1)
        self.feat_timer.toc()

        corres_idx0, corres_idx1 = self.fcgf_feature_matching(fcgf_feats0, fcgf_feats1)
        corres_idx1 = self._post_matching(xyz0, xyz1, corres_idx1)
        self.last_corres_idx1 = corres_idx1 if self.keep_intermediates else None

        inlier_coords, inlier_feats = ops.inlier_inputs(coords0, xyz0, coords1, xyz1, corres_idx1,
                                                        self.inlier_feature_type)
        logit = self.inlier_prediction(inlier_feats.contiguous(), coords=inlier_coords)
        logit = self._post_inlier_prediction(xyz0, xyz1, corres_idx1, logit)
        self.last_logit = logit if self.keep_intermediates else None
        weights, wsum = ops.sigmoid_clip_sum(logit, self.clip_weight_thresh)

        wsum_threshold = max(200, len(weights) * 0.05)
        self.last_wsum = (float(wsum), float(wsum_threshold))     # host values the gate needs anyway; the reference prints them (:279-281)
        T = np.identity(4)
        safeguard = wsum < wsum_threshold
        if not safeguard:
            try:
                rot, trans, opt_output = GlobalRegistration(xyz0, ops.gather_rows3(xyz1, corres_idx1),
                                                            weights=weights, break_threshold_ratio=1e-4,
                                                            quantization_size=2 * self.voxel_size,
                                                            verbose=False)
                T[0:3, 0:3] = rot.detach().cpu().numpy()
                T[0:3, 3] = trans.detach().cpu().numpy()
                self.last_status, self.last_stats = 'ok', opt_output
            except _lib.DgrError as e:
                # reference (:295-300): `except RuntimeError` around the SVD, "Will directly go to Safeguard" -- there
                # T simply stays the identity (the SVD branch never reaches the `else` below).  Only the SVD failure
                # is that case here: a workspace or HIP error is an infrastructure failure and must not be counted
                # as a registration failure.
                if e.code != _lib.DGR_ESVD:
                    raise
                self.last_status = 'svd_failed'
        else:
            # Case 1 (:302-315): safeguard RANSAC on the putative correspondences
            T = self.safeguard_registration(xyz0, xyz1, corres_idx0, corres_idx1, feats0, feats1,
                                            2 * self.voxel_size, num_iterations=80000)
            self.last_status = 'safeguard'
        self.reg_timer.toc()
        if self.use_icp:                       # :317-322
            T, fitness, rmse, iters = ops.icp_point_to_point(xyz0, xyz1, self.voxel_size * 2, init=T)
            self.last_icp = {'fitness': fitness, 'inlier_rmse': rmse, 'iterations': iters}
        return T

    # ---- batched throughput path (no reference counterpart) ---------------
    def register_batch(self, pairs, forced_logits=None, skip_refinement=False, safeguard=False, icp=False):
        """Registers a list of (xyz0, xyz1) pairs with ONE sparse tensor per network (pairs are
        distinguished by the batch column, the layout of ME.utils.batched_coordinates).  Returns
        T [n,4,4] float64, status [n] (0 ok / 1 low confidence / 2 SVD failed), stats [n,4]."""
        x0, c0, x1, c1, off0, off1 = [], [], [], [], [0], [0]
        for p, (a, b) in enumerate(pairs):
            xa, ca, _ = self.preprocess(a, batch_index=p)
            xb, cb, _ = self.preprocess(b, batch_index=p)
            x0.append(xa); c0.append(ca); x1.append(xb); c1.append(cb)
            off0.append(off0[-1] + len(xa)); off1.append(off1[-1] + len(xb))
        return self.register_voxelized(torch.cat(c0), torch.cat(x0), off0, torch.cat(c1), torch.cat(x1), off1,
                                       forced_logits=forced_logits, skip_refinement=skip_refinement,
                                       safeguard=safeguard, icp=icp)

    def _collated(self, input_dict):
        """(coords0, xyz0, off0, coords1, xyz1, off1) of a collated batch on the device, checked against `len_batch`."""
        len_batch = [(int(a), int(b)) for a, b in input_dict['len_batch']]
        off0, off1 = [0], [0]
        for n0, n1 in len_batch:
            off0.append(off0[-1] + n0)
            off1.append(off1[-1] + n1)
        c0 = torch.as_tensor(input_dict['sinput0_C']).to(self.device).int()
        c1 = torch.as_tensor(input_dict['sinput1_C']).to(self.device).int()
        x0 = torch.cat([torch.as_tensor(np.asarray(x)).float() for x in input_dict['pcd0']]).to(self.device)
        x1 = torch.cat([torch.as_tensor(np.asarray(x)).float() for x in input_dict['pcd1']]).to(self.device)
        if len(c0) != off0[-1] or len(c1) != off1[-1] or len(x0) != off0[-1] or len(x1) != off1[-1]:
            raise ValueError('len_batch does not match the concatenated coordinates / points')
        for p in range(len(len_batch)):   # the batch column must be the pair index of the row block
            if off0[p + 1] > off0[p] and (int(c0[off0[p], 0]) != p or int(c0[off0[p + 1] - 1, 0]) != p):
                raise ValueError('sinput0_C is not in batched_coordinates order')
        return c0, x0, off0, c1, x1, off1

    def register_collated(self, input_dict, **kw):
        """Registers every pair of a collated batch in the reference's data-loader layout
        (`CollationFunctionFactory.collate_pair_fn`, dataloader/base_loader.py:40-98): `sinput0_C` /
        `sinput1_C` int [N,4] batched coordinates (batch column first, `ME.utils.batched_coordinates`),
        `pcd0` / `pcd1` sequences of per-pair xyz [Ni,3] aligned with those rows, `len_batch` [[N0,N1],...].
        Returns T [n,4,4] float64, status [n], stats [n,4]."""
        return self.register_voxelized(*self._collated(input_dict), **kw)

    def register_voxelized(self, coords0, xyz0, off0, coords1, xyz1, off1, forced_logits=None,
                           skip_refinement=False, override_idx1=None, safeguard=False, icp=False):
        """Fused batched path (one `dgr_register_batch`).  With `safeguard`, pairs that fail the confidence
        gate (status 1) are re-estimated by the RANSAC safeguard over their putative correspondences and get
        status 3 -- like `register()` and the reference, a pair whose SVD failed (status 2) keeps T = identity
        (:295-300 never reaches the safeguard branch); with `icp`, every pair is finally refined by
        point-to-point ICP -- the two Open3D steps of `register()` (:302-322), both inside the same library call
        (dgr_params.safeguard / use_icp)."""
        T, status, stats = ops.register_batch(
            self.fcgf_model._handle(), self.inlier_model._handle(), coords0, xyz0, off0, coords1, xyz1, off1,
            self.voxel_size, clip_weight_thresh=self.clip_weight_thresh,
            inlier_feature_type=self.inlier_feature_type, break_threshold_ratio=1e-4,
            skip_refinement=skip_refinement, forced_logit=forced_logits, override_idx1=override_idx1,
            safeguard=safeguard, use_icp=icp, ransac_hypotheses=self.ransac_max_iteration,
            ransac_seed=self.ransac_seed)
        T = T.astype(np.float64)   # (already float64 when the safeguard / ICP stages ran: their results at full width)
        return T, status, stats

    # ---- a scene: every fragment featurised once, any list of pairs registered from that (no reference counterpart) --
    def extract_fragments(self, clouds, chunk_rows=300_000):
        """Voxelises every cloud and runs the FCGF net over them in chunks: `FragmentBank` with fragment i = clouds[i].
        Each cloud is `preprocess`ed with its position in the chunk as the batch index and a chunk goes through
        `fcgf_model` as ONE sparse tensor of ones; a chunk closes before the cloud that would push it past `chunk_rows`
        voxels (a cloud larger than that is a chunk of its own).  The default is about the row count of the timed 6-pair
        batch (12 fragments); it has not been tuned.  The bank's batch column is 0 whatever the chunking.
        `feat_timer` covers the call."""
        from .fragment_bank import FragmentBank
        clouds = list(clouds)
        if not clouds:
            raise ValueError('no clouds')
        self.feat_timer.tic()
        xyz, coords, feats, off = [], [], [], [0]
        chunk = []          # coords of the open chunk, batch column = position in the chunk

        def close():
            if chunk:
                c = torch.cat(chunk)
                feats.append(self.fcgf_feature_extraction(torch.ones(len(c), 1, device=self.device), c))
                chunk.clear()
        for cloud in clouds:
            x, c, _ = self.preprocess(cloud, batch_index=len(chunk))
            if len(x) == 0:
                raise ValueError(f'cloud {len(xyz)} has no points')
            if chunk and sum(len(k) for k in chunk) + len(c) > chunk_rows:
                close()
                c[:, 0] = 0     # first of the next chunk
            chunk.append(c)
            coords.append(c)
            xyz.append(x)
            off.append(off[-1] + len(x))
        close()
        bank_coords = torch.cat(coords)
        bank_coords[:, 0] = 0
        self.feat_timer.toc()
        return FragmentBank.from_tensors(bank_coords, torch.cat(xyz), torch.cat(feats), np.asarray(off, np.int64))

    def _check_bank_device(self, bank):
        bd = torch.device(bank.device)    # ('cuda' without an index is the current device: not told apart here)
        if bd.type != self.device.type or (None not in (bd.index, self.device.index) and bd.index != self.device.index):
            raise ValueError(f'the bank is on {bank.device}, this object on {self.device}')

    def _scored_pairs_args(self, bank, pairs, T, radius):
        """What `score_pairs` and `optimize_scene` open with: the bank's device, the pair ids and the poses checked as in
        `register_pairs` / `ops.check_score_args`.  Returns (ids int32 [n,2], T float64 [n,4,4] with the last row set to
        (0, 0, 0, 1), radius: 2 voxels when None)."""
        from .fragment_bank import pair_groups
        self._check_bank_device(bank)
        ids = np.concatenate([g for _, g in pair_groups(bank, pairs, 1)])
        radius = 2 * self.voxel_size if radius is None else radius
        _, _, T, radius = ops.check_score_args(len(bank.xyz), bank.off, ids, T, radius)
        T = T.reshape(len(ids), 4, 4).copy()
        T[:, 3] = (0, 0, 0, 1)                    # (the library ignores the last row; an inverse must not see it)
        return ids, T, radius

    def register_pairs(self, bank, pairs, batch_pairs=6, safeguard=False, icp=False, skip_refinement=False,
                       forced_logits=None, override_idx1=None):
        """Registers `pairs` ([n,2] integers: fragment i of `bank` onto fragment j) through the fused path
        (`dgr_register_pairs`), `batch_pairs` consecutive pairs per library call, without voxelising or featurising
        anything again.  Returns what `register_voxelized` returns, in the order of `pairs`; `safeguard` / `icp` /
        `skip_refinement` as there.  A fragment may occur in any number of pairs, on either side.
        The two harness hooks are lists with one entry per PAIR: forced_logits[k] one value per row of pair k's
        fragment 0, override_idx1[k] rows of pair k's fragment 1 (-1 = keep the match)."""
        from .fragment_bank import group_hooks, pair_groups
        self._check_bank_device(bank)
        if bank.n_out != self.fcgf_model.out_channels:
            raise ValueError(f'the bank holds {bank.n_out}-wide features, the FCGF model writes '
                             f'{self.fcgf_model.out_channels}')
        groups = pair_groups(bank, pairs, batch_pairs)
        for name, seq in (('forced_logits', forced_logits), ('override_idx1', override_idx1)):
            if seq is not None and len(seq) != sum(len(ids) for _, ids in groups):
                raise ValueError(f'{name} must have one entry per pair')
        out = []
        for first, ids in groups:
            fl, ov = group_hooks(bank, first, ids, forced_logits, override_idx1, self.device)
            out.append(ops.register_pairs(
                self.inlier_model._handle(), bank.coords, bank.xyz, bank.F, bank.off, ids, self.voxel_size,
                clip_weight_thresh=self.clip_weight_thresh, inlier_feature_type=self.inlier_feature_type,
                break_threshold_ratio=1e-4, skip_refinement=skip_refinement, forced_logit=fl, override_idx1=ov,
                safeguard=safeguard, use_icp=icp, ransac_hypotheses=self.ransac_max_iteration,
                ransac_seed=self.ransac_seed))
        T, status, stats = (np.concatenate([o[k] for o in out]) for k in range(3))
        return T.astype(np.float64), status, stats

    def score_pairs(self, bank, pairs, T, radius=None):
        """The geometric fit of `pairs` ([n,2] integers: fragment i of `bank` onto fragment j) under the poses `T`
        [n,4,4] (i into j's frame, e.g. what `register_pairs` returned): pair k is scored as (i, j) under T[k] and as
        (j, i) under inv(T[k]) in ONE library call of 2n directed pairs (`dgr_score_pairs`).  `radius` defaults to 2
        voxels, the distance the reference gives its ICP (:317-322).  Returns a dict of per-pair arrays: `n_corr`,
        `fitness` (rows of i with a row of j strictly within the radius, over the rows of i), `inlier_rmse`,
        `information` [n,6,6] (Open3D's order: rotation, translation; `core.pair_score`), `fitness_reverse` (the same
        share of j's rows) and `overlap` = max(fitness, fitness_reverse) -- the reference's `compute_overlap_ratio`
        (util/pointcloud.py:72-80) at that radius.  Only the bank's `xyz` is read: neither network runs and the feature
        width does not matter.  The bank's device and the pair ids are checked as in `register_pairs`."""
        from .pair_score import scores_from_sums
        ids, T, radius = self._scored_pairs_args(bank, pairs, T, radius)
        n = len(ids)
        try:
            T_inv = np.linalg.inv(T)
        except np.linalg.LinAlgError as e:
            raise ValueError(f'a pose cannot be inverted: {e}') from None
        if not np.isfinite(T_inv).all():
            raise ValueError('a pose cannot be inverted')
        sums = ops.score_pairs(bank.xyz, bank.off, np.concatenate((ids, ids[:, ::-1])), np.concatenate((T, T_inv)), radius)
        rows = np.diff(bank.off)
        out = scores_from_sums(sums[:n], rows[ids[:, 0]])
        out['fitness_reverse'] = scores_from_sums(sums[n:], rows[ids[:, 1]])['fitness']
        out['overlap'] = np.maximum(out['fitness'], out['fitness_reverse'])
        return out

    def optimize_scene(self, bank, pairs, T, scores=None, uncertain=None, radius=None, reference_node=0,
                       preference_loop_closure=1.0, edge_prune_threshold=0.25, pose_init=None, max_iter=100, rel_tol=1e-13):
        """One pose per fragment of `bank` in the frame of fragment `reference_node`, from `pairs` ([m,2]: fragment i onto
        fragment j) and their poses `T` [m,4,4] (what `register_pairs` returned): robust pose-graph optimisation with line
        processes (`ops.pose_graph_optimize`, csrc/posegraph.hip; `core.pose_graph` states the objective), in the two
        passes of Open3D's `global_optimization`.
          * `scores`: what `score_pairs(bank, pairs, T, radius)` returns (computed here when None); its `information` are
            the edge weights.  Pairs without a correspondence (`n_corr` = 0) are dropped.
          * `uncertain` [m] bool: the loop closures, subject to a line process; default |i - j| != 1 (consecutive
            fragments are odometry, as in Open3D's reconstruction pipeline).  All-True is allowed.
          * mu = preference_loop_closure * radius^2 * mean n_corr (`core.pose_graph.default_mu`); `radius` defaults to
            2 voxels, the radius `score_pairs` defaults to.
          * start: the maximum spanning tree by n_corr, certain edges first, unless `pose_init` [n,4,4] is given.
          * pass 1 over the fragments connected to the reference node; uncertain edges with l < `edge_prune_threshold`
            are pruned; pass 2 over the kept edges from pass 1's poses (skipped when nothing was pruned: it would repeat
            pass 1).  Fragments that the kept edges do not connect to the reference node are left out of pass 2 and keep
            their pass-1 pose (their start when never connected).  A pass takes at most 128 connected fragments.
        Returns a dict: `poses` [n,4,4] (fragment -> the reference fragment's frame times pose_init[reference_node]),
        `line_process` [m] (pass 2's, pass 1's for the edges pruned there, NaN for edges that took no part), `kept` [m]
        bool, `reachable` [n] bool, `objective_initial` / `objective_final` (F* at the start of pass 1 / the end of
        pass 2), `iterations` and `converged` (both passes), `mu`."""
        from . import pose_graph as pgm
        ids, T, radius = self._scored_pairs_args(bank, pairs, T, radius)
        ids = ids.astype(np.int64)
        m, n = len(ids), len(bank)
        if not 0 <= reference_node < n:
            raise ValueError(f'reference node {reference_node} outside [0, {n})')
        if not (edge_prune_threshold >= 0 and edge_prune_threshold <= 1):
            raise ValueError('edge_prune_threshold must lie in [0, 1]')
        if bool((ids[:, 0] == ids[:, 1]).any()):
            raise ValueError('a pair joins a fragment to itself')
        unc = np.abs(ids[:, 0] - ids[:, 1]) != 1 if uncertain is None else np.asarray(uncertain, bool).reshape(-1)
        if unc.shape != (m,):
            raise ValueError('one uncertain flag per pair expected')
        if pose_init is not None:
            pose_init = np.array(pose_init, np.float64)
            if pose_init.shape != (n, 4, 4) or not np.isfinite(pose_init).all():
                raise ValueError(f'pose_init must be [{n},4,4] and finite')
        if scores is None:
            scores = self.score_pairs(bank, ids, T, radius)
        info = np.asarray(scores['information'], np.float64)
        if info.shape != (m, 6, 6) or not np.isfinite(info).all():
            raise ValueError(f'scores["information"] must be [{m},6,6] and finite')
        used = info[:, 3, 3] > 0
        if not used.any():
            raise ValueError('no pair has a correspondence')
        mu = pgm.default_mu(info[used], radius, preference_loop_closure)
        if pose_init is None:
            poses, _ = pgm.spanning_tree_poses(n, ids[used], T[used], info[used, 3, 3], reference_node, unc[used])
        else:
            poses = pose_init
        line = np.full(m, np.nan)
        kept = used.copy()
        out = {'mu': mu, 'iterations': 0, 'converged': True, 'objective_initial': None, 'objective_final': None}
        for pass_no in range(2):
            reach = pgm.reachable_nodes(n, ids, kept, reference_node)
            sel = kept & reach[ids[:, 0]]           # (an edge has both ends in one component)
            if not sel.any():
                break
            local = np.cumsum(reach) - 1            # node ids of the reachable sub-graph
            sub = np.nonzero(reach)[0]
            P, l, stats = ops.pose_graph_optimize([0, len(sub)], [0, int(sel.sum())], local[ids[sel]], T[sel], info[sel],
                                                  unc[sel], poses[sub], [(mu, int(local[reference_node]), max_iter, rel_tol)],
                                                  device=self.device)
            poses = poses.copy()
            poses[sub] = P
            line[sel] = l
            if out['objective_initial'] is None:
                out['objective_initial'] = float(stats[0, 0])
            out['objective_final'] = float(stats[0, 1])
            out['iterations'] += int(stats[0, 2])
            out['converged'] = out['converged'] and bool(stats[0, 3])
            if pass_no == 0:                        # prune once, between the passes
                pruned = sel & unc & (line < edge_prune_threshold)
                if not pruned.any():
                    break                           # nothing to drop: pass 2 would repeat pass 1
                kept = kept & ~pruned
        out.update(poses=poses, line_process=line, kept=kept, reachable=pgm.reachable_nodes(n, ids, kept, reference_node))
        return out

    def fuse_scene(self, bank, poses, voxel_size=None, fragments=None, min_points=1, clouds=None):
        """The scene of `bank` under `poses` [n,4,4] (fragment -> common frame: `optimize_scene(...)['poses']`): the points of
        the selected fragments, each under its pose, averaged per voxel of one lattice with origin 0 (`ops.voxel_mean`,
        csrc/voxelmean.hip).  `fragments`: a bool mask over the bank or a list of distinct fragment ids, e.g.
        `res['reachable']` (default: all); `voxel_size` defaults to this object's.  `clouds` (one [N_k,3] float32 / float64
        array or tensor per fragment of the bank) are fused instead of the bank's voxelised `xyz`: the raw points of the
        fragments.  Voxels with fewer than `min_points` points are removed.  Returns a dict of device tensors, voxels in the
        order of their first point: `xyz` float64 [V,3], `count` int32 [V], `first_fragment` int64 [V] (the fragment that
        voxel's first point belongs to), and `dropped` (int): points that are not finite or leave the int32 lattice.
        Neither network runs.  The bank's device and the fragment ids are checked as in `score_pairs`."""
        self._check_bank_device(bank)
        n = len(bank)
        poses = _args.host(poses)
        if poses.shape != (n, 4, 4):
            raise ValueError(f'poses must be [{n},4,4], got {poses.shape}')
        min_points = _args.integer(min_points, 'min_points', lambda v: v >= 1, 'an integer >= 1')
        voxel_size = self.voxel_size if voxel_size is None else voxel_size
        if clouds is None:
            parts, off, rows = None, bank.off, len(bank.xyz)
        else:
            if len(clouds) != n:
                raise ValueError(f'one cloud per fragment of the bank expected: {len(clouds)} for {n}')
            parts = [c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c)) for c in clouds]
            for k, c in enumerate(parts):
                if c.dim() != 2 or c.shape[1] != 3 or len(c) == 0 or c.dtype not in (torch.float32, torch.float64):
                    raise ValueError(f'cloud {k} must be a non-empty float32 / float64 [N,3] array, got {c.dtype} {tuple(c.shape)}')
            off = np.cumsum([0] + [len(c) for c in parts]).astype(np.int64)
            rows = int(off[-1])
        off, ids, _, _, voxel_size, _ = ops.check_voxel_mean_rows(rows, voxel_size, off, np.arange(n) if fragments is None else fragments)
        T = np.ascontiguousarray(poses[ids], np.float64)
        if not np.isfinite(T[:, :3]).all():
            raise ValueError('poses must be finite (first three rows)')
        if parts is None:
            xyz = bank.xyz
        else:   # (one float64 cloud makes the fused array float64: every cloud widens exactly)
            wide = torch.float64 if any(c.dtype == torch.float64 for c in parts) else torch.float32
            xyz = torch.cat([c.to(self.device, wide) for c in parts])
        res = ops.voxel_mean(xyz, voxel_size, off, ids, T)
        out = {'xyz': res['xyz'], 'count': res['count'], 'dropped': res['dropped'],
               'first_fragment': torch.bucketize(res['first'], torch.from_numpy(off[1:]).to(res['first'].device), right=True)}
        if min_points > 1:
            keep = out['count'] >= int(min_points)
            out.update({k: out[k][keep] for k in ('xyz', 'count', 'first_fragment')})
        return out

    # ---- measurement beside the registration path (core/trainer.py:353-489, `_valid_epoch`) ----------------------
    def validate_collated(self, input_dict, matching_radius=None, success_rte_thresh=0.3, success_rre_thresh=15.0, **kw):
        """The validation statistics of the reference's trainer for one collated batch (layout of `register_collated`) that
        also carries `T_gt` [n,4,4]: how good the feature matches and the inlier weights are against the ground-truth
        pose.  Read-only beside registration: the batch goes through `register_voxelized(..., skip_refinement=True, **kw)`
        (the harness hooks `forced_logits` / `override_idx1` pass through), then
          * positive pairs: `input_dict['correspondences']` (one [P,2] array per pair) when present, otherwise every
            (i, j) within `matching_radius` (default 2 voxels) under T_gt (ops.radius_pairs_batch);
          * a match (i, idx1[i]) is correct when it is a positive pair (ops.pairs_isin, seed max(N0, N1));
          * (n, hits, tp, fp, tn, fn) per pair at weight > 0.5 (ops.validation_counts);
          * the weighted-Procrustes pose of every pair whatever the confidence gate said (`_valid_epoch` does not gate),
            `valid = wsum > 10` (:417), success = RTE and RRE below the thresholds and valid.
        Returns a dict with the reference's keys (hit_ratio, precision, recall, f1, tpr, tnr, balanced_accuracy with its
        eps; regist_rte, regist_rre, succ_rate: means over the pairs) and the per-pair arrays `counts` [n,6], `rte`, `rre`,
        `success`, `valid`, `wsum`, `T_pred` [n,4,4], `num_pos_pairs`."""
        from ..eval.metrics import batch_rte_rre, validation_statistics
        c0, x0, off0, c1, x1, off1 = self._collated(input_dict)
        n = len(off0) - 1
        T_gt = input_dict['T_gt']
        T_gt = _args.host(T_gt).astype(np.float64)
        if T_gt.shape != (n, 4, 4):
            raise ValueError(f'T_gt must be [{n},4,4], got {T_gt.shape}')
        radius = 2 * self.voxel_size if matching_radius is None else matching_radius
        if input_dict.get('correspondences') is None:
            ops.check_radius_args(radius, None, T_gt, n)          # fail before the networks run
        kw = dict(kw, skip_refinement=True)
        _, _, stats = self.register_voxelized(c0, x0, off0, c1, x1, off1, **kw)
        idx1 = ops.batch_output(self.device, 'idx1')              # rows of the concatenated fragment 1
        weights = ops.batch_output(self.device, 'weights')
        o0, o1 = np.asarray(off0, np.int64), np.asarray(off1, np.int64)
        seg = torch.repeat_interleave(torch.arange(n, device=self.device), torch.from_numpy(np.diff(o0)).to(self.device))
        rows = torch.arange(len(idx1), device=self.device)
        pred = torch.stack((rows - torch.from_numpy(o0).to(self.device)[seg],
                            idx1 - torch.from_numpy(o1).to(self.device)[seg]), 1)     # pair-local (i, j), trainer.find_pairs
        if input_dict.get('correspondences') is not None:
            parts = [torch.as_tensor(np.asarray(p) if not torch.is_tensor(p) else p).reshape(-1, 2).to(self.device, torch.int64)
                     for p in input_dict['correspondences']]
            if len(parts) != n:
                raise ValueError('one correspondence array per pair expected')
            pos, pos_off = torch.cat(parts), np.cumsum([0] + [len(p) for p in parts])
        else:
            pos, pos_off = ops.radius_pairs_batch(x0, o0, x1, o1, T_gt, radius)
        seeds = [max(int(o0[p + 1] - o0[p]), int(o1[p + 1] - o1[p])) for p in range(n)]
        label = ops.pairs_isin(pos, pos_off, pred, o0, seeds)
        counts = ops.validation_counts(label, weights, o0, 0.5)
        T_pred = np.tile(np.eye(4), (n, 1, 1))
        solved = np.ones(n, bool)
        for p in range(n):
            a, b = int(o0[p]), int(o0[p + 1])
            try:
                R, t = ops.weighted_procrustes(x0[a:b], ops.gather_rows3(x1, idx1[a:b]), weights[a:b])
                T_pred[p, :3, :3], T_pred[p, :3, 3] = R, t
            except _lib.DgrError as e:      # non-finite input / SVD failure: no pose for this pair
                if e.code != _lib.DGR_ESVD:
                    raise
                solved[p] = False
        wsum = np.asarray(stats[:, 3], np.float64)
        valid = (wsum > 10) & solved
        rte, rre = batch_rte_rre(T_pred[:, :3, :3], T_pred[:, :3, 3], T_gt)
        success = (rte < success_rte_thresh) & (rre < success_rre_thresh) & valid
        out = validation_statistics(counts)
        out.update(regist_rte=float(rte.mean()), regist_rre=float(rre.mean()), succ_rate=float(success.mean()),
                   counts=counts, rte=rte, rre=rre, success=success, valid=valid, wsum=wsum, T_pred=T_pred,
                   num_pos_pairs=np.diff(pos_off))
        return out
