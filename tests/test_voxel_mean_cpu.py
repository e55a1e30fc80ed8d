"""CPU-side checks of the averaging voxel down-sample (csrc/voxelmean.hip, `ops.voxel_mean`, `voxel_down_sample`,
`fuse_scene`): the C entry point exists, links from C and refuses bad arguments before any device work; the Python wrappers
refuse them before any device state exists; the numpy statement the GPU tests compare against (tests/voxel_mean_ref.py)
gets hand-computed cases right; `compute_overlap_ratio` keeps its default."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from voxel_mean_ref import FRAC_BITS, transformed_f64, voxel_mean_ref

ONE = 1 << FRAC_BITS


def _build_if_missing():
    from deepglobalregistration_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_library_exports_the_entry_point():
    from deepglobalregistration_amd import _lib, ops
    _build_if_missing()
    lib = _lib.load()
    assert 'dgr_voxel_mean' in _lib.SIGNATURES
    assert hasattr(lib, 'dgr_voxel_mean')
    with open(os.path.join(ROOT, 'include', 'dgr_hip.h')) as f:
        assert f'#define DGR_VM_FRAC_BITS {ops.VM_FRAC_BITS}\n' in f.read()
    assert ops.VM_FRAC_BITS == FRAC_BITS == 40


def test_entry_point_links_from_c_and_checks_arguments(tmp_path):
    """A C99 program links dgr_voxel_mean and gets DGR_EINVAL for every bad argument the header lists -- reported before
    any device work, so the program needs no GPU (the context is a dummy non-NULL pointer)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    _build_if_missing()
    lib_dir = os.path.join(ROOT, 'deepglobalregistration_amd', 'lib')
    src = tmp_path / 'vm_abi.c'
    src.write_text(r'''
#include <stdio.h>
#include <math.h>
#include "dgr_hip.h"
#define CALL(ctx, xyz, off, nfrag, ids, nsel, T, org, vox, first, coords, count, mean, n, dropped) \
  dgr_voxel_mean(ctx, xyz, 0, off, nfrag, ids, nsel, T, org, vox, first, coords, count, 0, mean, n, dropped, 0)
#define BAD(...) bad += CALL(__VA_ARGS__) != DGR_EINVAL
int main(void) {
  /* a context is only dereferenced behind the argument checks: any non-NULL pointer will do here */
  int dummy = 0; dgr_ctx *ctx = (dgr_ctx *)&dummy;
  void *dev = (void *)&dummy;   /* device pointers in real use: never dereferenced on the host */
  int64_t *first = (int64_t *)dev; int32_t *coords = (int32_t *)dev, *count = (int32_t *)dev; double *mean = (double *)dev;
  int64_t off[3] = {0, 4, 9}, off_neg[3] = {-1, 4, 9}, off_empty[3] = {0, 4, 4}, off_desc[3] = {0, 4, 2};
  int64_t off_huge[3] = {0, 1, 2147483649ll};   /* 2^31 rows in fragment 1 */
  int32_t ids[2] = {1, 0}, ids_hi[2] = {0, 2}, ids_neg[2] = {-1, 0}, ids_rep[2] = {1, 1};
  double T[32] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1,  1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1}, Tnan[32], Tinf[32], Tlast[32];
  double org[3] = {0, 0, 0}, org_nan[3] = {0, NAN, 0}, org_inf[3] = {0, 0, -INFINITY};
  int64_t n = 0, dropped = 0;
  int bad = 0, i;
  for (i = 0; i < 32; ++i) Tnan[i] = Tinf[i] = Tlast[i] = T[i];
  Tnan[16 + 3] = NAN; Tinf[5] = INFINITY; Tlast[12] = NAN;
  if (DGR_VM_FRAC_BITS != 40) bad += 1;
  BAD(0, dev, off, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, 0, off, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, 0, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, 0, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, 0, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, first, 0, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, first, coords, 0, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, first, coords, count, 0, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, first, coords, count, mean, 0, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, 0);
  BAD(ctx, dev, off, 0, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, -1, 0, -1, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 0, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, -2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, 0, 1, T, org, 0.05, first, coords, count, mean, &n, &dropped);   /* all fragments: nsel = nfrag */
  BAD(ctx, dev, off_neg, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off_empty, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off_desc, 2, ids, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids_hi, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids_neg, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids_rep, 2, T, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, Tnan, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, Tinf, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org_nan, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org_inf, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, 0.0, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, -0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, NAN, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off, 2, ids, 2, T, org, INFINITY, first, coords, count, mean, &n, &dropped);
  /* frag_ids, T and fsum_out may be NULL and the last row of a pose is ignored: these calls WOULD reach the device, so
     they are made with 2^31 selected rows: the only error left is that count, reported last */
  BAD(ctx, dev, off_huge, 2, 0, 2, 0, org, 0.05, first, coords, count, mean, &n, &dropped);
  BAD(ctx, dev, off_huge, 2, ids, 2, Tlast, org, 0.05, first, coords, count, mean, &n, &dropped);
  printf("%d %s\n", bad, dgr_last_error());
  return bad;
}
''')
    exe = tmp_path / 'vm_abi'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    str(src), '-o', str(exe), '-L', lib_dir, '-ldgr_hip', f'-Wl,-rpath,{lib_dir}',
                    '-Wl,-rpath,/opt/rocm/lib', '-lm'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert '2^31 or more selected rows' in out.stdout     # the last call got past every other check


def test_wrappers_reject_bad_arguments_before_any_device_state(monkeypatch):
    from deepglobalregistration_amd import _lib, ops
    from deepglobalregistration_amd.core.deep_global_registration import DeepGlobalRegistration
    from deepglobalregistration_amd.core.fragment_bank import FragmentBank
    from deepglobalregistration_amd.util.pointcloud import compute_overlap_ratio, voxel_down_sample

    def no_device(*a, **k):
        raise AssertionError('device state touched before the argument check')
    monkeypatch.setattr(_lib, 'load', no_device)
    monkeypatch.setattr(ops, 'get_ctx', no_device)
    monkeypatch.setattr(ops, '_xyz_dev', no_device)
    monkeypatch.setattr(ops, '_xyz_any_dev', no_device)
    monkeypatch.setattr(ops, 'voxelize', no_device)
    x = np.zeros((9, 3), np.float32)
    off, T2 = [0, 4, 9], np.tile(np.eye(4), (2, 1, 1))
    for voxel in (0.0, -0.1, float('nan'), float('inf'), '0.1', None, True):
        with pytest.raises(ValueError, match='voxel_size'):
            ops.voxel_mean(x, voxel)
        with pytest.raises(ValueError, match='voxel_size'):
            voxel_down_sample(x, voxel)
    for bad_x in (np.zeros((9, 2), np.float32), np.zeros(9, np.float32), np.zeros((2, 9, 3), np.float32)):
        with pytest.raises(ValueError, match=r'\[N,3\]'):
            ops.voxel_mean(bad_x, 0.1)
    for bad_x in (np.zeros((9, 3), np.int32), np.zeros((9, 3), np.float16), torch.zeros(9, 3, dtype=torch.int64), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError, match='xyz must be'):
            ops.voxel_mean(bad_x, 0.1)
    with pytest.raises(ValueError, match='empty'):
        ops.voxel_mean(np.zeros((0, 3), np.float32), 0.1)
    for bad_off in ([0, 4, 8], [0, 4, 4, 9], [0, 5, 4, 9], [-1, 4, 9], [9], [0.0, 9.0], [[0, 9]]):
        with pytest.raises(ValueError, match='off must'):
            ops.voxel_mean(x, 0.1, bad_off)
    for bad_ids, what in (([0, 2], 'outside'), ([-1], 'outside'), ([1, 1], 'repeated'), ([], 'empty'), ([[0, 1]], '1-D'),
                          ([0.0], '1-D'), ([True, False, True], 'mask'), ([False, False], 'empty')):
        with pytest.raises(ValueError, match=what):
            ops.voxel_mean(x, 0.1, off, bad_ids)
    for bad_T in (np.eye(4), np.zeros((3, 4, 4)), np.zeros((2, 16)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match='T must'):
            ops.voxel_mean(x, 0.1, off, None, bad_T)
    for where in ((0, 0, 3), (1, 2, 2)):
        Tn = T2.copy()
        Tn[where] = np.nan if where[0] else np.inf
        with pytest.raises(ValueError, match='finite'):
            ops.voxel_mean(x, 0.1, off, [1, 0], Tn)
    Tl = T2.copy()
    Tl[1, 3, 0] = np.nan                         # the last row is ignored: the check passes
    o, ids, T, org, voxel, rows = ops.check_voxel_mean_args(x, 0.1, off, [True, True], Tl)
    assert T.shape == (2, 16) and ids.tolist() == [0, 1] and ids.dtype == np.int32 and org.tolist() == [0, 0, 0] and rows == 9
    assert ops.check_voxel_mean_args(x, 0.1, off, [1])[5] == 5 and ops.check_voxel_mean_args(x, 0.1)[0].tolist() == [0, 9]
    assert ops.check_voxel_mean_args(x, 0.1, off, [1], np.eye(4))[2].shape == (1, 16)
    for bad_origin in ([0, 0], [0, np.nan, 0], [np.inf, 0, 0], 'abc', [[0, 0, 0]]):
        with pytest.raises(ValueError, match='origin'):
            ops.voxel_mean(x, 0.1, origin=bad_origin)
        with pytest.raises(ValueError, match='origin'):
            voxel_down_sample(x, 0.1, origin=bad_origin)
    with pytest.raises(ValueError, match='2\\^31'):
        ops.check_voxel_mean_rows(2 ** 31, 0.1)
    with pytest.raises(ValueError, match='radius'):
        compute_overlap_ratio(x, x, np.eye(4), 0.0, downsample='mean')
    # the method: the bank's device, the poses and the fragment list, before the library is asked for anything
    bank = FragmentBank.from_tensors(torch.zeros(9, 4, dtype=torch.int32), torch.zeros(9, 3), torch.zeros(9, 16), off)
    dgr = DeepGlobalRegistration.__new__(DeepGlobalRegistration)    # (no networks are needed to refuse an argument)
    dgr.device, dgr.voxel_size = torch.device('cuda'), 0.05
    with pytest.raises(ValueError, match='the bank is on'):
        dgr.fuse_scene(bank, T2)
    dgr.device = torch.device('cpu')             # (a device the bank is on: the remaining checks are reached)
    with pytest.raises(ValueError, match='poses must'):
        dgr.fuse_scene(bank, np.eye(4))
    with pytest.raises(ValueError, match='outside'):
        dgr.fuse_scene(bank, T2, fragments=[0, 2])
    with pytest.raises(ValueError, match='mask'):
        dgr.fuse_scene(bank, T2, fragments=np.ones(3, bool))
    with pytest.raises(ValueError, match='empty'):
        dgr.fuse_scene(bank, T2, fragments=np.zeros(2, bool))
    with pytest.raises(ValueError, match='voxel_size'):
        dgr.fuse_scene(bank, T2, voxel_size=-1.0)
    for bad_min in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='min_points'):
            dgr.fuse_scene(bank, T2, min_points=bad_min)
    with pytest.raises(ValueError, match='one cloud per fragment'):
        dgr.fuse_scene(bank, T2, clouds=[x])
    with pytest.raises(ValueError, match='cloud 1'):
        dgr.fuse_scene(bank, T2, clouds=[x, np.zeros((3, 2))])
    Tn = T2.copy()
    Tn[1, 0, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        dgr.fuse_scene(bank, Tn)
    with pytest.raises(ValueError, match='finite'):
        dgr.fuse_scene(bank, Tn, fragments=[1])


def test_overlap_ratio_keeps_its_default():
    from deepglobalregistration_amd.util.pointcloud import compute_overlap_ratio
    assert inspect.signature(compute_overlap_ratio).parameters['downsample'].default is True


# ---- the numpy statement, by hand ------------------------------------------------------------------------------------
def test_reference_lattice_by_hand():
    """Voxel 0.25, origin 0, coordinates on multiples of 1/16 (every quotient is exact): floor for negatives, -0.0 in voxel
    0, a point on a face in the voxel above it, means of the fixed-point sums."""
    x = np.array([[0.0625, 0.0, 0.1875],      # voxel (0, 0, 0), fractions 1/4, 0, 3/4
                  [-0.0625, 0.25, -0.25],     # (-1, 1, -1): fractions 3/4, 0 (on the face: the voxel above), 0
                  [0.1875, -0.0, 0.0625],     # (0, 0, 0) again: -0.0 is in voxel 0
                  [-0.1875, 0.4375, -0.0625],  # (-1, 1, -1) again: fractions 1/4, 3/4, 3/4
                  [0.5, 0.5, 0.5]], np.float32)   # (2, 2, 2) exactly on three faces
    r = voxel_mean_ref(x, 0.25)
    assert r['first'].tolist() == [0, 1, 4] and r['count'].tolist() == [2, 2, 1] and r['dropped'] == 0
    assert r['coords'].tolist() == [[0, 0, 0], [-1, 1, -1], [2, 2, 2]] and r['coords'].dtype == np.int32
    q = ONE // 4
    assert r['sums'].tolist() == [[q + 3 * q, 0, 3 * q + q], [3 * q + q, 3 * q, 3 * q], [0, 0, 0]]
    np.testing.assert_array_equal(r['mean'], [[0.125, 0.0, 0.125], [-0.125, 0.34375, -0.15625], [0.5, 0.5, 0.5]])
    # a non-zero origin moves the lattice: origin 1/16 puts x = 1/16 on a face and x = 0 into voxel -1
    r = voxel_mean_ref(x[[0, 2]], 0.25, origin=[0.0625, 0.0625, 0.0])
    assert r['coords'].tolist() == [[0, -1, 0]] and r['count'].tolist() == [2]
    assert r['sums'].tolist() == [[0 + 2 * q, 3 * q + 3 * q, 3 * q + q]]
    np.testing.assert_array_equal(r['mean'], [[0.125, 0.0, 0.125]])


def test_reference_range_and_dropped_rows():
    """The int32 lattice: u = 2^31 - 0.5 and u = -2^31 are kept, u = 2^31 and the float64 just below -2^31 are dropped, as
    are NaN and infinite rows; the rest is unchanged.  A negative u so small that u - floor(u) rounds to 1 contributes the
    whole voxel (k = 2^40): the one inexact case the header names."""
    top, bottom = (2.0 ** 31 - 0.5) * 0.25, -2.0 ** 31 * 0.25
    x = np.array([[top, 0, 0], [2.0 ** 31 * 0.25, 0, 0], [bottom, 0, 0], [np.nextafter(bottom, -np.inf), 0, 0],
                  [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.125, 0.125, 0.125], [-1e-30, 0, 0]], np.float64)
    r = voxel_mean_ref(x, 0.25)
    assert r['dropped'] == 5 and r['first'].tolist() == [0, 2, 7, 8]
    assert r['coords'].tolist() == [[2 ** 31 - 1, 0, 0], [-2 ** 31, 0, 0], [0, 0, 0], [-1, 0, 0]]
    assert r['sums'].tolist() == [[ONE // 2, 0, 0], [0, 0, 0], [ONE // 2] * 3, [ONE, 0, 0]]
    np.testing.assert_array_equal(r['mean'], [[top, 0, 0], [bottom, 0, 0], [0.125] * 3, [0.0, 0, 0]])
    kept = voxel_mean_ref(x[[0, 2, 7, 8]], 0.25)
    for key in ('coords', 'count', 'sums', 'mean'):
        np.testing.assert_array_equal(kept[key], r[key])
    everything_dropped = voxel_mean_ref(x[[1, 4]], 0.25)
    assert everything_dropped['dropped'] == 2 and everything_dropped['mean'].shape == (0, 3)


def test_reference_fragments_and_poses():
    """Fragments under poses: the transform is the fixed-order float64 product; rows are numbered by their row in xyz, so
    the order of the fragment list changes nothing; unselected fragments take no part."""
    x = np.array([[0.0625, 0.0625, 0.0625], [1.0, 1.0, 1.0],       # fragment 0
                  [0.0625, 0.0625, 0.0625],                         # fragment 1
                  [0.3125, 0.0625, 0.0625], [9.0, 9.0, 9.0]], np.float32)   # fragment 2
    off = [0, 2, 3, 5]
    shift = np.eye(4)
    shift[0, 3] = 0.25                                               # fragment 1 moves one voxel along x
    T = np.stack((np.eye(4), shift, np.eye(4)))
    r = voxel_mean_ref(x, 0.25, off, [0, 1, 2], T)
    assert r['first'].tolist() == [0, 1, 2, 4] and r['count'].tolist() == [1, 1, 2, 1]
    assert r['coords'].tolist() == [[0, 0, 0], [4, 4, 4], [1, 0, 0], [36, 36, 36]]
    np.testing.assert_array_equal(r['mean'][2], [0.3125, 0.0625, 0.0625])
    back = voxel_mean_ref(x, 0.25, off, [2, 0, 1], T[[2, 0, 1]])
    for key in ('first', 'coords', 'count', 'sums', 'mean'):
        np.testing.assert_array_equal(back[key], r[key])
    two = voxel_mean_ref(x, 0.25, off, [2, 1], T[[2, 1]])
    assert two['first'].tolist() == [2, 4] and two['count'].tolist() == [2, 1]
    # the transform: one rounding per product and per sum, in the header's order
    rng = np.random.default_rng(0)
    P, y = rng.normal(size=(4, 4)), rng.normal(size=(50, 3)).astype(np.float32)
    want = np.array([[(np.float64(P[i, 0]) * np.float64(a) + np.float64(P[i, 1]) * np.float64(b)) + np.float64(P[i, 2]) * np.float64(c)
                      + P[i, 3] for i in range(3)] for a, b, c in y])
    np.testing.assert_array_equal(transformed_f64(y, P), want)
