"""The synthetic depth sequences the TSDF tests share, and their numpy statements, each computed once per session."""
import functools

from deepglobalregistration_amd import synth
import tsdf_ref

# the two sizes of the issue: image, focal length, frames, voxel, truncation
SIZES = {'small': dict(width=80, height=60, focal=70, n_frames=3, voxel=0.04, trunc=0.16),
         'large': dict(width=160, height=120, focal=140, n_frames=6, voxel=0.02, trunc=0.08)}


@functools.lru_cache(maxsize=None)
def sequence(size, seed=0):
    """(depth, intrinsic, poses, boxes) of synth_rgbd at one of SIZES; read-only"""
    s = SIZES[size]
    depth, K, poses, boxes = synth.synth_rgbd(seed, s['n_frames'], s['width'], s['height'], s['focal'])
    depth.setflags(write=False)
    poses.setflags(write=False)
    return depth, K, poses, boxes


@functools.lru_cache(maxsize=None)
def statement(size, seed=0, block=16, stride=4, min_weight=1):
    depth, K, poses, _ = sequence(size, seed)
    s = SIZES[size]
    out = tsdf_ref.tsdf_fragment(depth, K, poses, s['voxel'], s['trunc'], block=block, stride=stride, min_weight=min_weight,
                                 return_cross=True)
    for a in out.values():
        a.setflags(write=False)
    return out
