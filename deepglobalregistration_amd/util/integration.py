"""Depth frames -> fragments (util/integration.py of the reference): every `n_frames_per_fragment` frames of a 3DMatch-style
sequence are fused into one TSDF volume on the GPU (`ops.tsdf_fragment`) and the surface points are written as
`fragment-N.ply`: the vertices of the mesh the reference writes, without its triangles (the loaders read vertices only).
With `mesh` (`--mesh`) the file is that mesh: the same vertices in the same order, their normals and the triangles
(`ops.tsdf_mesh`).  With `color` (`--color`) the `*.color.png` beside every depth frame is fused too, as the reference's
RGB8 volume does, and the points or the mesh's vertices are written with their colours; without it colour files are
neither read nor required.

    python -m deepglobalregistration_amd.util.integration DATASET OUTPUT [--mesh] [--color]
"""
import argparse
import os

import numpy as np

from ..eval.formats import read_png_gray, read_png_rgb8, write_ply, write_ply_mesh


def read_pose(pose_file):
    """4x4 camera-to-world matrix of a `.pose.txt` file."""
    pose = np.loadtxt(pose_file, dtype=np.float64)
    if pose.shape != (4, 4):
        raise ValueError(f'{pose_file}: expected a 4x4 matrix, got {pose.shape}')
    return pose


def read_intrinsics(intrinsic_file):
    """(fx, fy, cx, cy) of a 3x3 camera matrix file."""
    K = np.loadtxt(intrinsic_file, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] < 2 or K.shape[1] < 3:
        raise ValueError(f'{intrinsic_file}: expected a 3x3 camera matrix, got {K.shape}')
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def read_depth(depth_file):
    """uint16 [H,W] raw depth (millimetres in 3DMatch) of a 16-bit grayscale PNG."""
    img = read_png_gray(depth_file)
    if img.dtype != np.uint16:
        raise ValueError(f'{depth_file}: expected a 16-bit depth image')
    return img


def integrate_frames_for_fragment(depth_files, pose_files, seq_path, intrinsic, fragment_id, n_frames_per_fragment,
                                  voxel_length=0.008, sdf_trunc=0.04, relative_to_first=False, mesh=False, color_files=None,
                                  **tsdf_args):
    """The points (float64 [P,3] device tensor) of fragment `fragment_id`: frames [id n, (id + 1) n) of the sorted file
    lists, fused by `ops.tsdf_fragment` (further keyword arguments go to it).  `relative_to_first`: the fragment in the
    frame of its first camera (every pose premultiplied by the inverse of the fragment's first).  With `mesh` the dict of
    `ops.tsdf_mesh` on the fused volume instead: `xyz` (the same points), `normal`, `triangles`.  With `color_files` (the
    sorted colour images, one per depth file) the colours are fused too and the result is a dict in both cases, with
    `color` float64 [P,3] in [0, 1]; a colour image of another size than its depth image is a ValueError."""
    from .. import ops
    start = fragment_id * n_frames_per_fragment
    end = min(start + n_frames_per_fragment, len(pose_files))
    if start >= end:
        raise ValueError(f'fragment {fragment_id} has no frames')
    depth = np.stack([read_depth(os.path.join(seq_path, depth_files[i])) for i in range(start, end)])
    pose = np.stack([read_pose(os.path.join(seq_path, pose_files[i])) for i in range(start, end)])
    if relative_to_first:
        pose = np.linalg.inv(pose[0]) @ pose
    if color_files is not None:
        images = []
        for i in range(start, end):
            img = read_png_rgb8(os.path.join(seq_path, color_files[i]))
            if img.shape[:2] != depth.shape[1:]:
                raise ValueError(f'{os.path.join(seq_path, color_files[i])}: {img.shape[1]} x {img.shape[0]} pixels, the depth '
                                 f'image {depth_files[i]} has {depth.shape[2]} x {depth.shape[1]}')
            images.append(img)
        tsdf_args = dict(tsdf_args, color=np.stack(images))
    if not mesh:
        return ops.tsdf_fragment(depth, intrinsic, pose, voxel_length, sdf_trunc, **tsdf_args)
    tsdf_args = dict(tsdf_args, return_volume=True)
    vol = ops.tsdf_fragment(depth, intrinsic, pose, voxel_length, sdf_trunc, **tsdf_args)
    return ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], voxel_length, block=tsdf_args.get('block', 16),
                         min_weight=tsdf_args.get('min_weight', 1), rgb_sum=vol.get('rgb_sum'))


def list_color_files(seq_path, n_depth):
    """The sorted `*.color.png` files of a sequence directory; ValueError unless there are `n_depth` of them."""
    color_files = sorted(f for f in os.listdir(seq_path) if f.endswith('.color.png'))
    if len(color_files) != n_depth:
        raise ValueError(f'{seq_path}: {n_depth} depth files but {len(color_files)} colour files')
    return color_files


def list_sequence(seq_path):
    """(intrinsic, depth files, pose files) of a sequence directory, found as the reference finds them: sorted
    `*.depth.png` and `*.pose.txt`, and `intrinsics.txt` in the directory or `camera-intrinsics.txt` one level up."""
    files = os.listdir(seq_path)
    if 'intrinsics.txt' in files:
        intrinsic = read_intrinsics(os.path.join(seq_path, 'intrinsics.txt'))
    else:
        intrinsic = read_intrinsics(os.path.join(seq_path, '..', 'camera-intrinsics.txt'))
    depth_files = sorted(f for f in files if f.endswith('.depth.png'))
    pose_files = sorted(f for f in files if f.endswith('.pose.txt'))
    if not depth_files:
        raise ValueError(f'{seq_path}: no *.depth.png files')
    if len(depth_files) != len(pose_files):
        raise ValueError(f'{seq_path}: {len(depth_files)} depth files but {len(pose_files)} pose files')
    return intrinsic, depth_files, pose_files


def process_seq(seq_path, output_path, n_frames_per_fragment=50, voxel_length=0.008, sdf_trunc=0.04,
                relative_to_first=False, mesh=False, color=False, **tsdf_args):
    """Writes `fragment-{id}.ply` into `output_path` for every `n_frames_per_fragment` frames of the sequence (the last
    fragment takes what is left): the surface points, or with `mesh` the triangle mesh with vertex normals, whose vertices
    are those points.  With `color` the sorted `*.color.png` files (as many as depth files, each of its depth image's size:
    else ValueError) are fused too and the points or vertices are written with `uchar red green blue`.  Returns the files
    written."""
    intrinsic, depth_files, pose_files = list_sequence(seq_path)
    color_files = list_color_files(seq_path, len(depth_files)) if color else None
    n_fragments = (len(depth_files) + n_frames_per_fragment - 1) // n_frames_per_fragment
    os.makedirs(output_path, exist_ok=True)
    written = []
    for fragment_id in range(n_fragments):
        out = integrate_frames_for_fragment(depth_files, pose_files, seq_path, intrinsic, fragment_id, n_frames_per_fragment,
                                            voxel_length, sdf_trunc, relative_to_first, mesh, color_files, **tsdf_args)
        name = os.path.join(output_path, 'fragment-{}.ply'.format(fragment_id))
        colors = out['color'].cpu().numpy() if color else None
        if mesh:
            write_ply_mesh(name, out['xyz'].cpu().numpy(), out['triangles'].cpu().numpy(), out['normal'].cpu().numpy(),
                           colors=colors)
        elif color:
            write_ply(name, out['xyz'].cpu().numpy(), colors=colors)
        else:
            write_ply(name, out.cpu().numpy())
        written.append(name)
    return written


def main(argv=None):
    parser = argparse.ArgumentParser(description='Depth integration for a 3DMatch-style raw dataset')
    parser.add_argument('dataset', help='path to the scene: directories seq* with depth images and poses')
    parser.add_argument('output', help='path to the output fragments')
    parser.add_argument('--frames', type=int, default=50, help='frames per fragment')
    parser.add_argument('--voxel', type=float, default=0.008)
    parser.add_argument('--relative-to-first', action='store_true', help="fragments in their first camera's frame")
    parser.add_argument('--mesh', action='store_true', help='write triangle meshes with vertex normals, not points only')
    parser.add_argument('--color', action='store_true', help='fuse the *.color.png beside every depth frame; write colours')
    args = parser.parse_args(argv)
    scene_name = os.path.basename(os.path.normpath(args.dataset))
    output_scene_path = os.path.join(args.output, scene_name)
    for seq in sorted(s for s in os.listdir(args.dataset) if s.startswith('seq')):
        files = process_seq(os.path.join(args.dataset, seq), os.path.join(output_scene_path, seq), args.frames, args.voxel,
                            relative_to_first=args.relative_to_first, mesh=args.mesh, color=args.color)
        print(f'{seq}: {len(files)} fragments -> {os.path.join(output_scene_path, seq)}')


if __name__ == '__main__':
    main()
