"""Device-event times of `ops.tsdf_mesh` (csrc/tsdfmesh.hip) on the volume of a fragment-sized input: tools/tsdf_bench.py's
`synth_rgbd(0)` sequence of 50 frames at 640 x 480, 8-mm voxels, 4-cm truncation, stride 4, blocks of 8^3 and of 16^3 voxels.

Per block size: median / min / max of `--reps` whole calls after 3 warm-up calls (everything between the two events: output
allocation, hash, counts, scans, the one host synchronisation, vertices with normals, triangles; the volume is on the
device already, where `ops.tsdf_fragment` left it), the vertex and triangle counts, and the fragment call's time from the
same run.  Beside them ONE cold run of the numpy statement (tests/tsdf_mesh_ref.py) on the `large` fixture of
tests/tsdf_cases.py on the host's wall clock -- an order of magnitude, not a median -- with the library's time on that same
volume, the two results compared for exact equality.  The one condition: there the call is not slower than the statement.

    python tools/tsdf_mesh_bench.py [--reps 20] [--out profiles/tsdf_mesh_bench.json] [--commit HASH]
    python tools/tsdf_mesh_bench.py --profile-only     # three calls per block size and nothing else: what a kernel trace wraps

The colour leg (`--color`): per block size the mesh call with and without `rgb_sum=` on the volume fused
from the same frames with `synth_color` images, the vertex colours compared with the fragment's point colours bit for bit,
and the median / maximum |vertex colour - texture at the vertex| in levels of 255 (information only).  The record goes
into the output file beside tools/tsdf_bench.py's, under `mesh`.

    python tools/tsdf_mesh_bench.py --color [--reps 20] [--out profiles/tsdf_color_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
from tsdf_bench import FOCAL, FRAMES, HEIGHT, STRIDE, SWEEP, TRUNC, VOXEL, WIDTH  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--profile-only', action='store_true')
    ap.add_argument('--color', action='store_true', help='the colour leg instead (see the module docstring)')
    a = ap.parse_args()
    from deepglobalregistration_amd import ops, synth
    import tsdf_cases
    import tsdf_mesh_ref
    from voxel_mean_bench import commit_stamp, timed
    if not torch.cuda.is_available():
        raise SystemExit('tsdf_mesh_bench measures on the GPU; there is nothing to time without one')
    depth, K, poses, _ = synth.synth_rgbd(0, FRAMES, WIDTH, HEIGHT, FOCAL, sweep_deg=SWEEP)
    depth_dev = torch.from_numpy(depth).cuda()
    if a.color:
        color = synth.synth_color(depth, K, poses, seed=0)
        color_dev = torch.from_numpy(color).cuda()
        rec = {'commit': a.commit or commit_stamp(), 'device': torch.cuda.get_device_name(0), 'reps': a.reps}
        for block in (8, 16):
            vol = ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE, return_volume=True, color=color_dev)

            def mesh(rgb_sum=None):
                return ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], VOXEL, block=block, rgb_sum=rgb_sum)
            m = mesh(vol['rgb_sum'])
            if not torch.equal(m['color'].view(torch.int64), vol['color'].view(torch.int64)):
                raise SystemExit(f"block {block}: the vertex colours are not the fragment's point colours")
            err = np.abs(255.0 * m['color'].cpu().numpy() - synth.color_texture(m['xyz'].cpu().numpy(), 0).astype(np.float64))
            rec[f'block{block}'] = {'vertices': len(m['xyz']), 'triangles': len(m['triangles']), 'mesh_ms': timed(mesh, a.reps),
                                    'mesh_color_ms': timed(lambda: mesh(vol['rgb_sum']), a.reps),
                                    'texture_error_levels': {'median': float(np.median(err)), 'max': float(err.max())}}
            del m, vol
        out = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        out['mesh'] = rec
        print(json.dumps(rec, indent=1))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    out = {'commit': a.commit or commit_stamp(), 'device': torch.cuda.get_device_name(0), 'reps': a.reps,
           'input': {'width': WIDTH, 'height': HEIGHT, 'focal': FOCAL, 'frames': FRAMES, 'sweep_deg': SWEEP, 'voxel_length': VOXEL,
                     'sdf_trunc': TRUNC, 'stride': STRIDE}}
    ok = True
    for block in (8, 16):
        def fragment():
            return ops.tsdf_fragment(depth_dev, K, poses, VOXEL, TRUNC, block=block, stride=STRIDE, return_volume=True)
        vol = fragment()

        def mesh(normals=True):
            return ops.tsdf_mesh(vol['blocks'], vol['tsdf'], vol['weight'], VOXEL, block=block, normals=normals)
        if a.profile_only:
            for _ in range(3):
                mesh()
            torch.cuda.synchronize()
            continue
        m = mesh()
        if not torch.equal(m['xyz'], vol['xyz']):
            raise SystemExit(f'block {block}: the vertices are not the points of the fragment')
        entry = {'block': block, 'blocks': len(vol['blocks']), 'voxels': len(vol['blocks']) * block ** 3,
                 'vertices': len(m['xyz']), 'triangles': len(m['triangles']),
                 'mesh_ms': timed(mesh, a.reps), 'mesh_without_normals_ms': timed(lambda: mesh(False), a.reps),
                 'fragment_ms': timed(fragment, a.reps)}
        del m
        # the statement, once and cold, on the `large` fixture; the library on the same volume
        s = tsdf_cases.SIZES['large']
        ld, lK, lposes, _ = tsdf_cases.sequence('large')
        lv = ops.tsdf_fragment(ld, lK, lposes, s['voxel'], s['trunc'], block=block, stride=4, return_volume=True)
        host = [lv[k].cpu().numpy() for k in ('blocks', 'tsdf', 'weight')]
        t0 = time.perf_counter()
        want = tsdf_mesh_ref.tsdf_mesh(*host, s['voxel'], block, 1)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = ops.tsdf_mesh(lv['blocks'], lv['tsdf'], lv['weight'], s['voxel'], block=block)
        for key, w in zip(('xyz', 'normal', 'triangles'), want):
            if got[key].cpu().numpy().tobytes() != np.ascontiguousarray(w).tobytes():
                raise SystemExit(f'block {block}: the library and the numpy statement disagree on {key}')
        dev_ms = timed(lambda: ops.tsdf_mesh(lv['blocks'], lv['tsdf'], lv['weight'], s['voxel'], block=block), a.reps)
        entry['large_fixture'] = {'blocks': len(host[0]), 'vertices': len(want[0]), 'triangles': len(want[2]),
                                  'numpy_statement_host_ms': host_ms, 'numpy_statement_runs': 1, 'mesh_ms': dev_ms,
                                  'numpy_over_device': host_ms / dev_ms['median_ms']}
        ok &= dev_ms['median_ms'] <= host_ms
        out[f'block{block}'] = entry
    if a.profile_only:
        return
    out['not_slower_than_numpy'] = bool(ok)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not ok:
        raise SystemExit('the library is slower on the device than the numpy statement on the host')


if __name__ == '__main__':
    main()
