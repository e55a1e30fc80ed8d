"""CPU: the numpy statement of `ops.tsdf_mesh` (tests/tsdf_mesh_ref.py) checked on its own -- the triangle table against
the rule it is built from and against the committed header, the meshes of hand-made volumes and of the TSDF fixtures for
the properties a surface must have -- and the PLY mesh writer and reader."""
import importlib.util
import os
import re

import numpy as np
import pytest

import tsdf_cases
import tsdf_mesh_ref as ref
import tsdf_ref
from conftest import ROOT

HEADER = os.path.join(ROOT, 'deepglobalregistration_amd', 'csrc', 'mc_table.h')


def _bits(cfg, ring):
    return tuple(bool(cfg >> c & 1) for c in ring)


def _triangles(cfg):
    count, edges = ref.mc_table()
    return [tuple(int(e) for e in edges[cfg, 3 * j:3 * j + 3]) for j in range(count[cfg])]


def _cut_edges(cfg):
    return {e for e in range(12) if (cfg >> ref.edge_corners(e)[0] & 1) != (cfg >> ref.edge_corners(e)[1] & 1)}


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_every_configuration_uses_exactly_its_sign_changing_edges():
    count, edges = ref.mc_table()
    for cfg in range(256):
        used = {e for t in _triangles(cfg) for e in t}
        assert used == _cut_edges(cfg), cfg
        assert (edges[cfg, 3 * count[cfg]:] == -1).all() and (edges[cfg, :3 * count[cfg]] >= 0).all()
        for t in _triangles(cfg):
            assert len(set(t)) == 3


def test_triangle_counts():
    count, _ = ref.mc_table()
    assert int(count.sum()) == 820 and int(count.max()) == 5
    assert np.bincount(count).tolist() == [2, 16, 50, 80, 76, 32]
    assert count[0] == 0 and count[255] == 0


def test_every_configuration_is_a_set_of_closed_fans_facing_the_positive_side():
    """Within a cell every directed triangle edge occurs once; the ones without a reverse are the loops' links, each on
    exactly one cube face; no fan diagonal lies on a cube face.  With the vertices at the edge midpoints, the area vector
    of every loop points from the negative corners its edges touch towards the positive ones."""
    mid = np.array([(np.array(ref.edge_low_corner(e), float) + np.eye(3)[e >> 2] * 0.5) for e in range(12)])
    corners = np.array([[c & 1, c >> 1 & 1, c >> 2 & 1] for c in range(8)], float)
    for cfg in range(1, 255):
        tris = _triangles(cfg)
        d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert len(set(d)) == len(d), cfg
        for a, b in d:
            if (b, a) in d:      # a fan diagonal
                assert not (ref.EDGE_FACES[a] & ref.EDGE_FACES[b]), (cfg, a, b)
            else:                # a link
                assert len(ref.EDGE_FACES[a] & ref.EDGE_FACES[b]) == 1, (cfg, a, b)
        for lp in ref.config_loops(cfg):
            # a loop separates the negative corners it cuts off from the rest: its area vector points away from them
            area = sum(np.cross(mid[lp[k]] - mid[lp[0]], mid[lp[k + 1]] - mid[lp[0]]) for k in range(1, len(lp) - 1))
            ends = {c for e in lp for c in ref.edge_corners(e)}
            neg = [c for c in ends if cfg >> c & 1]
            pos = [c for c in ends if not cfg >> c & 1]
            assert area @ (corners[pos].mean(0) - corners[neg].mean(0)) > 0, (cfg, lp)


def _ambiguous(cfg):
    return any(_bits(cfg, ring) in ((True, False, True, False), (False, True, False, True)) for ring in ref.FACES)


def test_complementary_configurations():
    """What holds: the complement of a configuration has the same loops reversed EXACTLY when no face of the cube carries
    two diagonal negative corners -- 136 of the 256 configurations.  On such an ambiguous face the rule cuts off the
    NEGATIVE corners, which the complement swaps, so the other 120 differ."""
    def canon(lp):
        i = lp.index(min(lp))
        return tuple(lp[i:] + lp[:i])
    same = 0
    for cfg in range(256):
        mine = sorted(canon(lp) for lp in ref.config_loops(cfg))
        other = sorted(canon(lp[::-1]) for lp in ref.config_loops(255 - cfg))
        assert (mine == other) == (not _ambiguous(cfg)), cfg
        same += mine == other
    assert same == 136


def test_the_links_of_a_face_depend_on_its_four_signs_only():
    """read back from the TABLE: the directed triangle edges that lie on a face are the rule's links for that face's signs,
    whatever the other four corners are -- so two cells that share a face cut it alike"""
    for f, ring in enumerate(ref.FACES):
        seen = {}
        for cfg in range(256):
            on_face = {(t[i], t[(i + 1) % 3]) for t in _triangles(cfg) for i in range(3)
                       if f in ref.EDGE_FACES[t[i]] and f in ref.EDGE_FACES[t[(i + 1) % 3]]}
            signs = _bits(cfg, ring)
            assert on_face == set(ref.face_links(signs, ring)), (f, cfg)
            assert seen.setdefault(signs, on_face) == on_face
        assert len(seen) == 16
    # the face seen from the neighbouring cell: same corners, opposite sense -- every link reversed
    for n in range(3):
        lo, hi = ref.FACES[2 * n], ref.FACES[2 * n + 1]
        shift = 1 << n
        for cfg4 in range(16):
            signs_hi = tuple(bool(cfg4 >> k & 1) for k in range(4))
            neg = {c for c, s in zip(hi, signs_hi) if s}
            signs_lo = tuple((c | shift) in neg for c in lo)

            def as_pairs(links, ring_shift):
                return {(frozenset(x ^ ring_shift for x in ref.edge_corners(a)), frozenset(x ^ ring_shift for x in ref.edge_corners(b)))
                        for a, b in links}
            a = as_pairs(ref.face_links(signs_hi, hi), 0)
            b = as_pairs(ref.face_links(signs_lo, lo), shift)
            assert a == {(y, x) for x, y in b}, (n, cfg4)


def _load_generator():
    spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(ROOT, 'tools', 'gen_mc_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_header_is_the_generators_output_and_the_statements_table(tmp_path):
    gen = _load_generator()
    out = gen.main([str(tmp_path / 'mc_table.h')])
    fresh = open(out, 'rb').read()
    assert fresh == open(HEADER, 'rb').read()
    text = re.sub(r'//[^\n]*', '', fresh.decode())
    body = re.findall(r'\{([^{}]*)\}', text.split('dgr_mc_edges')[1])
    edges = np.array([[int(v) for v in row.split(',') if v.strip()] for row in body if row.strip()], np.int8)
    counts = np.array([int(v) for v in re.search(r'dgr_mc_count\[256\] = \{([^}]*)\}', text).group(1).split(',') if v.strip()])
    count, want = ref.mc_table()
    assert edges.shape == (256, 15) and np.array_equal(edges, want)
    assert counts.shape == (256,) and np.array_equal(counts, count)
    assert f'#define DGR_MC_TRIANGLES {int(count.sum())}\n' in fresh.decode()


# ---- hand-made volumes ----------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_noise_volume_is_watertight_and_meets_every_configuration():
    blocks, tsdf, weight = ref.noise_volume()
    assert len(blocks) == 27 and (weight >= 1).all() and (np.abs(tsdf) < 0.98).all()
    # precondition: all 254 non-trivial configurations occur
    T = np.zeros((24, 24, 24), np.float32)
    i = (blocks.astype(np.int64)[:, None, :] * 8 + tsdf_ref._local(8)[None]).reshape(-1, 3) + 8
    T[i[:, 2], i[:, 1], i[:, 0]] = tsdf.reshape(-1)
    cfg = np.zeros((23, 23, 23), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2 & 1
        cfg |= (T[dz:dz + 23, dy:dy + 23, dx:dx + 23] < 0).astype(np.int64) << c
    assert set(np.unique(cfg)) >= set(range(1, 255))
    xyz, normal, tri = ref.tsdf_mesh(blocks, tsdf, weight, 0.01, 8, 1)
    count, _ = ref.mc_table()
    assert len(tri) == count[cfg].sum() and tri.dtype == np.int32
    assert ref.is_closed(tri)
    assert _same_bits(xyz, tsdf_ref.tsdf_points(blocks, tsdf, weight, 0.01, 8, 1))
    assert set(np.unique(tri)) == set(range(len(xyz)))          # closed: every crossing is used
    assert np.isfinite(normal).all()


def _sphere_mesh():
    blocks, tsdf, weight = ref.sphere_volume()
    return (blocks, tsdf, weight) + ref.tsdf_mesh(blocks, tsdf, weight, 1.0, 8, 1)


def test_sphere_is_closed_outward_and_has_the_right_volume_and_normals():
    blocks, tsdf, weight, xyz, normal, tri = _sphere_mesh()
    assert len(tri) > 1000 and ref.is_closed(tri)
    v = xyz[tri]
    volume = np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6
    analytic = 4 / 3 * np.pi * ref.SPHERE['radius'] ** 3
    # measured: 935.50 against 950.78, -1.61 % (702 vertices, 1400 triangles; the chords of a sphere of 6.1 voxels)
    assert volume > 0 and abs(volume / analytic - 1) < 0.02, (volume, analytic)
    face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert (np.einsum('ij,ij->i', face, normal[tri].sum(1)) > 0).all()
    radial = xyz - np.array(ref.SPHERE['centre'])
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    angle = np.degrees(np.arccos(np.clip(np.einsum('ij,ij->i', radial, normal), -1, 1)))
    # measured: at most 0.331 degrees (median 0.12)
    assert angle.max() < 1.0, angle.max()
    assert np.allclose(np.linalg.norm(normal, axis=1), 1.0, atol=1e-15)


def _no_directed_edge_twice(tri):
    d = ref.directed_edges(tri)
    return len(np.unique(d)) == len(d)


def test_sphere_with_one_block_removed_is_open_not_broken():
    blocks, tsdf, weight = ref.sphere_volume()
    keep = np.arange(8) != 5
    xyz, normal, tri = ref.tsdf_mesh(blocks[keep], tsdf[keep], weight[keep], 1.0, 8, 1)
    assert 0 < len(tri) < 1400 and not ref.is_closed(tri) and _no_directed_edge_twice(tri)
    assert _same_bits(xyz, tsdf_ref.tsdf_points(blocks[keep], tsdf[keep], weight[keep], 1.0, 8, 1))
    assert (tri >= 0).all() and tri.max() < len(xyz)
    # the order of the block list changes the numbering, not the surface
    perm = np.random.default_rng(1).permutation(8)
    a = ref.tsdf_mesh(blocks, tsdf, weight, 1.0, 8, 1)
    b = ref.tsdf_mesh(blocks[perm], tsdf[perm], weight[perm], 1.0, 8, 1)
    assert not np.array_equal(a[0], b[0])

    def as_set(xyz, normal, tri):
        return sorted(tuple(np.concatenate([xyz[t].reshape(-1), normal[t].reshape(-1)]).tolist()) for t in tri)
    assert as_set(*a) == as_set(*b)


@pytest.mark.parametrize('block', [8, 16])
@pytest.mark.parametrize('size', ['small', 'large'])
def test_fixtures_give_open_meshes_on_the_fragments_points(size, block):
    st = tsdf_cases.statement(size, 0, block, 4)
    xyz, normal, tri = ref.tsdf_mesh(st['blocks'], st['tsdf'], st['weight'], tsdf_cases.SIZES[size]['voxel'], block, 1)
    assert _same_bits(xyz, st['xyz']) and len(tri) > len(xyz)
    assert _no_directed_edge_twice(tri) and (tri >= 0).all() and tri.max() < len(xyz)
    assert np.isfinite(normal).all() and np.allclose(np.linalg.norm(normal, axis=1), 1.0, atol=1e-15)
    v = xyz[tri]
    face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    agree = np.einsum('ij,ij->i', face, normal[tri].sum(1)) > 0
    assert agree.mean() > 0.99       # (noisy borders of the observed region may disagree; the sphere test is the strict one)


def test_empty_and_all_positive_volumes():
    xyz, normal, tri = ref.tsdf_mesh(np.zeros((0, 3), np.int32), np.zeros((0, 512), np.float32), np.zeros((0, 512), np.int32),
                                     0.01, 8, 1)
    assert xyz.shape == (0, 3) and normal.shape == (0, 3) and tri.shape == (0, 3) and tri.dtype == np.int32
    blocks = ref.grid_blocks(2, 1, 1)
    xyz, normal, tri = ref.tsdf_mesh(blocks, np.full((2, 512), 0.5, np.float32), np.ones((2, 512), np.int32), 0.01, 8, 1)
    assert xyz.shape == (0, 3) and normal.shape == (0, 3) and tri.shape == (0, 3)


# ---- files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_normals', [False, True])
@pytest.mark.parametrize('binary', [False, True])
def test_ply_mesh_round_trip(tmp_path, binary, with_normals):
    from deepglobalregistration_amd.eval.formats import read_ply, read_ply_mesh, write_ply, write_ply_mesh
    _, _, _, xyz, normal, tri = _sphere_mesh()
    name = str(tmp_path / 'mesh.ply')
    write_ply_mesh(name, xyz, tri, normal if with_normals else None, binary=binary)
    got = read_ply_mesh(name)
    assert _same_bits(got['xyz'], xyz) and got['triangles'].dtype == np.int32 and np.array_equal(got['triangles'], tri)
    assert ('normals' in got) == with_normals
    if with_normals:
        assert _same_bits(got['normals'], normal)
    # read_ply returns the same vertices from a mesh file as from the points-only file of the same fragment
    points = str(tmp_path / 'points.ply')
    write_ply(points, xyz, binary=binary)
    assert _same_bits(read_ply(name), read_ply(points)) and _same_bits(read_ply(name), xyz)
    head = open(name, 'rb').read().split(b'end_header\n')[0].decode()
    assert 'property double x' in head and f'element face {len(tri)}' in head
    assert 'property list uchar int vertex_indices' in head and ('property double nx' in head) == with_normals


def test_ply_mesh_rejects_bad_input_and_writes_empty_meshes(tmp_path):
    from deepglobalregistration_amd.eval.formats import read_ply, read_ply_mesh, write_ply_mesh
    name = str(tmp_path / 'm.ply')
    xyz = np.zeros((3, 3))
    with pytest.raises(ValueError):
        write_ply_mesh(name, xyz, [[0, 1, 3]])
    with pytest.raises(ValueError):
        write_ply_mesh(name, xyz, [[0, 1, 2]], normals=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        write_ply_mesh(name, xyz, np.array([[0.0, 1.0, 2.0]]))
    for binary in (False, True):
        write_ply_mesh(name, np.zeros((0, 3)), np.zeros((0, 3), np.int32), binary=binary)
        got = read_ply_mesh(name)
        assert got['xyz'].shape == (0, 3) and got['triangles'].shape == (0, 3) and read_ply(name).shape == (0, 3)
