"""The numpy statement of `ops.tsdf_mesh` (include/dgr_hip.h at dgr_tsdf_mesh): triangles and vertex normals
of a fused TSDF volume.  The vertices ARE `tsdf_ref.tsdf_points`; the triangles come from a 256-entry table built here by
rule (`mc_table`), the normals from central differences of the volume, every step one correctly rounded float64 operation
in the order written, so the GPU result is compared with it bit for bit.  Vectorised over voxels, cells and vertices."""
import functools

import numpy as np

import tsdf_ref

# corner c of a cell sits at ((c & 1), (c >> 1) & 1, (c >> 2) & 1); edge e = 4 a + j lies along axis a, bit 0 of j is the
# offset on the lower of the two other axes, bit 1 the offset on the higher one
OTHER = ((1, 2), (0, 2), (0, 1))


def edge_low_corner(e):
    """offset (x, y, z) of the low corner of edge e"""
    a, j = e >> 2, e & 3
    o = [0, 0, 0]
    o[OTHER[a][0]], o[OTHER[a][1]] = j & 1, j >> 1
    return tuple(o)


def edge_corners(e):
    lo = edge_low_corner(e)
    c0 = lo[0] | lo[1] << 1 | lo[2] << 2
    return c0, c0 | 1 << (e >> 2)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def faces():
    """the six faces as 4 corners each, counter-clockwise seen from outside the cube: face 2 n + s is the side s of axis n"""
    out = []
    for n in range(3):
        u, v = (n + 1) % 3, (n + 2) % 3                  # e_u x e_v = e_n
        for s in (0, 1):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]      # counter-clockwise seen from +n
            if s == 0:
                ring = ring[::-1]                         # the outside of the low side is -n
            out.append(tuple(s << n | a << u | b << v for a, b in ring))
    return out


FACES = faces()
EDGE_FACES = [frozenset(f for f, ring in enumerate(FACES) if set(edge_corners(e)) <= set(ring)) for e in range(12)]


def face_links(neg4, ring):
    """the links (edge in, edge out) of one face from the signs of its four corners alone: one per maximal cyclic run of
    1..3 negative corners, from the edge by which the counter-clockwise walk enters the run to the edge by which it leaves"""
    links = []
    if all(neg4) or not any(neg4):
        return links
    for s in range(4):
        if neg4[s] and not neg4[s - 1]:
            t = s
            while neg4[(t + 1) % 4]:
                t += 1
            links.append((EDGE_OF[frozenset((ring[s - 1], ring[s]))], EDGE_OF[frozenset((ring[t % 4], ring[(t + 1) % 4]))]))
    return links


def config_loops(cfg):
    """the loops of configuration cfg (bit c = corner c negative): closed edge cycles in link direction, each rotated to its
    fan apex (see `mc_table`), ordered by their smallest edge"""
    succ = {}
    for ring in FACES:
        for a, b in face_links([bool(cfg >> c & 1) for c in ring], ring):
            assert a not in succ
            succ[a] = b
    cut = {e for e in range(12) if (cfg >> edge_corners(e)[0] & 1) != (cfg >> edge_corners(e)[1] & 1)}
    assert set(succ) == cut and set(succ.values()) == cut
    loops, seen = [], set()
    for e in sorted(cut):
        if e in seen:
            continue
        loop = [e]
        while succ[loop[-1]] != e:
            loop.append(succ[loop[-1]])
        seen.update(loop)
        L = len(loop)
        for r in range(L):
            rot = loop[r:] + loop[:r]
            if not any(EDGE_FACES[rot[0]] & EDGE_FACES[rot[k]] for k in range(2, L - 1)):
                break
        else:
            raise AssertionError(f'configuration {cfg}: no admissible fan apex')
        loops.append(rot)
    return loops


@functools.lru_cache(maxsize=None)
def mc_table():
    """(count uint8 [256], edges int8 [256,15] padded with -1): the triangles of every configuration.  A loop of length L
    is the fan (v0, vk, vk+1), k = 1 .. L-2, from the first rotation (starting at its smallest edge) none of whose fan
    diagonals (v0, vk), 2 <= k <= L-2, joins two edges of one cube face.  The link direction already winds every triangle
    so that (v1 - v0) x (v2 - v0) points to the positive side."""
    count = np.zeros(256, np.uint8)
    edges = np.full((256, 15), -1, np.int8)
    for cfg in range(256):
        tris = [(lp[0], lp[k], lp[k + 1]) for lp in config_loops(cfg) for k in range(1, len(lp) - 1)]
        count[cfg] = len(tris)
        edges[cfg, :3 * len(tris)] = np.array(tris, np.int8).reshape(-1)
    count.setflags(write=False)
    edges.setflags(write=False)
    return count, edges


def block_lookup(blocks):
    """a function int [N,3] block coordinates -> index in `blocks` or -1 (per-axis ranks, then one sorted key)"""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    axes = [np.unique(blocks[:, a]) for a in range(3)]

    def key(q):
        k = np.zeros(len(q), np.int64)
        ok = np.ones(len(q), bool)
        for a in range(3):
            pos = np.minimum(np.searchsorted(axes[a], q[:, a]), max(len(axes[a]) - 1, 0))
            ok &= axes[a][pos] == q[:, a] if len(axes[a]) else False
            k = k * (len(axes[a]) + 1) + pos
        return k, ok
    bk, _ = key(blocks)
    order = np.argsort(bk, kind='stable')
    sk = bk[order]

    def find(q):
        q = np.asarray(q, np.int64).reshape(-1, 3)
        if len(blocks) == 0:
            return np.full(len(q), -1, np.int64)
        k, ok = key(q)
        pos = np.minimum(np.searchsorted(sk, k), len(sk) - 1)
        return np.where(ok & (sk[pos] == k), order[pos], -1)
    return find


def _crossings(blocks, tsdf, weight, block, min_weight):
    """(emit bool [nb,B,B,B,3], f1 float32 of the same shape): `tsdf_ref.tsdf_points`'s own test, once more"""
    B, nb = block, len(blocks)
    find = block_lookup(blocks)
    T = tsdf.reshape(nb, B, B, B)
    Wt = weight.reshape(nb, B, B, B)
    f1 = np.zeros((nb, B, B, B, 3), np.float32)
    w1 = np.zeros((nb, B, B, B, 3), np.int32)
    for a in range(3):
        ax = 3 - a
        nbr = find(blocks.astype(np.int64) + np.eye(3, dtype=np.int64)[a])
        have = nbr >= 0
        inner, shifted, last, first = ([slice(None)] * 4 for _ in range(4))
        inner[ax], shifted[ax], last[ax], first[ax] = slice(0, B - 1), slice(1, B), B - 1, 0
        f1[tuple(inner) + (a,)] = T[tuple(shifted)]
        w1[tuple(inner) + (a,)] = Wt[tuple(shifted)]
        first[0], last[0] = nbr[have], np.nonzero(have)[0]
        f1[tuple(last) + (a,)] = T[tuple(first)]
        w1[tuple(last) + (a,)] = Wt[tuple(first)]
    f0, w0 = T[..., None], Wt[..., None]
    lim = np.float32(0.98)
    emit = (w0 >= min_weight) & (w1 >= min_weight) & (f0 >= -lim) & (f0 < lim) & (f1 >= -lim) & (f1 < lim) \
        & ((f0 < 0) != (f1 < 0))
    return emit, f1


def tsdf_mesh(blocks, tsdf, weight, voxel_length, block, min_weight):
    """(xyz float64 [P,3], normal float64 [P,3], tri int32 [T,3]) of a volume in the layout `ops.tsdf_fragment(...,
    return_volume=True)` returns: blocks int32 [nb,3] in any order, tsdf float32 and weight int32 [nb, B^3] with
    l = (lz B + ly) B + lx."""
    B = block
    blocks = np.asarray(blocks, np.int32).reshape(-1, 3)
    nb = len(blocks)
    tsdf = np.asarray(tsdf, np.float32).reshape(nb, B ** 3)
    weight = np.asarray(weight, np.int32).reshape(nb, B ** 3)
    xyz = tsdf_ref.tsdf_points(blocks, tsdf, weight, voxel_length, block, min_weight)
    if nb == 0:
        return xyz, np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    find = block_lookup(blocks)
    flatT, flatW = tsdf.reshape(-1), weight.reshape(-1)
    b64 = blocks.astype(np.int64)

    def voxel(i):
        """flat index into the volume of the global voxel coordinates i [N,3], -1 where the block is absent"""
        k = find(i // B)
        lc = i % B
        return np.where(k >= 0, (k * B ** 3) + (lc[:, 2] * B + lc[:, 1]) * B + lc[:, 0], -1)

    # ---- vertices: the points, and the index each leaves on its edge -------------------------------------------------
    emit, f1 = _crossings(blocks, tsdf, weight, B, min_weight)
    e2v = np.full(emit.shape, -1, np.int64)
    e2v[emit] = np.arange(emit.sum())
    assert emit.sum() == len(xyz)
    k, lz, ly, lx, a = np.nonzero(emit)
    i0 = b64[k] * B + np.stack([lx, ly, lz], 1)
    i1 = i0.copy()
    i1[np.arange(len(a)), a] += 1

    # ---- normals -----------------------------------------------------------------------------------------------------
    def F(j, own):
        at = voxel(j)
        ok = (at >= 0) & (flatW[np.maximum(at, 0)] >= min_weight)
        return np.where(ok, flatT[np.maximum(at, 0)], own).astype(np.float64)

    def gradient(i):
        own = flatT[voxel(i)]
        g = np.zeros((len(i), 3))
        for e in range(3):
            step = np.eye(3, dtype=np.int64)[e]
            g[:, e] = F(i + step, own) - F(i - step, own)
        return g
    r0 = np.abs(flatT[voxel(i0)].astype(np.float64))
    r1 = np.abs(f1[emit].astype(np.float64))
    r = (r0 / (r0 + r1))[:, None]
    g0, g1 = gradient(i0), gradient(i1)
    n = g0 + r * (g1 - g0)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        normal = np.where(length[:, None] == 0, 0.0, n / length[:, None])

    # ---- cells ---------------------------------------------------------------------------------------------------------
    count, edges = mc_table()
    lim = np.float32(0.98)
    good = (flatW >= min_weight) & (flatT >= -lim) & (flatT < lim)
    neg = flatT < 0
    cell = (b64[:, None, :] * B + tsdf_ref._local(B)[None]).reshape(-1, 3)     # cells in output order: block, l
    valid = np.ones(len(cell), bool)
    cfg = np.zeros(len(cell), np.int64)
    for c in range(8):
        at = voxel(cell + np.array([c & 1, c >> 1 & 1, c >> 2 & 1]))
        valid &= (at >= 0) & good[np.maximum(at, 0)]
        cfg |= neg[np.maximum(at, 0)].astype(np.int64) << c
    cfg = np.where(valid, cfg, 0)
    sel = np.nonzero(count[cfg] > 0)[0]
    cfg, cell = cfg[sel], cell[sel]
    ed = edges[cfg].astype(np.int64).reshape(len(sel), 5, 3)
    used = np.arange(5)[None, :] < count[cfg][:, None]
    ci, ti = np.nonzero(used)                                                   # cell-major, then table order
    ed = ed[ci, ti]                                                             # [T,3] edge numbers
    low = np.array([edge_low_corner(e) for e in range(12)], np.int64)
    flat_e2v = e2v.reshape(-1, 3)
    tri = np.zeros((len(ci), 3), np.int64)
    for v in range(3):
        at = voxel(cell[ci] + low[ed[:, v]])
        tri[:, v] = flat_e2v[at, ed[:, v] >> 2]
    assert (tri >= 0).all()
    return xyz, normal, tri.astype(np.int32)


# ---- hand-made volumes the tests share ----------------------------------------------------------------------------------
def grid_blocks(nx, ny, nz, origin=(0, 0, 0)):
    return np.array([[origin[0] + x, origin[1] + y, origin[2] + z] for z in range(nz) for y in range(ny) for x in range(nx)],
                    np.int32)


def fill_volume(blocks, B, fn):
    """tsdf float32 [nb,B^3] = fn(global voxel coordinates float64 [N,3]) in the volume's layout"""
    i = (np.asarray(blocks, np.int64)[:, None, :] * B + tsdf_ref._local(B)[None]).reshape(-1, 3)
    return np.asarray(fn(i.astype(np.float64)), np.float32).reshape(len(blocks), B ** 3)


def noise_volume(seed=0, n=3, B=8):
    """n^3 blocks of clipped Gaussian noise, every voxel valid: the ambiguous faces in bulk.  The outermost layer of voxels
    is positive, so no surface reaches the border of the volume and the mesh is closed."""
    rng = np.random.default_rng(seed)
    blocks = grid_blocks(n, n, n, (-1, -1, -1))
    tsdf = np.clip(rng.standard_normal((len(blocks), B ** 3)) * 0.5, -0.97, 0.97).astype(np.float32)
    i = (blocks.astype(np.int64)[:, None, :] * B + tsdf_ref._local(B)[None])
    shell = ((i == -B) | (i == (n - 1) * B - 1)).any(2)
    tsdf[shell] = np.float32(0.5)
    return blocks, tsdf, np.ones(tsdf.shape, np.int32)


SPHERE = dict(centre=(0.31, -0.27, 0.13), radius=6.1, trunc=4.0)    # in voxels; the centre near the common corner, off the lattice


def sphere_volume(B=8, origin=(-1, -1, -1)):
    """2 x 2 x 2 blocks around a sphere: tsdf = clip((|x + 0.5 - c| - R) / trunc, -1, 1), negative inside"""
    blocks = grid_blocks(2, 2, 2, origin)
    c, R, tr = np.array(SPHERE['centre']), SPHERE['radius'], SPHERE['trunc']
    tsdf = fill_volume(blocks, B, lambda i: np.clip((np.linalg.norm(i + 0.5 - c, axis=1) - R) / tr, -1.0, 1.0))
    return blocks, tsdf, np.ones(tsdf.shape, np.int32)


def directed_edges(tri):
    """(edges int64 [3T] as a * 2^32 + b, their counts): the directed edges of the triangles"""
    t = np.asarray(tri, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return d[:, 0] << 32 | d[:, 1]


def is_closed(tri):
    """every directed edge exactly once and its reverse exactly once"""
    d = directed_edges(tri)
    u, n = np.unique(d, return_counts=True)
    rev = (u & 0xffffffff) << 32 | u >> 32
    return bool((n == 1).all() and np.isin(rev, u).all())
