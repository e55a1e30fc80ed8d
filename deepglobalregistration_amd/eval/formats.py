"""Readers / writers of the file formats the reference's data loaders consume."""
import os
import struct

import numpy as np


# ---- gt.log trajectories (3DMatch geometric-registration benchmark) -----------------------------------
def read_trajectory(filename, dim=4):
    """util/file.py:69-90: a sequence of records "i j n" + dim rows of a dim x dim pose.  Returns a list of
    (metadata [int, ...], pose [dim, dim] float64)."""
    out = []
    with open(filename, 'r') as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) % (dim + 1):
        raise ValueError(f'{filename}: {len(lines)} non-empty lines is not a multiple of {dim + 1}')
    for r in range(0, len(lines), dim + 1):
        meta = [int(v) for v in lines[r].split()]
        pose = np.array([[float(v) for v in lines[r + 1 + k].split()] for k in range(dim)], np.float64)
        if pose.shape != (dim, dim):
            raise ValueError(f'{filename}: malformed pose in record {r // (dim + 1)}')
        out.append((meta, pose))
    return out


def write_trajectory(filename, records):
    with open(filename, 'w') as f:
        for meta, pose in records:
            f.write('\t'.join(str(int(v)) for v in meta) + '\n')
            for row in np.asarray(pose, np.float64):
                f.write('\t'.join(f'{v:.17g}' for v in row) + '\n')


# ---- KITTI velodyne scans -----------------------------------------------------------------------------
def read_kitti_bin(filename):
    """dataloader/kitti_loader.py:132-137: float32 records (x, y, z, reflectance); returns xyz [N,3] float32."""
    raw = np.fromfile(filename, dtype=np.float32)
    if raw.size % 4:
        raise ValueError(f'{filename}: size is not a multiple of 4 floats')
    return raw.reshape(-1, 4)[:, :3].copy()


def write_kitti_bin(filename, xyz, reflectance=None):
    xyz = np.asarray(xyz, np.float32)
    r = np.zeros(len(xyz), np.float32) if reflectance is None else np.asarray(reflectance, np.float32)
    np.concatenate([xyz, r[:, None]], 1).astype(np.float32).tofile(filename)


# ---- PLY ------------------------------------------------------------------------------------------------
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2',
              'ushort': 'u2', 'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4',
              'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply(filename):
    """Vertex positions [N,3] float64 of an ASCII or binary PLY (what `np.asarray(o3d.io.read_point_cloud(f)
    .points)` returns).  Other vertex properties and other elements are skipped; list properties are only
    supported on elements after `vertex` (e.g. faces), which are not read."""
    with open(filename, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError(f'{filename}: not a PLY file')
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f'{filename}: unterminated PLY header')
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] == 'comment' or tok[0] == 'obj_info':
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == 'property':
                elements[-1][2].append(tok[1:])
            elif tok[0] == 'end_header':
                break
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise ValueError(f'{filename}: unsupported PLY format {fmt}')
        if not elements or elements[0][0] != 'vertex':
            raise ValueError(f'{filename}: the first element must be "vertex"')
        _, n, props = elements[0]
        if any(p[0] == 'list' for p in props):
            raise ValueError(f'{filename}: list properties on vertices are not supported')
        names = [p[1] for p in props]
        if not all(k in names for k in 'xyz'):
            raise ValueError(f'{filename}: vertex element has no x/y/z')
        if fmt == 'ascii':
            rows = [f.readline().split() for _ in range(n)]
            data = np.array(rows, dtype=np.float64).reshape(n, len(names)) if n else np.zeros((0, len(names)))
            return np.stack([data[:, names.index(k)] for k in 'xyz'], 1)
        order = '<' if fmt == 'binary_little_endian' else '>'
        dt = np.dtype([(p[1], order + _PLY_TYPES[p[0]]) for p in props])
        data = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
        return np.stack([data[k].astype(np.float64) for k in 'xyz'], 1)


def write_ply(filename, xyz, binary=True):
    xyz = np.asarray(xyz, np.float64)
    with open(filename, 'wb') as f:
        f.write(b'ply\nformat ' + (b'binary_little_endian' if binary else b'ascii') + b' 1.0\n')
        f.write(f'element vertex {len(xyz)}\nproperty double x\nproperty double y\nproperty double z\nend_header\n'.encode())
        if binary:
            f.write(xyz.astype('<f8').tobytes())
        else:
            for p in xyz:
                f.write(f'{p[0]:.17g} {p[1]:.17g} {p[2]:.17g}\n'.encode())


def write_ply_mesh(filename, xyz, triangles, normals=None, binary=True):
    """A triangle mesh as PLY: vertices double x y z (then double nx ny nz with `normals`), faces as `property list uchar
    int vertex_indices`.  The vertex block is what `write_ply` writes, so `read_ply` returns the same points."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    tri = np.asarray(triangles).reshape(-1, 3)
    if tri.dtype.kind not in 'iu':
        raise ValueError(f'triangles must be integers, got {tri.dtype}')
    if len(tri) and (tri.min() < 0 or tri.max() >= len(xyz)):
        raise ValueError(f'a triangle names a vertex outside [0, {len(xyz)})')
    cols = [xyz]
    if normals is not None:
        normals = np.asarray(normals, np.float64).reshape(-1, 3)
        if normals.shape != xyz.shape:
            raise ValueError(f'normals {normals.shape} do not match the vertices {xyz.shape}')
        cols.append(normals)
    rows = np.concatenate(cols, 1)
    names = ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if normals is not None else [])
    with open(filename, 'wb') as f:
        f.write(b'ply\nformat ' + (b'binary_little_endian' if binary else b'ascii') + b' 1.0\n')
        f.write(f'element vertex {len(xyz)}\n'.encode() + ''.join(f'property double {k}\n' for k in names).encode())
        f.write(f'element face {len(tri)}\nproperty list uchar int vertex_indices\nend_header\n'.encode())
        if binary:
            f.write(rows.astype('<f8').tobytes())
            faces = np.empty(len(tri), np.dtype([('n', 'u1'), ('v', '<i4', 3)]))
            faces['n'], faces['v'] = 3, tri
            f.write(faces.tobytes())
        else:
            for r in rows:
                f.write((' '.join(f'{v:.17g}' for v in r) + '\n').encode())
            for t in tri:
                f.write(f'3 {t[0]} {t[1]} {t[2]}\n'.encode())


def read_ply_mesh(filename):
    """dict(xyz float64 [N,3], triangles int32 [T,3][, normals float64 [N,3]]) of an ASCII or binary PLY whose elements
    are `vertex` (scalar properties) and then `face` (one list property of three indices per face)."""
    with open(filename, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError(f'{filename}: not a PLY file')
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f'{filename}: unterminated PLY header')
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == 'property':
                elements[-1][2].append(tok[1:])
            elif tok[0] == 'end_header':
                break
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise ValueError(f'{filename}: unsupported PLY format {fmt}')
        if [e[0] for e in elements[:2]] != ['vertex', 'face']:
            raise ValueError(f'{filename}: expected the elements "vertex" and "face"')
        (_, n, props), (_, nf, fprops) = elements[:2]
        if any(p[0] == 'list' for p in props):
            raise ValueError(f'{filename}: list properties on vertices are not supported')
        if len(fprops) != 1 or fprops[0][0] != 'list':
            raise ValueError(f'{filename}: a face must be one list property')
        names = [p[1] for p in props]
        if not all(k in names for k in 'xyz'):
            raise ValueError(f'{filename}: vertex element has no x/y/z')
        if fmt == 'ascii':
            rows = [f.readline().split() for _ in range(n)]
            data = np.array(rows, dtype=np.float64).reshape(n, len(names))
            col = {k: data[:, i] for i, k in enumerate(names)}
            faces = [f.readline().split() for _ in range(nf)]
            if any(len(r) != 4 or r[0] != b'3' for r in faces):
                raise ValueError(f'{filename}: only triangles are supported')
            tri = np.array(faces, dtype=np.int64).reshape(nf, 4)[:, 1:].astype(np.int32)
        else:
            order = '<' if fmt == 'binary_little_endian' else '>'
            dt = np.dtype([(p[1], order + _PLY_TYPES[p[0]]) for p in props])
            data = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
            col = {k: data[k].astype(np.float64) for k in names}
            ft = np.dtype([('n', order + _PLY_TYPES[fprops[0][1]]), ('v', order + _PLY_TYPES[fprops[0][2]], 3)])
            faces = np.frombuffer(f.read(ft.itemsize * nf), dtype=ft, count=nf)
            if (faces['n'] != 3).any():
                raise ValueError(f'{filename}: only triangles are supported')
            tri = faces['v'].astype(np.int32).reshape(nf, 3)
    out = {'xyz': np.stack([col[k] for k in 'xyz'], 1), 'triangles': tri}
    if all(k in col for k in ('nx', 'ny', 'nz')):
        out['normals'] = np.stack([col[k] for k in ('nx', 'ny', 'nz')], 1)
    return out


def load_cloud(filename):
    """xyz [N,3] from .ply / .bin (KITTI) / .npy / .npz (key 'pcd' like the reference's 3DMatch pairs, else
    'xyz' or the first array) / .txt."""
    ext = os.path.splitext(filename)[1].lower()
    if ext == '.ply':
        return read_ply(filename)
    if ext == '.bin':
        return read_kitti_bin(filename)
    if ext == '.npy':
        return np.load(filename)[:, :3]
    if ext == '.npz':
        z = np.load(filename)
        key = 'pcd' if 'pcd' in z.files else ('xyz' if 'xyz' in z.files else z.files[0])
        return z[key][:, :3]
    if ext in ('.txt', '.xyz'):
        return np.loadtxt(filename)[:, :3]
    raise ValueError(f'unrecognised point-cloud file type: {filename}')


# ---- PNG (grayscale depth images) -----------------------------------------------------------------------
_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _png_chunk(tag, data):
    import zlib
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def write_png_gray16(filename, image, filter_type=0):
    """A [H,W] uint16 image as a 16-bit grayscale PNG (the 3DMatch depth format; stdlib zlib only).  Every scanline is
    written with `filter_type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth); readers must accept all five."""
    import zlib
    img = np.asarray(image)
    if img.ndim != 2 or img.dtype != np.uint16:
        raise ValueError(f'expected a [H,W] uint16 image, got {img.dtype} {img.shape}')
    if filter_type not in (0, 1, 2, 3, 4):
        raise ValueError(f'PNG filter type {filter_type}')
    h, w = img.shape
    raw = img.astype('>u2').view(np.uint8).reshape(h, w * 2).astype(np.int32)
    bpp = 2
    left = np.zeros_like(raw)
    left[:, bpp:] = raw[:, :-bpp]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    upleft = np.zeros_like(raw)
    upleft[1:, bpp:] = raw[:-1, :-bpp]
    if filter_type == 0:
        pred = 0
    elif filter_type == 1:
        pred = left
    elif filter_type == 2:
        pred = up
    elif filter_type == 3:
        pred = (left + up) // 2
    else:
        p = left + up - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    rows = np.empty((h, 1 + w * 2), np.uint8)
    rows[:, 0] = filter_type
    rows[:, 1:] = ((raw - pred) & 0xff).astype(np.uint8)
    with open(filename, 'wb') as f:
        f.write(_PNG_MAGIC)
        f.write(_png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16, 0, 0, 0, 0)))
        f.write(_png_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b'IEND', b''))


def read_png_gray(filename):
    """A non-interlaced grayscale PNG of 8 or 16 bits as [H,W] uint8 / uint16 (what `o3d.io.read_image` gives for a
    depth file), all five scanline filters.  Other colour types, bit depths and interlacing raise ValueError."""
    import zlib
    with open(filename, 'rb') as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f'{filename}: not a PNG file')
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n:
            raise ValueError(f'{filename}: truncated PNG chunk')
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat.append(body)
        elif tag == b'IEND':
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError(f'{filename}: PNG without IHDR')
    w, h, depth, colour, comp, filt, interlace = hdr
    if colour != 0 or depth not in (8, 16) or interlace != 0 or comp != 0 or filt != 0:
        raise ValueError(f'{filename}: only non-interlaced 8/16-bit grayscale PNG is supported '
                         f'(colour type {colour}, bit depth {depth}, interlace {interlace})')
    bpp = depth // 8
    stride = w * bpp
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8)
    if raw.size != h * (stride + 1):
        raise ValueError(f'{filename}: PNG image data has {raw.size} bytes, expected {h * (stride + 1)}')
    raw = raw.reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft = int(raw[y, 0])
        line = raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 0xff
        elif ft == 1:       # Sub: a running sum per byte lane
            cur = line.copy()
            for b in range(bpp):
                cur[b::bpp] = np.cumsum(line[b::bpp]) & 0xff
        elif ft in (3, 4):  # Average / Paeth depend on the reconstructed left neighbour: sequential
            cur = np.zeros(stride, np.int32)
            ln, pv = line.tolist(), prev.tolist()
            c = [0] * stride
            for i in range(stride):
                a = c[i - bpp] if i >= bpp else 0
                b_ = pv[i]
                if ft == 3:
                    pr = (a + b_) >> 1
                else:
                    cc = pv[i - bpp] if i >= bpp else 0
                    p = a + b_ - cc
                    pa, pb, pc = abs(p - a), abs(p - b_), abs(p - cc)
                    pr = a if (pa <= pb and pa <= pc) else (b_ if pb <= pc else cc)
                c[i] = (ln[i] + pr) & 0xff
            cur = np.array(c, np.int32)
        else:
            raise ValueError(f'{filename}: PNG filter type {ft}')
        out[y] = cur.astype(np.uint8)
        prev = cur
    if depth == 8:
        return out
    return out.view('>u2').astype(np.uint16).reshape(h, w)
