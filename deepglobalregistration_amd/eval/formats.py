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


def read_ply(filename, *, return_colors=False):
    """Vertex positions [N,3] float64 of an ASCII or binary PLY (what `np.asarray(o3d.io.read_point_cloud(f)
    .points)` returns).  Other vertex properties and other elements are skipped; list properties are only
    supported on elements after `vertex` (e.g. faces), which are not read.  With `return_colors` the pair (positions,
    colours uint8 [N,3] of the properties red, green, blue, or None when the file has none)."""
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
            col = {k: data[:, i] for i, k in enumerate(names)}
        else:
            order = '<' if fmt == 'binary_little_endian' else '>'
            dt = np.dtype([(p[1], order + _PLY_TYPES[p[0]]) for p in props])
            data = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
            col = {k: data[k] for k in names}
        xyz = np.stack([col[k].astype(np.float64) for k in 'xyz'], 1)
        return (xyz, _ply_colors(col)) if return_colors else xyz


_PLY_RGB = ('red', 'green', 'blue')


def _ply_colors(col):
    """uint8 [N,3] of a vertex element's columns red, green, blue; None without them"""
    if not all(k in col for k in _PLY_RGB):
        return None
    return np.stack([np.asarray(col[k]).astype(np.uint8) for k in _PLY_RGB], 1)


def _ply_vertex_block(cols, colors, binary):
    """(header lines, bytes) of a vertex element: the float64 columns `cols` ([N,k] with their k names) as `property
    double`, then -- with `colors` float [N,3] in [0, 1] -- `property uchar` red, green, blue (Open3D's order: positions,
    normals, colours), the byte clip(rint(255 c), 0, 255)."""
    rows, names = cols
    header = ''.join(f'property double {k}\n' for k in names)
    if colors is None:
        if binary:
            return header, rows.astype('<f8').tobytes()
        return header, b''.join((' '.join(f'{v:.17g}' for v in r) + '\n').encode() for r in rows)
    colors = np.asarray(colors, np.float64).reshape(-1, 3)
    if len(colors) != len(rows):
        raise ValueError(f'colors {colors.shape} do not match the {len(rows)} vertices')
    rgb = np.clip(np.rint(255.0 * colors), 0, 255).astype(np.uint8)
    header += ''.join(f'property uchar {k}\n' for k in _PLY_RGB)
    if binary:
        rec = np.empty(len(rows), np.dtype([('v', '<f8', len(names)), ('c', 'u1', 3)]))
        rec['v'], rec['c'] = rows, rgb
        return header, rec.tobytes()
    return header, b''.join((' '.join(f'{v:.17g}' for v in r) + f' {c[0]} {c[1]} {c[2]}\n').encode() for r, c in zip(rows, rgb))


def write_ply(filename, xyz, binary=True, colors=None):
    """Points as PLY: double x y z, with `colors` (float [N,3] in [0, 1]) then uchar red green blue."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    props, body = _ply_vertex_block((xyz, ['x', 'y', 'z']), colors, binary)
    with open(filename, 'wb') as f:
        f.write(b'ply\nformat ' + (b'binary_little_endian' if binary else b'ascii') + b' 1.0\n')
        f.write(f'element vertex {len(xyz)}\n{props}end_header\n'.encode())
        f.write(body)


def write_ply_mesh(filename, xyz, triangles, normals=None, binary=True, colors=None):
    """A triangle mesh as PLY: vertices double x y z (then double nx ny nz with `normals`, then uchar red green blue with
    `colors`, float [N,3] in [0, 1]), faces as `property list uchar int vertex_indices`.  The vertex block is what
    `write_ply` writes, so `read_ply` returns the same points."""
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
    props, body = _ply_vertex_block((rows, names), colors, binary)
    with open(filename, 'wb') as f:
        f.write(b'ply\nformat ' + (b'binary_little_endian' if binary else b'ascii') + b' 1.0\n')
        f.write(f'element vertex {len(xyz)}\n{props}'.encode())
        f.write(f'element face {len(tri)}\nproperty list uchar int vertex_indices\nend_header\n'.encode())
        f.write(body)
        if binary:
            faces = np.empty(len(tri), np.dtype([('n', 'u1'), ('v', '<i4', 3)]))
            faces['n'], faces['v'] = 3, tri
            f.write(faces.tobytes())
        else:
            for t in tri:
                f.write(f'3 {t[0]} {t[1]} {t[2]}\n'.encode())


def read_ply_mesh(filename):
    """dict(xyz float64 [N,3], triangles int32 [T,3][, normals float64 [N,3]][, colors uint8 [N,3]]) of an ASCII or binary
    PLY whose elements are `vertex` (scalar properties) and then `face` (one list property of three indices per face)."""
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
            col = {k: data[k] for k in names}
            ft = np.dtype([('n', order + _PLY_TYPES[fprops[0][1]]), ('v', order + _PLY_TYPES[fprops[0][2]], 3)])
            faces = np.frombuffer(f.read(ft.itemsize * nf), dtype=ft, count=nf)
            if (faces['n'] != 3).any():
                raise ValueError(f'{filename}: only triangles are supported')
            tri = faces['v'].astype(np.int32).reshape(nf, 3)
    out = {'xyz': np.stack([col[k].astype(np.float64) for k in 'xyz'], 1), 'triangles': tri}
    if all(k in col for k in ('nx', 'ny', 'nz')):
        out['normals'] = np.stack([col[k].astype(np.float64) for k in ('nx', 'ny', 'nz')], 1)
    colors = _ply_colors(col)
    if colors is not None:
        out['colors'] = colors
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


# ---- PNG (grayscale depth images, RGB colour images) -----------------------------------------------------
_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _png_chunk(tag, data):
    import zlib
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def _png_write(filename, raw, bpp, width, bit_depth, colour, filter_type):
    """`raw` uint8 [H, W bpp], the image's bytes as PNG orders them, as a non-interlaced PNG of one IDAT chunk whose every
    scanline is written with `filter_type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; stdlib zlib only)."""
    import zlib
    if filter_type not in (0, 1, 2, 3, 4):
        raise ValueError(f'PNG filter type {filter_type}')
    raw = raw.astype(np.int32)
    h = len(raw)
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
    rows = np.empty((h, 1 + raw.shape[1]), np.uint8)
    rows[:, 0] = filter_type
    rows[:, 1:] = ((raw - pred) & 0xff).astype(np.uint8)
    with open(filename, 'wb') as f:
        f.write(_PNG_MAGIC)
        f.write(_png_chunk(b'IHDR', struct.pack('>IIBBBBB', width, h, bit_depth, colour, 0, 0, 0)))
        f.write(_png_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)))
        f.write(_png_chunk(b'IEND', b''))


def write_png_gray16(filename, image, filter_type=0):
    """A [H,W] uint16 image as a 16-bit grayscale PNG (the 3DMatch depth format; stdlib zlib only).  Every scanline is
    written with `filter_type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth); readers must accept all five."""
    img = np.asarray(image)
    if img.ndim != 2 or img.dtype != np.uint16:
        raise ValueError(f'expected a [H,W] uint16 image, got {img.dtype} {img.shape}')
    h, w = img.shape
    _png_write(filename, img.astype('>u2').view(np.uint8).reshape(h, w * 2), 2, w, 16, 0, filter_type)


def write_png_rgb8(filename, image, filter_type=0):
    """A [H,W,3] uint8 image (R, G, B) as an 8-bit RGB PNG (colour type 2: the 3DMatch colour format), every scanline
    written with `filter_type` as in `write_png_gray16`."""
    img = np.asarray(image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f'expected a [H,W,3] uint8 image, got {img.dtype} {img.shape}')
    h, w = img.shape[:2]
    _png_write(filename, np.ascontiguousarray(img).reshape(h, w * 3), 3, w, 8, 2, filter_type)


def _png_scanlines(filename, bytes_per_pixel, supported):
    """(width, height, bit depth, colour type, uint8 [H, W bpp]: the unfiltered scanlines) of a non-interlaced PNG.
    `bytes_per_pixel` maps the (colour type, bit depth) pairs the caller reads to their bpp; `supported` names them in the
    ValueError every other PNG gets.  All five scanline filters."""
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
    if (colour, depth) not in bytes_per_pixel or interlace != 0 or comp != 0 or filt != 0:
        raise ValueError(f'{filename}: only {supported} is supported '
                         f'(colour type {colour}, bit depth {depth}, interlace {interlace})')
    bpp = bytes_per_pixel[(colour, depth)]
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
    return w, h, depth, colour, out


def read_png_gray(filename):
    """A non-interlaced grayscale PNG of 8 or 16 bits as [H,W] uint8 / uint16 (what `o3d.io.read_image` gives for a
    depth file), all five scanline filters.  Other colour types, bit depths and interlacing raise ValueError."""
    w, h, depth, _, out = _png_scanlines(filename, {(0, 8): 1, (0, 16): 2}, 'non-interlaced 8/16-bit grayscale PNG')
    if depth == 8:
        return out
    return out.view('>u2').astype(np.uint16).reshape(h, w)


def read_png_rgb8(filename):
    """A non-interlaced 8-bit PNG of colour type 2 (RGB) or 6 (RGBA, the alpha dropped) as [H,W,3] uint8 (what
    `o3d.io.read_image` gives for a 3DMatch colour file), all five scanline filters.  Anything else raises ValueError."""
    w, h, _, colour, out = _png_scanlines(filename, {(2, 8): 3, (6, 8): 4}, 'non-interlaced 8-bit RGB / RGBA PNG')
    return np.ascontiguousarray(out.reshape(h, w, 4 if colour == 6 else 3)[:, :, :3])
