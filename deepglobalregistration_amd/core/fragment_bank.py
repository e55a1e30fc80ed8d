"""The fragments of a scene, voxelised and featurised once: what `DeepGlobalRegistration.extract_fragments` returns and
`DeepGlobalRegistration.register_pairs` registers any list of (i, j) pairs from (no reference counterpart: the reference
voxelises and featurises both clouds of every pair again, scripts/test_3dmatch.py:108-111).

Layout: three row-aligned tensors on one device -- `coords` int32 [N,4] (batch column 0: the library writes the pair
index there when it copies a fragment into a batch), `xyz` f32 [N,3], `F` f32 [N,C] -- with fragment i in rows
off[i]:off[i+1]; `off` is a host int64 array.  The library holds no bank object: the tensors are torch's memory."""
import numpy as np
import torch

from .. import _args

FEATURE_WIDTHS = (16, 32, 64)   # the widths the feature matcher is built for (csrc/knn_common.h)


class FragmentBank:
    def __init__(self, coords, xyz, F, off):
        self.coords, self.xyz, self.F, self.off = coords, xyz, F, off

    @classmethod
    def from_tensors(cls, coords, xyz, F, off):
        """Checks shapes, dtypes, device, offsets (ascending from 0 to N, no empty fragment) and the feature width;
        ValueError otherwise.  Works on CPU tensors too (only `register_pairs` needs the GPU)."""
        for name, t, dtype, width in (('coords', coords, torch.int32, 4), ('xyz', xyz, torch.float32, 3),
                                      ('F', F, torch.float32, None)):
            if not torch.is_tensor(t):
                raise ValueError(f'{name} must be a torch tensor')
            if t.dtype != dtype:
                raise ValueError(f'{name} must be {dtype}, got {t.dtype}')
            if t.dim() != 2 or (width is not None and t.shape[1] != width):
                raise ValueError(f'{name} must be [N,{width if width else "C"}], got {tuple(t.shape)}')
        if F.shape[1] not in FEATURE_WIDTHS:
            raise ValueError(f'feature width {F.shape[1]} is not one of {FEATURE_WIDTHS}')
        if not (len(coords) == len(xyz) == len(F)):
            raise ValueError('coords, xyz and F must have the same number of rows')
        if not (coords.device == xyz.device == F.device):
            raise ValueError('coords, xyz and F must be on one device')
        # (not _args.fragment_offsets: a bank's offsets start at 0 exactly, and the two faults have messages of their own)
        off = np.asarray(off.cpu() if torch.is_tensor(off) else off)
        if off.ndim != 1 or len(off) < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError('off must be a 1-D integer array [nfrag+1]')
        off = off.astype(np.int64)
        if off[0] != 0 or off[-1] != len(coords):
            raise ValueError(f'off must run from 0 to the row count {len(coords)}')
        if (np.diff(off) <= 0).any():
            raise ValueError('off must ascend strictly (no empty fragment)')
        return cls(coords.contiguous(), xyz.contiguous(), F.contiguous(), off)

    def __len__(self):
        return len(self.off) - 1

    @property
    def device(self):
        return self.F.device

    @property
    def n_out(self):
        return int(self.F.shape[1])

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.coords, self.xyz, self.F)) + self.off.nbytes

    def rows(self, i):
        """The rows of fragment i as a slice."""
        i = range(len(self))[i]
        return slice(int(self.off[i]), int(self.off[i + 1]))

    def coords_of(self, i):
        return self.coords[self.rows(i)]

    def xyz_of(self, i):
        return self.xyz[self.rows(i)]

    def features_of(self, i):
        return self.F[self.rows(i)]


def pair_groups(bank, pairs, batch_pairs):
    """`pairs` ([n,2] integers) checked against the bank and cut into consecutive groups of `batch_pairs` in the given
    order: a list of (first pair index, ids int32 [g,2]).  ValueError for an empty list or an id outside the bank."""
    ids = _args.pair_ids(np.asarray(pairs), len(bank), 'pairs')   # (np.asarray: a device tensor is not taken here)
    if int(batch_pairs) < 1:
        raise ValueError('batch_pairs must be at least 1')
    return [(k, ids[k:k + int(batch_pairs)]) for k in range(0, len(ids), int(batch_pairs))]


def group_hooks(bank, first, ids, forced_logits, override_idx1, device):
    """The two test hooks of one group in the batch's numbering.  Both come per pair: forced_logits[k] has one value per
    row of pair k's fragment 0 and is concatenated; override_idx1[k] holds rows of pair k's fragment 1 (-1 = keep the
    match) and is shifted by where that fragment starts in the group's concatenated fragment 1."""
    n0 = bank.off[ids[:, 0] + 1] - bank.off[ids[:, 0]]
    n1 = bank.off[ids[:, 1] + 1] - bank.off[ids[:, 1]]
    start1 = np.concatenate(([0], np.cumsum(n1)))

    def per_pair(seq, name, p):
        t = seq[first + p]
        t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
        t = t.to(device).reshape(-1)
        if len(t) != n0[p]:
            raise ValueError(f'{name}[{first + p}] has {len(t)} entries, fragment 0 of the pair has {n0[p]} rows')
        return t
    fl = ov = None
    if forced_logits is not None:
        fl = torch.cat([per_pair(forced_logits, 'forced_logits', p).float() for p in range(len(ids))])
    if override_idx1 is not None:
        parts = []
        for p in range(len(ids)):
            o = per_pair(override_idx1, 'override_idx1', p).long()
            if bool((o >= int(n1[p])).any()):
                raise ValueError(f'override_idx1[{first + p}] points past fragment 1 of the pair ({n1[p]} rows)')
            parts.append(torch.where(o >= 0, o + int(start1[p]), o))
        ov = torch.cat(parts)
    return fl, ov
