"""`core/correspondence.py` of the reference: the correctness label of every putative match, on the GPU."""
import numpy as np
import torch

from .. import ops


def find_correct_correspondence(pos_pairs, pred_pairs, hash_seed=None, len_batch=None):
    """core/correspondence.py:29-53.  `pos_pairs` / `pred_pairs`: one [P,2] / [Q,2] integer array or tensor per batch
    entry.  Returns a numpy bool array over the concatenated predicted pairs: True where the pair's key
    i + j * seed occurs among the keys of the entry's positive pairs (seed = `hash_seed`, or max(N0, N1) of `len_batch`;
    a small seed collides exactly as the reference's `_hash` does)."""
    assert len(pos_pairs) == len(pred_pairs)
    if hash_seed is None:
        assert len(len_batch) == len(pos_pairs)
    if len(pos_pairs) == 0:
        return np.zeros(0, bool)
    seeds = [max(int(n) for n in len_batch[i]) if hash_seed is None else int(hash_seed) for i in range(len(pos_pairs))]
    dev = next((t.device for t in list(pred_pairs) + list(pos_pairs) if torch.is_tensor(t) and t.is_cuda),
               torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None)
    if dev is None:
        raise RuntimeError('find_correct_correspondence runs on the GPU only; there is no CPU fallback')

    def cat(parts):
        parts = [torch.as_tensor(np.asarray(p) if not torch.is_tensor(p) else p).reshape(-1, 2).to(dev, torch.int64)
                 for p in parts]
        return torch.cat(parts), np.cumsum([0] + [len(p) for p in parts])
    pos, pos_off = cat(pos_pairs)
    pred, pred_off = cat(pred_pairs)
    return ops.pairs_isin(pos, pos_off, pred, pred_off, seeds).cpu().numpy().astype(bool)
