"""The argument vocabulary of the Python layer: one function per check that `ops` and `core` make in more than one place.
Every function works on host values alone (numpy and torch only): none loads the library or touches a device.  A check
that accepts other things or says other words than these stays where it is, with a note of what sets it apart."""
import numpy as np
import torch


def is_number(v):
    """A real number as an argument: a Python or numpy int / float, not a bool."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def positive_number(v, name):
    if not is_number(v) or not np.isfinite(v) or v <= 0:
        raise ValueError(f'{name} must be a positive finite number, got {v!r}')
    return float(v)


def integer(v, name, ok, what):
    """`v` as an int when it is a Python or numpy integer (not a bool) with ok(v); `what` says what ok asks for."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not ok(v):
        raise ValueError(f'{name} must be {what}, got {v!r}')
    return int(v)


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def rows(a, width, name):
    """The row count of an [N,width] array or tensor."""
    shape = tuple(a.shape) if hasattr(a, 'shape') else np.asarray(a).shape
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f'{name} must be [N,{width}], got {shape}')
    return shape[0]


def pair_offsets(off, name, total=None):
    """int64 [npairs+1] row offsets of a batch of pairs: from 0, not decreasing (a pair may be empty), to `total`."""
    o = np.ascontiguousarray(np.asarray(off), dtype=np.int64).reshape(-1)
    if len(o) < 2 or o[0] != 0 or bool((np.diff(o) < 0).any()):
        raise ValueError(f'{name} must be [npairs+1] row offsets that start at 0 and do not decrease')
    if total is not None and o[-1] != total:
        raise ValueError(f'{name} ends at {int(o[-1])}, the array has {int(total)} rows')
    return o


def fragment_offsets(off, n_rows, name):
    """int64 [nfrag+1] row offsets of a bank's fragments: integers, ascending strictly from >= 0 to `n_rows`."""
    off = np.asarray(off.cpu() if torch.is_tensor(off) else off)
    if off.ndim != 1 or len(off) < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f'{name} must be a 1-D integer array [nfrag+1]')
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] < 0 or bool((np.diff(off) <= 0).any()) or off[-1] != n_rows:
        raise ValueError(f'{name} must ascend strictly (no empty fragment) from >= 0 to the row count {int(n_rows)}')
    return off


def pair_ids(ids, nfrag, name):
    """int32 [n,2] fragment ids of a non-empty pair list over a bank of `nfrag` fragments."""
    ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
    if ids.size == 0:
        raise ValueError('the pair list is empty')
    if ids.ndim != 2 or ids.shape[1] != 2 or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f'{name} must be an [n,2] integer array')
    if bool((ids < 0).any()) or bool((ids >= nfrag).any()):
        raise ValueError(f'pair id outside [0, {nfrag})')
    return np.ascontiguousarray(ids, dtype=np.int32)


def pose_stack(T, n, name, finite_rows):
    """float64 [n,16] from `n` poses [n,4,4] (one [4,4] stands for n = 1) whose first `finite_rows` rows (3: what the
    library reads; 4: all) are finite."""
    T = host(T)
    if T.shape == (4, 4) and n == 1:
        T = T[None]
    if T.shape != (n, 4, 4):
        raise ValueError(f'{name} must be [{n},4,4], got {T.shape}')
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(n, 16)
    if not np.isfinite(T[:, :4 * finite_rows]).all():
        raise ValueError(f'{name} must be finite' + ('' if finite_rows == 4 else ' (first three rows)'))
    return T
