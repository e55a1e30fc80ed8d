"""Guard bands for the wrapper side of the poisoned-memory tests (tests/test_gpu_workspace_poison.py): pure torch, works
on CPU tensors too.

`guarded(t, word)` puts a tensor's values in the middle of a larger allocation whose every other byte holds the 32-bit
`word`; `Outputs(word)` makes `deepglobalregistration_amd.ops` allocate its outputs that way and checks, when it ends,
that nothing was written next to them.  An `empty` output holds the word too, so a row the library does not write changes
with the word."""
import sys

import numpy as np
import torch

BAND = 4096    # bytes on each side: a multiple of every vector width in use, far more than any tile tail
ALIGN = 256    # the view starts at a multiple of this (the workspace's own alignment)


class BandDamaged(AssertionError):
    pass


def _signed(word):
    word = int(word) & 0xffffffff
    return word - (1 << 32) if word >= 1 << 31 else word


def _pattern(word, start, length, device):
    """`length` bytes of the word's little-endian bytes, as they lie from byte `start` of a buffer filled with it."""
    b = np.frombuffer(np.uint32(int(word) & 0xffffffff).tobytes(), np.uint8)
    idx = (np.arange(length, dtype=np.int64) + start) % 4
    return torch.from_numpy(b[idx].copy()).to(device)


def _alloc(shape, dtype, device, word):
    """-> (view of `shape` / `dtype`, its whole allocation as bytes, byte offset of the view): every byte holds the word."""
    if isinstance(shape, (int, np.integer)):
        shape = (int(shape),)
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    total = BAND + ALIGN + nbytes + BAND
    words = torch.full(((total + 3) // 4,), _signed(word), dtype=torch.int32, device=device)
    raw = words.view(torch.uint8)
    off = BAND + (-(raw.data_ptr() + BAND)) % ALIGN
    assert off % item == 0 and off + nbytes + BAND <= raw.numel()
    view = raw[off:off + nbytes].view(dtype).reshape(shape)
    assert view.data_ptr() % ALIGN == 0 and view.is_contiguous()
    return view, raw, off


def guarded(t, word, keep=None):
    """A contiguous tensor with `t`'s values, dtype and shape that starts 256-byte aligned in the middle of a larger
    allocation: the BAND bytes before it and behind it (and the rest of the allocation) hold `word`.  `keep`: a list that
    receives what `check_inputs` needs to show later that nobody wrote to the input or next to it."""
    view, raw, off = _alloc(t.shape, t.dtype, t.device, word)
    view.copy_(t)
    if keep is not None:
        keep.append((raw, off, view.numel() * view.element_size(), raw[off:off + view.numel() * view.element_size()].clone()))
    return view


def check_inputs(keep, word, what=''):
    """Every input recorded in `keep` still holds its bytes and lies between intact bands; BandDamaged otherwise."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for raw, off, nbytes, was in keep:
        at = first_damage(raw, off, nbytes, word)
        if at is None and not torch.equal(raw[off:off + nbytes], was):
            at = int(torch.nonzero(raw[off:off + nbytes] != was)[0, 0])
        if at is not None:
            raise BandDamaged(f'{what}: an input of {nbytes} bytes was written to, first at byte offset {at} from its start '
                              f'(word {int(word) & 0xffffffff:08X})')


def first_damage(raw, off, nbytes, word):
    """Byte offset relative to the view's start (negative: in front of it; >= nbytes: behind it) of the first byte of
    the two bands that no longer holds the word, or None."""
    for start, base in ((off - BAND, -BAND), (off + nbytes, nbytes)):
        bad = raw[start:start + BAND] != _pattern(word, start, BAND, raw.device)
        if bool(bad.any()):
            return base + int(torch.nonzero(bad)[0, 0])
    return None


class _TorchProxy:
    """What `ops` sees as `torch` inside `Outputs`: torch itself, but for the allocators of outputs."""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        return getattr(torch, name)

    def _make(self, size, dtype, device, zero):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device('cpu')
        op = sys._getframe(2).f_code.co_name
        view, raw, off = _alloc(size, dtype, device, self._owner.word)
        if zero:
            view.zero_()
        self._owner.made.append((op, raw, off, view.numel() * view.element_size()))
        return view

    def empty(self, *size, dtype=None, device=None):
        return self._make(size, dtype, device, False)

    def zeros(self, *size, dtype=None, device=None):
        return self._make(size, dtype, device, True)

    def empty_like(self, t):
        return self._make((tuple(t.shape),), t.dtype, t.device, False)

    def zeros_like(self, t):
        return self._make((tuple(t.shape),), t.dtype, t.device, True)


class Outputs:
    """Context manager: inside it, every output `ops` allocates (torch.empty, empty_like, zeros, zeros_like -- as seen
    from `ops` only; torch itself is not patched) is a guarded view, `empty` ones holding the word, `zeros` ones zeros.
    On exit, after a device synchronise, every band must still hold the word: BandDamaged names the op that made the
    output and the first damaged byte offset relative to the output's start otherwise."""

    def __init__(self, word, module=None):
        self.word = int(word) & 0xffffffff
        self.made = []
        self._module = module

    def __enter__(self):
        if self._module is None:
            from deepglobalregistration_amd import ops
            self._module = ops
        self._saved = self._module.torch
        self._module.torch = _TorchProxy(self)
        return self

    def check(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        for op, raw, off, nbytes in self.made:
            at = first_damage(raw, off, nbytes, self.word)
            if at is not None:
                raise BandDamaged(f'{op}: an output of {nbytes} bytes has a damaged guard band, first at byte offset {at} '
                                  f'from its start (word {self.word:08X})')
        self.made = []

    def __exit__(self, exc_type, exc, tb):
        self._module.torch = self._saved
        if exc_type is None:
            self.check()
        return False
