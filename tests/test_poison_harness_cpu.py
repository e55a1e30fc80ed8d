"""The guard-band helper of the poisoned-memory tests (tests/aux/poison.py) on CPU tensors: what it must report when an
op is wrong in one of the three ways tests/test_gpu_workspace_poison.py looks for, and that a clean op passes."""
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import poison   # noqa: E402

WORDS = (0x00000000, 0x00000001, 0x7FC00000)


def fake_ops():
    """A stand-in for `ops`: a module with its own `torch` and four ops on [n, 3] float32 rows."""
    m = types.ModuleType('fake_ops')
    m.torch = torch

    def flat(t, extra=0):   # the memory of a contiguous tensor and `extra` elements behind it, as a kernel sees it
        return torch.as_strided(t, (t.numel() + extra,), (1,))

    def clean(x):
        out = m.torch.empty(x.shape, dtype=x.dtype, device=x.device)
        flat(out).copy_(flat(x) * 2)
        return out

    def overrun(x):
        out = m.torch.empty(x.shape, dtype=x.dtype, device=x.device)
        flat(out, 1)[:-1].copy_(flat(x) * 2)
        flat(out, 1)[-1] = 5.0          # one element past the output
        return out

    def overread(x):
        out = m.torch.zeros(x.shape, dtype=x.dtype, device=x.device)
        flat(out).copy_(flat(x, 1)[1:])   # a window that is off by one: its last element lies past the input
        return out

    def lazy(x):
        out = m.torch.empty_like(x)
        out[:-1] = x[:-1] * 2           # the last row is never written
        return out

    m.clean, m.overrun, m.overread, m.lazy = clean, overrun, overread, lazy
    return m


def run(m, op, word, x):
    with poison.Outputs(word, module=m):
        out = getattr(m, op)(poison.guarded(x, word))
    return out.clone()


def damaged_at(err):
    return int(re.search(r'byte offset (-?\d+) ', str(err)).group(1))


X = torch.arange(15, dtype=torch.float32).reshape(5, 3) + 1


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32, torch.float64])
@pytest.mark.parametrize('word', WORDS + (0xA1B2C3D4,))
def test_guarded_view_sits_aligned_between_bands_of_the_word(word, dtype):
    t = (torch.arange(63) % 7).to(dtype).reshape(21, 3)
    g = poison.guarded(t, word)
    assert g.dtype == t.dtype and g.shape == t.shape and g.is_contiguous() and torch.equal(g, t)
    assert g.data_ptr() % poison.ALIGN == 0
    item = g.element_size()
    around = torch.as_strided(g, (poison.BAND // item + g.numel() + poison.BAND // item,), (1,), g.storage_offset() - poison.BAND // item)
    raw = around.view(torch.uint8)
    n = g.numel() * item
    want = poison._pattern(word, 0, poison.BAND, 'cpu')   # the view starts at a multiple of 4 bytes of a filled buffer
    assert torch.equal(raw[:poison.BAND], want)
    # behind the view the word's phase continues from the view's end
    assert torch.equal(raw[poison.BAND + n:], poison._pattern(word, n, poison.BAND, 'cpu'))


def test_proxy_is_seen_from_the_module_only_and_restored():
    m = fake_ops()
    with poison.Outputs(1, module=m) as o:
        assert m.torch is not torch and m.torch.float32 is torch.float32
        z = m.torch.zeros(4, dtype=torch.int64)
        e = m.torch.empty((2, 3), dtype=torch.float32)
        assert torch.equal(z, torch.zeros(4, dtype=torch.int64))
        assert e.view(torch.int32).eq(1).all()          # an output nobody wrote holds the word
        assert len(o.made) == 2
        assert torch.empty(3).data_ptr() % 4 == 0       # torch itself is untouched
    assert m.torch is torch


@pytest.mark.parametrize('word', WORDS)
def test_clean_op_passes_with_the_same_bits(word):
    assert torch.equal(run(fake_ops(), 'clean', word, X), X * 2)


@pytest.mark.parametrize('word', WORDS)
def test_overrun_of_one_element_is_reported(word):
    with pytest.raises(poison.BandDamaged) as e:
        run(fake_ops(), 'overrun', word, X)
    # (the first byte of the stray element that differs from the word's: within the element)
    assert 'overrun' in str(e.value) and 0 <= damaged_at(e.value) - X.numel() * 4 < 4


def test_overrun_in_front_is_reported_with_a_negative_offset():
    m = fake_ops()
    with pytest.raises(poison.BandDamaged) as e:
        with poison.Outputs(0, module=m):
            out = m.torch.empty(8, dtype=torch.float32)
            torch.as_strided(out, (1,), (1,), out.storage_offset() - 1)[0] = 1.0
    assert -4 <= damaged_at(e.value) < 0


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize('op', ['overread', 'lazy'])
def test_read_past_the_input_and_unwritten_row_change_with_the_word(op):
    m = fake_ops()
    r0, r1, r2 = (run(m, op, w, X) for w in WORDS)
    assert not same_bytes(r0, r1)        # 0 against a denormal / the integer 1
    assert not same_bytes(r0, r2) and bool(torch.isnan(r2).any())
    # ... and only where the op is wrong
    assert same_bytes(r0[:-1], r1[:-1]) and same_bytes(r0[:-1], r2[:-1])
    assert same_bytes(r0[-1, :2], r2[-1, :2]) or op == 'lazy'


def test_clean_op_is_the_same_at_every_word():
    m = fake_ops()
    r = [run(m, 'clean', w, X) for w in WORDS]
    assert same_bytes(r[0], r[1]) and same_bytes(r[0], r[2])


def test_write_to_an_input_or_next_to_it_is_reported():
    keep = []
    g = poison.guarded(X, 1, keep)
    poison.check_inputs(keep, 1)
    g[2, 1] += 1                          # an op that writes to its input
    with pytest.raises(poison.BandDamaged) as e:
        poison.check_inputs(keep, 1, 'fam')
    assert 'fam' in str(e.value) and 28 <= damaged_at(e.value) < 32
    keep = []
    g = poison.guarded(X, 1, keep)
    torch.as_strided(g, (1,), (1,), g.storage_offset() + g.numel())[0] = 3.0
    with pytest.raises(poison.BandDamaged) as e:
        poison.check_inputs(keep, 1)
    assert 0 <= damaged_at(e.value) - X.numel() * 4 < 4
