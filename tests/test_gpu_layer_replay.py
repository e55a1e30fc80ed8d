"""The forward's run records and tensor registry, pinned from outside (in-process, no switch set).

  1. replay: `NetHandle.rerun_layer` launches a layer of the last forward again from its run record -- the same kernels on
     the same operands.  After every layer has been replayed once, every named tensor reads back with the same dtype,
     shape and bytes in every representation it had (and the same ones are still refused with "did not write").  The
     one layer that cannot be replayed is a conv1 fused with its neighbour search ("not re-runnable"); once another net
     object's forward has reused the context's workspace, every replay is refused ("gone").
  2. aliases: the seven names of `NetHandle.intermediate` are the registry's tensors under the model's names, as f32
     rows with the ReLU applied on the host; cloud D6 has coarse 6-D maps, whose rows come back renumbered.

Nets and clouds of tests/aux/layer_trace_inputs.py: the smallest that reach every row-block edge and every kernel kind
(fused conv1, small-Cin, rule-major f32, wide, output-stationary lists, dense tiles, parity-class up-conv, identity)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import layer_trace_inputs as inp   # noqa: E402
from layer_trace_dump import REPRS, TENSORS   # noqa: E402
from deepglobalregistration_amd import ops   # noqa: E402

pytestmark = pytest.mark.gpu
# (net, cloud, wide_coarse)
CASES = [('fcgf32', 'C', False), ('fcgf32', 'D', False), ('rule12', 'D', False), ('inl6', 'D6', False),
         ('inl1', 'D6', False), ('fcgf32', 'D', True)]
IDS = [f'{n}-{c}' + ('-wide_coarse' if w else '') for n, c, w in CASES]
ALIASES = {'s1': 'S1', 's2': 'S2', 's4': 'S4', 's8': 'S8', 's4_tr': 'S4T', 's2_tr': 'S2T', 's1_tr': 'S1T'}


def make_net(name, wide_coarse=False):
    D, cin, cout, ks, norm, _, _ = inp.NETS[name]
    return ops.NetHandle(inp.state_dict(name), D, cin, cout, ks, norm, wide_coarse=wide_coarse)


def run_forward(net, name, cloud):
    coords = inp.clouds()[cloud]
    return net.forward(torch.from_numpy(coords).cuda(), torch.from_numpy(inp.feats(name, cloud, len(coords))).cuda())


def read_all(net):
    """{'<tensor>/<repr>': array, or None where the forward did not write it}."""
    got = {}
    for t in TENSORS + ('OUT',):
        for r in REPRS:
            try:
                got[f'{t}/{r}'] = net.tensor(t, r)
            except (RuntimeError, ValueError) as e:
                if 'did not write' not in str(e):
                    raise
                got[f'{t}/{r}'] = None
    return got


@pytest.mark.parametrize('name,cloud,wide_coarse', CASES, ids=IDS)
def test_replaying_every_layer_changes_no_byte(name, cloud, wide_coarse):
    net = make_net(name, wide_coarse)
    run_forward(net, name, cloud)
    before = read_all(net)
    assert sum(v is not None for v in before.values()) >= len(TENSORS) + 1
    fused = inp.NETS[name][0] == 3 and inp.NETS[name][1] <= 8   # conv1 runs fused with its neighbour search
    refused = []
    for li in range(23):
        try:
            g, r = net.rerun_layer(li, 1)
            assert g >= 0 and r >= 0
        except (RuntimeError, ValueError) as e:
            assert 'not re-runnable' in str(e), (li, e)
            refused.append(li)
    assert refused == ([0] if fused else []), refused
    after = read_all(net)
    assert after.keys() == before.keys()
    for k, a in before.items():
        b = after[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    # another net object's forward reuses the context's workspace: the records point into memory that is gone
    run_forward(make_net(name, wide_coarse), name, cloud)
    for li in range(23):
        with pytest.raises((RuntimeError, ValueError), match='gone'):
            net.rerun_layer(li, 1)


@pytest.mark.parametrize('name,cloud,wide_coarse', CASES, ids=IDS)
def test_intermediates_are_the_named_tensors_after_relu(name, cloud, wide_coarse):
    net = make_net(name, wide_coarse)
    run_forward(net, name, cloud)
    for alias, t in ALIASES.items():
        got = net.intermediate(alias)
        want = np.maximum(net.tensor(t, 'f32'), np.float32(0))
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (alias, t)
