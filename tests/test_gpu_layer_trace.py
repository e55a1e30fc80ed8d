"""Every conv layer of both nets, in isolation, per element, against float64 -- from the input the device itself fed it.

A forward leaves every named tensor in the workspace (`NetHandle.tensor`, dgr_net_get_tensor): f32 rows, the `amax`
words, the 6-D split rows, the 3-D dense split rows.  Per arithmetic mode (one process each: default, DGR_OS_LISTS=1,
DGR_EXACT_F32=1), net and cloud of tests/aux/layer_trace_inputs.py, and for each of the 23 layers:

  (a) the layer's input as the device holds it (f32 rows; the decoded pieces where a block's middle tensor exists as
      pieces only -- exactly what the consumer multiplies) goes through `layer_trace_ref.unit_truth` in float64; the
      device's output must satisfy |y - y64| <= c B for ALL elements, B = |shift| + sum |x||W| + |res|.  An output that
      exists as pieces only is compared after decoding, with 2^-22 rowmax added.
  (b) the hand-overs, exactly: amax[row] = integer max of the bits of max(x, 0) / |x| (over both halves for the
      concatenations); 6-D planes and scales = split2 of the f32 rows under row_scale_of, bit for bit; dense split rows
      are the split of their own decoded value and their scale matches amax.
  (c) which kernel family ran each layer (ops.conv_launch_kinds).

The constant c is not taken from the kernels.  Yardstick: e32 = the largest |y32 - y64| / B of the reference's own
float32 arithmetic (oracle.resunet.sparse_conv + batch_norm) on the same unit and input.  Margins: x 1.5 for another
summation order (the allowance of test_gpu_split_f64.py); + 2^-21 in the split modes (two operand roundings of 2^-23
each, plus the dropped m m product of at most 2^-22); + 2^-23 in exact-f32 mode (the f32 rounding of the folded weight).

About the dense-split check of (b): "re-split gives the same bytes" holds up to two cases that are the same split
(layer_trace_ref.resplit_mismatches): a residual piece that underflowed to a zero of either sign, and an exact
round-to-nearest tie in h, which the re-split sees from the other side.  Everything else must match.

The measured maxima go to <DGR_PARITY_REPORT>/layer_trace_vs_f64.txt (committed as profiles/layer_trace_vs_f64.txt),
with the report-only lines of the wide-range checkpoint (folded batch-norm scales over eight decades).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'aux'))
import layer_trace_inputs as inp   # noqa: E402
import layer_trace_ref as ref   # noqa: E402
from oracle import resunet as oresunet   # noqa: E402

pytestmark = pytest.mark.gpu
MODES = {'split': {}, 'os_lists': {'DGR_OS_LISTS': '1'}, 'exact_f32': {'DGR_EXACT_F32': '1'}}
MODE_ENV = ('DGR_EXACT_F32', 'DGR_OS_LISTS', 'DGR_NO_UP', 'DGR_NO_DSPLIT', 'DGR_OS_MB01', 'DGR_OS_MB2', 'DGR_OS_MB3', 'DGR_OS_CK')
ADD = {'split': 2.0 ** -21, 'os_lists': 2.0 ** -21, 'exact_f32': 2.0 ** -23}
_lines = []
_maps = {}


def report(line):
    print(line)
    _lines.append(line)


@pytest.fixture(scope='module')
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp('layer_trace')
    out = {}
    for mode, env in MODES.items():
        e = {k: v for k, v in os.environ.items() if k not in MODE_ENV}
        e.update(env)
        for what in ('trace', 'wide'):
            path = str(d / f'{mode}_{what}.npz')
            subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'aux', 'layer_trace_dump.py'), path, what], env=e,
                           check=True, timeout=600)
            out[mode, what] = np.load(path)
    yield out
    rep = os.environ.get('DGR_PARITY_REPORT')
    if rep and _lines:
        os.makedirs(rep, exist_ok=True)
        with open(os.path.join(rep, 'layer_trace_vs_f64.txt'), 'w') as f:
            f.write('\n'.join(_lines) + '\n')


def maps_of(key, coords, D, ks):
    if key not in _maps:
        _maps[key] = oresunet.SparseMaps(coords, D, ks)
    return _maps[key]


class Forward:
    """One dumped forward: tensors by name in the representation the device holds."""

    def __init__(self, z, prefix, feats):
        self.z, self.p, self.feats = z, prefix, feats
        self.kinds = z[prefix + 'kinds'].tolist()
        self.missing = set(z[prefix + 'missing'].tolist())

    def has(self, name, r):
        return self.p + f'{name}/{r}' in self.z.files

    def get(self, name, r):
        return self.z[self.p + f'{name}/{r}']

    def value(self, name):
        """(float64 rows, 'f32' | 'split6' | 'dense'): the f32 rows, or the decoded pieces of a pieces-only tensor."""
        if name == 'X':
            return self.feats.astype(np.float64), 'f32'
        if self.has(name, 'f32'):
            return self.get(name, 'f32').astype(np.float64), 'f32'
        assert f'{name}/f32' in self.missing   # refused with "did not write", not absent for another reason
        if self.has(name, 'split_planes'):
            return ref.decode_split6(self.get(name, 'split_planes'), self.get(name, 'split_scale')), 'split6'
        return ref.decode_dense(self.get(name, 'dense_split'), self.get(name, 'amax')), 'dense'


OS_FAMILY = ('sparse_conv_os<', 'sparse_conv_dense_f16x2', 'sparse_conv_up_f16x2')


def expected_family(D, cin, mode, li, L, ci, co):
    """Kernel family of layer li (ci -> co channels) by net shape and mode: the dispatch of layer_kind (net.hip) as a table."""
    if L['map'] is None:
        return 'identity_conv_kernel'
    fused3 = D == 3 and cin <= 8
    if li == 0:
        return 'conv1_grid' if fused3 else 'sparse_conv_mfma_v2' if D == 3 else \
            'conv_cin6_quad_kernel' if cin == 6 else 'conv_small_cin_row_kernel'
    if fused3:
        if mode == 'exact_f32':
            return 'sparse_conv_os<'
        if mode == 'split' and L['map'][0] == 'same' and ci <= 64 and co <= 64:
            return 'sparse_conv_dense_f16x2'
        if mode == 'split' and L['map'][0] == 'up':
            return 'sparse_conv_up_f16x2'
        return 'sparse_conv_os<'
    if D == 6 and mode != 'exact_f32':
        wide = (co == 64 and ci == 64) or (co == 128 and ci in (64, 128, 256)) or (co == 256 and ci in (128, 256))
        if wide:
            return 'sparse_conv_wide_f16x2'
    return 'sparse_conv_mfma_v2'


def check_forward(mode, net, cloud, z, sd, coords, feats, D, cin, ks, norm, assert_bound=True):
    """-> per layer (kernel, worst |y - y64| / B, e32, c).  Asserts (a), (b), (c)."""
    fw = Forward(z, f'{net}/{cloud}/', feats)
    maps = maps_of((net, cloud), coords, D, ks)
    assert len(fw.kinds) == 23, fw.kinds
    rows = []
    split_mode = mode != 'exact_f32'
    for li, L in enumerate(ref.LAYERS):
        x, _ = fw.value(L['inp'])
        res = fw.value(L['res'])[0] if L['res'] else None
        normalize = norm and L['name'] == 'final'
        y64, B, e32 = ref.run_unit(maps, sd, L, x, res, normalize)
        kind = fw.kinds[li]
        # ---- (c)
        fam = expected_family(D, cin, mode, li, L, x.shape[1], y64.shape[1])
        if assert_bound:
            assert kind.startswith(fam), (mode, net, cloud, li, L['name'], kind, fam)
            if mode == 'os_lists':
                assert 'dense' not in kind and '_up_' not in kind
            if mode == 'exact_f32':
                assert 'f16x2' not in kind
        # ---- (a)
        y, how = fw.value(L['out'])
        assert y.shape == y64.shape and np.isfinite(y).all(), (mode, net, cloud, L['name'])
        extra = 0.0
        truth = y64
        if how != 'f32':   # pieces carry the pending ReLU
            assert ref.RELU[L['out']]
            truth = np.maximum(y64, 0)
            extra = 2.0 ** -22 * np.abs(y).max(axis=1, keepdims=True)
        elif ref.RELU[L['out']] and kind.startswith(OS_FAMILY):   # these kernels store max(x, 0) (conv_os.hip, step 5)
            assert (y >= 0).all()
            truth = np.maximum(y64, 0)
        c = 1.5 * e32 + ADD[mode]
        err = np.abs(y - truth)
        rel = np.maximum(err - extra, 0) / np.maximum(B, 1e-300)
        ratio = float(rel.max())
        # the channel of the worst element and the size of its folded weights next to the layer's largest
        ch = int(np.unravel_index(np.argmax(rel), rel.shape)[1])
        Wa = np.abs(ref.folded(sd, L)[0])
        wrel = float(Wa[:, :, ch].max() / max(Wa.max(), 1e-300))
        rows.append((L['name'], kind, ratio, e32, c, ch, wrel))
        if assert_bound:
            assert (err <= c * B + extra).all(), (mode, net, cloud, li, L['name'], kind, ratio, e32, c)
    if not assert_bound:
        return rows
    # ---- (b) the hand-overs
    fused3 = D == 3 and cin <= 8
    for name in ('T1', 'Y1', 'S1', 'T2', 'Y2', 'S2', 'T4', 'Y4', 'S4', 'T8', 'Y8', 'S8', 'U4', 'V4', 'U2', 'V2', 'U1', 'V1',
                 'CAT4', 'CAT2'):
        relu = ref.RELU[name]
        if fused3:
            amax = fw.get(name, 'amax')
            if fw.has(name, 'f32'):
                assert np.array_equal(amax, ref.row_amax_bits(fw.get(name, 'f32'), relu)), (mode, net, cloud, name)
            else:
                raw = fw.get(name, 'dense_split')
                h, m = ref.dense_planes(raw)
                assert ref.resplit_mismatches(h, m) == 0, (mode, net, cloud, name)
                # the scale the pieces were made with is row_scale_of(amax): the row's largest piece sum IS amax's value
                # up to the split's 2^-22, and sits in [2^14, 2^15] (zero rows: amax = 0, all pieces zero)
                top = np.abs(h.astype(np.float64) + m.astype(np.float64)).max(axis=1)
                av = amax.view(np.float32).astype(np.float64)
                assert ((top == 0) == (amax == 0)).all()
                nz = amax != 0
                assert (np.abs(top[nz] / ref.row_scale_of(amax)[nz] - av[nz]) <= 2.0 ** -22 * av[nz]).all(), (mode, net, cloud, name)
                assert ((top[nz] >= 2.0 ** 14 * (1 - 2.0 ** -22)) & (top[nz] <= 2.0 ** 15)).all()
        else:
            assert f'{name}/amax' in fw.missing and f'{name}/dense_split' in fw.missing
        if fw.has(name, 'split_planes'):
            assert D == 6 and split_mode
            if fw.has(name, 'f32'):
                planes, scale = ref.encode_split6(fw.get(name, 'f32'), relu)
                assert np.array_equal(scale.view(np.uint32), fw.get(name, 'split_scale').view(np.uint32)), (mode, net, cloud, name)
                assert np.array_equal(planes, fw.get(name, 'split_planes')), (mode, net, cloud, name)
        else:
            assert f'{name}/split_planes' in fw.missing and f'{name}/split_scale' in fw.missing
    # which tensors exist as pieces only
    pieces_only = {n for n in ('Y1', 'Y2', 'Y4', 'Y8', 'V4', 'V2', 'V1') if not fw.has(n, 'f32')}
    if fused3 and mode == 'split':
        assert pieces_only == {'Y1', 'Y2', 'V2', 'V1'}
    elif D == 6 and split_mode:
        assert pieces_only == {'Y2', 'Y4', 'Y8', 'V4', 'V2', 'V1'}
        both = {n for n in ('T2', 'S2', 'T4', 'S4', 'T8', 'S8', 'U4', 'U2', 'U1') if fw.has(n, 'split_planes') and fw.has(n, 'f32')}
        assert both == {'T2', 'S2', 'T4', 'S4', 'T8', 'S8', 'U4', 'U2', 'U1'}
    else:
        assert pieces_only == set()
    return rows


@pytest.mark.parametrize('net', list(inp.NETS))
@pytest.mark.parametrize('mode', list(MODES))
def test_every_layer_per_element_against_f64(dumps, mode, net):
    D, cin, cout, ks, norm, _, cl = inp.NETS[net]
    sd = inp.state_dict(net)
    clouds = inp.clouds()
    worst = {}
    for cloud in cl:
        coords = clouds[cloud]
        rows = check_forward(mode, net, cloud, dumps[mode, 'trace'], sd, coords, inp.feats(net, cloud, len(coords)), D, cin, ks, norm)
        for li, (name, kind, ratio, e32, c, _, _) in enumerate(rows):
            w = worst.setdefault((li, name, kind), [0.0, 0.0, ''])
            if ratio >= w[0]:
                w[0], w[2] = ratio, cloud
            w[1] = max(w[1], e32)
    for (li, name, kind), (ratio, e32, cloud) in sorted(worst.items()):
        report(f'{mode:9s} {net:7s} {li:2d} {name:16s} {kind:44s} max |y - f64| / B {ratio:.2e} (cloud {cloud:2s})   f32 reference {e32:.2e}')


@pytest.mark.parametrize('mode', list(MODES))
def test_wide_range_checkpoint_report_only(dumps, mode):
    """Report only (no bound asserted): folded batch-norm scales over eight decades inside a layer -- ONE f16 weight
    scale per layer serves all output channels, so channels far below the largest may keep fewer than 22 bits."""
    import split_f64_inputs as wr_inp
    wr = wr_inp.wide_range_case()
    for net, D, cin, ks, norm, sd, coords, feats in (
            ('wr3', 3, 1, 5, True, wr['sd3'], wr['c3'], np.ones((len(wr['c3']), 1), np.float32)),
            ('wr6', 6, 6, 3, False, wr['sd6'], wr['c6'], wr['f6'])):
        rows = check_forward(mode, net, 'W', dumps[mode, 'wide'], sd, coords, feats, D, cin, ks, norm, assert_bound=False)
        for li, (name, kind, ratio, e32, c, ch, wrel) in enumerate(rows):
            report(f'{mode:9s} {net:7s} {li:2d} {name:16s} {kind:44s} max |y - f64| / B {ratio:.2e} (report only)   f32 reference {e32:.2e}'
                   f'   worst channel {ch:3d}: its largest |w| is {wrel:.1e} of the layer\'s')
