"""The fused inverted-residual launch (f8_ir.hip) at op level, without a GPU: the plan of every case of tests/ir_cases.py against the hand-written
table, the kernel instances as exported symbols, the liveness of every case on the oracle's values, and the graph cuts of pass 1e."""
import functools
import os
import subprocess

import numpy as np
import pytest

import ir_cases
from f8net_amd import _lib
from f8net_amd.net import F8Net

ALL = dict(ir_cases.CASES, max_batch=ir_cases.MAX_BATCH_CASE, pipelined=ir_cases.PIPELINED_CASE)


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return ir_cases.plan(name, case, ir_cases.make_input(name, case), 2)


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, _ = _planned(name)
    assert ir_cases.fused_lines(g.net) == case['expect'], g.net.describe()
    lines = [ln for ln in g.net.describe().splitlines() if 'fused_ir_s' in ln]
    assert len(lines) == len(case['blocks']), g.net.describe()
    off, _, _ = ir_cases.plan(name, case, ir_cases.make_input(name, case), 0)
    assert 'fused_ir_s' not in off.net.describe() and not ir_cases.fused_lines(off.net)
    assert off.net.num_launches == g.net.num_launches + 2 * len(case['blocks'])


def test_every_expected_kernel_is_an_exported_symbol_and_the_table_covers_the_instances():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for _, k in c['expect']}
    for k in sorted(names):
        assert f'void {k}(f8::IRArgs)' in syms, k
    mfma = [(32, 32), (32, 64), (64, 64), (64, 96), (96, 96)]
    valu = [(96, 160), (160, 160), (160, 320)]
    for ci, co in mfma:
        assert any(k.startswith(f'f8::fused_ir_kernel<{ci}, {co}, ') for k in names), (ci, co)
    for inst in (0, 1, 2):
        assert any(f', {inst}, true, 8>' in k for k in names), inst
    for ci, co in valu:
        assert f'f8::fused_ir_kernel<{ci}, {co}, 0, false, 4>' in names, (ci, co)


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure: the final value has more than 8 distinct values; every int8 tensor a depthwise, project, chained expand or
    reader conv reads has at least 16 distinct values and fewer than half of its entries at a clamp bound; a case that aims at a wrap or a
    clamp shows that event in the oracle's values."""
    case = ALL[name]
    g, out, ids = _planned(name)
    assert np.unique(g.v[out][0]).size > 8
    assert len(g.taps) == sum(3 if i else 2 for i in range(len(case['blocks']))) + len(case['readers'] or [])
    for label, xq, sgn in g.taps:
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        assert ((xq == lo) | (xq == hi)).mean() < 0.5, label
    aim = case.get('aim')
    if aim == 'bias_big':
        b = case['blocks'][0]
        e, d = ids[0][0], ids[0][1]
        for t, n in ((e, b['in_fl'] + b['w_fl'] - b['dw_in_fl']), (d, b['dw_in_fl'] + b['dw_w_fl'] - b['pw_in_fl'])):
            r = g.raw[t].astype(np.int64)
            assert (r > 2 ** 31 - 2 ** 13).any(), 'no accumulator next to 2^31'
            # the accumulator itself wrapped past 2^31, or the rounding add `v + 2^(n-1)` of the requantisation does
            assert (r < -2 ** 30).any() or (r + (1 << (n - 1)) > 2 ** 31 - 1).any(), 'nothing wraps'
    elif aim == 'stream_clamp':
        assert (g.v[ids[1][3]][0] == ir_cases.INT32_MIN_CLAMP).any()
        assert not (g.v[ids[1][3]][0] == -2 ** 31).any()
    elif aim == 'join':
        assert (np.abs(g.v[ids[0][3]][0].astype(np.int64)) > 2 ** 30).any()
    else:
        assert aim is None


# ---- graph cuts of pass 1e
def _cut(cin=32, cout=32, E=64, H=6, W=6, stride=1, second_reader=None, net_output=None, join=None, reads_input=False):
    """pre 1x1 -> expand -> depthwise -> project [-> join] -> a 1x1 reader (the net output unless `net_output` names expand / dw).
    second_reader: 'expand' / 'dw' get a second 1x1 reader (joined into the output); join: 'input' (the block input) or 'other' (another conv)."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    conv = lambda t, wt, **kw: net.conv(t, wt, None, **dict(dict(stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, quant_input=True,
                                                                 relu=False), **kw))
    net = F8Net()
    t = net.input(cin, H, W, 5)
    if not reads_input:
        t = conv(t, w(cin, cin, 1, 1))
    other = conv(t, w(cout, cin, 1, 1), stride=stride) if join == 'other' else None     # recorded first: the project conv then hosts the join
    e = conv(t, w(E, cin, 1, 1), relu=True)
    d = conv(e, w(E, 1, 3, 3), stride=stride, pad=1, groups=E, input_fl=6, input_signed=False, relu=True)
    p = conv(d, w(cout, E, 1, 1), input_fl=6, input_signed=False)
    if join == 'input':
        p = net.add(p, t)
    elif join == 'other':
        p = net.add(p, other)
    out = conv(p, w(32, cout, 1, 1))
    if second_reader:
        src = e if second_reader == 'expand' else d
        Ho, Wo = (H, W) if second_reader == 'expand' else ((H - 1) // stride + 1, (W - 1) // stride + 1)
        extra = conv(src, w(32, E, 1, 1), input_fl=6, input_signed=False)
        if (Ho, Wo) != ((H - 1) // stride + 1, (W - 1) // stride + 1):
            extra = conv(extra, w(32, 1, 3, 3), stride=stride, pad=1, groups=32)
        out = net.add(out, extra)
    net.output({'expand': e, 'dw': d}.get(net_output, out), as_float=False)
    net.set_option('fuse_irchain', 0)
    net.set_option('fuse_ir', 2)
    net.finalize(2)
    return [ln.split()[1] for ln in net.describe().splitlines() if 'fused_ir_s' in ln]


def test_graph_cuts():
    assert len(_cut()) == 1
    assert len(_cut(join='input')) == 1
    assert len(_cut(stride=2)) == 1
    assert not _cut(second_reader='expand')                     # the expand result has a second reader
    assert not _cut(second_reader='dw')                         # the depthwise result has a second reader
    assert not _cut(second_reader='dw', stride=2)
    assert not _cut(net_output='expand')                        # ... is the net output
    assert not _cut(net_output='dw')
    assert not _cut(join='other')                               # a join with a tensor other than the block input
    assert not _cut(reads_input=True)                           # the block reads the net input
    assert not _cut(cin=64, cout=32)                            # no <64, 32> instance
    assert len(_cut(cin=64, cout=64)) == 1


def test_a_join_on_a_stride_2_block_stays_unfused():
    """Only on a 1 x 1 map does a stride-2 block's result have the shape of its input."""
    assert len(_cut(H=1, W=1, join='input')) == 1
    assert len(_cut(H=1, W=1, stride=2)) == 1
    assert not _cut(H=1, W=1, stride=2, join='input')


def test_output_width_above_the_pixel_cap_stays_unfused():
    assert len(_cut(cin=64, cout=64, H=2, W=128)) == 1
    assert not _cut(cin=64, cout=64, H=2, W=130)                # 130 > 128 output pixels of one row
    assert len(_cut(H=2, W=256)) == 1
    assert not _cut(H=2, W=260)                                 # 260 > 256 on the <32, 32> instance
    assert len(_cut(cin=64, cout=64, H=2, W=256, stride=2)) == 1   # the cap is on the OUTPUT width
