"""Case table, reference and graph builder of the tests of windowed average pooling (f8_net_avgpool_window / `F8Net.avgpool`, f8_sumpool.hip):
tests/test_avgpool_plan.py (acceptance, refusals, tokens, kernel symbols on the three legs of option sumpool_wide, forms, launch_info, the cut cases,
the ONNX round trip; no GPU) and tests/test_gpu_avgpool.py (every case on every leg, bit for bit on the device).  No test functions here.

The reference is numpy on int64 over the zero-padded input: the k x k strided slices summed, wrapped to int32 at the end (`sumpool_exact`,
`sumpool_ref` of tests/ref_ops.py); the fraclen grows by `shift`, by default the reference's round(log2(k^2)).  `pin_to_torch` holds it with exact equality against
F.avg_pool2d(float64, count_include_pad=True, divisor_override=1) — the divisor 1, not "the average times k^2": sum / 9 * 9 is not exact in floating
point — and `pin_to_oracle` against the oracle's depthwise conv with all-ones weights on 8-bit inputs, where the two definitions coincide.

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv that reads it as it is, C outputs at
fraclen 13 -> pool -> readers: one 32-output 1x1 conv per (input_fl, signed), summed (concat_cases.readers), and / or the pool as an output.

The expected plan token of every case, the kernel symbol on each leg and the forms its launch writes are WRITTEN BY HAND (the rule: DESIGN.md
4.5l); nothing here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take them from here)
from f8net_amd import synth
from graph_cases import launch_lines
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import default_shift, sumpool_exact, sumpool_ref

# option sumpool_wide = 1: windows of this size and more that do not overlap (stride >= kernel) run the wide kernel (sumpool_wide_rule, f8_internal.h;
# measured: profiles/sumpool_r12.md) — by hand
WIDE_FROM = 3
GLOBAL = 'avgpool_sum:'


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def pin_to_torch(x, k, stride, pad):
    """sumpool_exact against torch in float64 with divisor_override=1: exact equality (the sums stay far below 2^53)."""
    import torch
    import torch.nn.functional as F
    want = F.avg_pool2d(torch.from_numpy(np.asarray(x, np.float64)), k, stride, pad, ceil_mode=False, count_include_pad=True, divisor_override=1)
    got = sumpool_exact(x, k, stride, pad)
    assert np.abs(got).max() < 2 ** 52
    np.testing.assert_array_equal(got.astype(np.float64), want.numpy())


def pin_to_oracle(x, k, stride, pad):
    """... and against the oracle's depthwise conv with all-ones weights (inputs already in 8-bit range: no requantisation in between)."""
    x = np.asarray(x, np.int32)
    assert x.min() >= -127 and x.max() <= 255
    C = x.shape[1]
    want = oracle.conv2d(x, np.ones((C, 1, k, k), np.int32), None, stride, pad, C)
    np.testing.assert_array_equal(sumpool_ref(x, 0, k, stride, pad)[0], want)


# ---- the builders.  Each returns (output tensor ids in output order, [pool tensor ids])
def _pool(g, t, c, label='pool'):
    return g.avgpool(t, c['k'], c['s'], c['pad'], label=label)


def _plain(g, x0, c):
    """producer -> pool -> readers (and / or the pool itself as an output)."""
    p = producer(g, x0, 0, c['C'], 9, w_fl=5, relu=c['relu'])
    pl = _pool(g, p, c)
    outs = []
    if c['readers']:
        outs.append(readers(g, pl, c['readers']))
        g.output(outs[0])
    if c['out']:
        outs.append(pl)
        g.output(pl, as_float=c.get('as_float', False))
    return outs, [pl]


def _coarse(g, x0, c):
    """The input on the pool's output map: max-pooled with the pool's own geometry (0 .. 255 stays 0 .. 255)."""
    return g.maxpool(x0, c['k'], c['s'], c['pad'])


def _join(g, x0, c):
    """ResNet-D's shortcut turned round: the pool (fraclen 13 + shift) joined with a 1x1 conv of the coarse input one fraclen below it: the join reads
    the pool in int32 and shifts the other operand by 1; one int8 reader behind the join."""
    pl = _pool(g, producer(g, x0, 0, c['C'], 9, w_fl=5, relu=True), c)
    sh = default_shift(c['k'])
    other = producer(g, _coarse(g, x0, c), 1, c['C'], 8 + sh, w_fl=4 + sh, relu=False)
    out = readers(g, g.add(pl, other, relu=True), [(4, False)])
    g.output(out)
    return [out], [pl]


def _concat(g, x0, c):
    """DenseNet / PSP: the pool concatenated with a 24-channel conv of the coarse input at the pool's fraclen, one int8 reader behind the concat.
    c['opts'] chooses the concat's mode; the byte-gather mode asks the pool for the concat's int8 format."""
    pl = _pool(g, producer(g, x0, 0, c['C'], 9, w_fl=5, relu=True), c)
    sh = default_shift(c['k'])
    skip = producer(g, _coarse(g, x0, c), 1, 24, 9 + sh, w_fl=5 + sh, relu=True)
    out = readers(g, g.concat([pl, skip], label='cat'), [(4, False)])
    g.output(out)
    return [out], [pl]


def _psp(g, x0, c):
    """A PSP branch: pool -> nearest upsample back to the source map -> reader.  The byte-copy upsample asks the pool for the reader's int8 format."""
    pl = _pool(g, producer(g, x0, 0, c['C'], 9, w_fl=5, relu=True), c)
    up = g.upsample(pl, c['s'], 'nearest', label='up')
    out = readers(g, up, c['readers'])
    g.output(out)
    return [out], [pl]


def _src_tap(g, x0, c):
    """The pool's source is also a network output (output 1): it exists in int32 anyway."""
    p = producer(g, x0, 0, c['C'], 9, w_fl=5, relu=True)
    pl = _pool(g, p, c)
    out = readers(g, pl, c['readers'])
    g.output(out)
    g.output(p)
    return [out, p], [pl]


def _wrap(g, x0, c):
    """upsample_cases._wrap's conv — 3x3 over 32 channels (0 .. 255), weights 64 .. 127: accumulators around 2^22 — with biases up to +-2^30 on top;
    a 3 x 3 window sums nine of them: the exact sums pass 2^31 and the result is their int32 wrap.  The pool is the output."""
    w = synth.rand_uniform_int(11, 'poolwrapw', (c['C'], 32, 3, 3), 64, 127).astype(np.int32)
    p = g.conv(x0, w, _b(12, c['C'], 2.0 ** 29), pad=1, groups=1, weight_fl=0, input_fl=X_FL, input_signed=False, relu=False, quant_input=False)
    pl = _pool(g, p, c)
    g.output(pl)
    exact = sumpool_exact(g.v[p][0], c['k'], c['s'], c['pad'])
    assert (np.abs(exact) >= 2 ** 31).mean() > 0.25, 'the exact sums stay inside int32: the case shows nothing'
    return [pl], [pl]


# ---- small nets (the GPU tests run them; the plan tests plan them).  Each takes (graph, input id) and returns the output ids
def _dense_block(g, run, k0, fl_run):
    """Two DenseNet layers on the running concat (read at unsigned fraclen 4 / 3 in turn): a 3x3 conv, 32 outputs one fraclen below it, appended."""
    for k in range(2):
        fl = 4 - (k & 1)
        grow = producer(g, run, k0 + k, 32, fl_run - 5, w_fl=fl_run - 1 - fl, relu=True, in_fl=fl, quant_input=True, kernel=3)
        run = g.concat([run, grow], label=f'dense{k0 + k}')
    return run


def net_densenet(g, x0):
    """64 channels on 12 x 12 -> dense block (128 channels) -> transition: 1x1 to 64, average 2x2 / 2 -> dense block on 6 x 6 -> reader."""
    run = _dense_block(g, producer(g, x0, 0, 64, 9, w_fl=5, relu=True), 1, 13)
    t = producer(g, run, 3, 64, 9, w_fl=9, relu=True, in_fl=4, quant_input=True)           # fraclen 13
    run = _dense_block(g, g.avgpool(t, 2, label='transition.pool'), 4, 15)                  # fraclen 15: an exact average
    out = readers(g, run, [(4, False)])
    g.output(out)
    return [out]


def net_inception(g, x0):
    """concat_cases' Inception-3a with the branch it could not have: average 3x3 / 1 / pad 1 of the 192-channel input (int32 at fraclen 8 + 3), read
    back at unsigned fraclen 8 by the 1x1 (32)."""
    b1 = producer(g, x0, 0, 64, 9, w_fl=5, relu=True)
    b2 = producer(g, producer(g, x0, 1, 96, 9, w_fl=5, relu=True), 2, 128, 9, w_fl=9, relu=True, in_fl=4, quant_input=True, kernel=3)
    b3 = producer(g, producer(g, x0, 3, 16, 9, w_fl=5, relu=True), 4, 32, 9, w_fl=9, relu=True, in_fl=4, quant_input=True, kernel=5)
    b4 = producer(g, g.avgpool(x0, 3, 1, 1, label='pool_proj.pool'), 5, 32, 9, w_fl=5, relu=True, in_fl=8, quant_input=True)
    out = readers(g, g.concat([b1, b2, b3, b4], label='inception_3a'), [(4, False)])
    g.output(out)
    return [out]


def net_resnet_d(g, x0):
    """ResNet-D's stride-2 opener: body 1x1 -> 3x3 / 2 -> 1x1; shortcut average 2x2 / 2 -> 1x1; join, ReLU.  Every conv reads at unsigned fraclen 4;
    both arms end at fraclen 13."""
    x = producer(g, x0, 0, 64, 9, w_fl=5, relu=True)                                                      # 64 x 8 x 8 at fraclen 13
    b = producer(g, x, 1, 32, 9, w_fl=9, relu=True, in_fl=4, quant_input=True)
    w = _w(131, (32, 32, 3, 3), 2.0 ** 9 * 100 / (128 * 288 ** 0.5))
    b = g.conv(b, w, _b(132, 32, 2.0 ** 9 * 20, 2.0 ** 9 * 40), stride=2, pad=1, groups=1, weight_fl=9, input_fl=4, input_signed=False, relu=True)
    b = producer(g, b, 3, 128, 9, w_fl=9, relu=False, in_fl=4, quant_input=True)
    sc = producer(g, g.avgpool(x, 2, label='shortcut.pool'), 4, 128, 9, w_fl=9, relu=False, in_fl=4, quant_input=True)
    out = readers(g, g.add(b, sc, relu=True), [(4, False)])
    g.output(out)
    return [out]


# name: (builder, input (C, H, W), the pool tokens of its plan)
NETS = {'densenet': (net_densenet, (8, 12, 12), ['sumpool2x2s2:']), 'inception': (net_inception, (192, 12, 12), ['sumpool3x3s1:']),
        'resnet_d': (net_resnet_d, (8, 8, 8), ['sumpool2x2s2:'])}


def net_input(name, n=2):
    return synth.rand_uniform_int(5, f'poolnet{name}', (n,) + NETS[name][1], 0, 255).astype(np.int32)


def _case(C, H, W, k, s, pad, *, forms=(0, 1), build=_plain, **kw):
    """H x W: the SOURCE map.  forms: (int32 forms, int8 forms) the pool's launch writes — by hand."""
    c = dict(C=C, H=H, W=W, N=3, k=k, s=s, pad=pad, forms=forms, build=build, readers=[(4, False)], out=False, relu=True, cin=8, opts={})
    c.update(kw)
    return c


U, S = (4, False), (3, True)
CASES = {
    # ---- geometry (one unsigned int8 reader)
    'g_2s2_8x8': _case(24, 8, 8, 2, 2, 0),
    'g_2s2_7x9': _case(40, 7, 9, 2, 2, 0),                                       # floor drops the last row / column; H != W
    'g_3s1p1_5x7': _case(64, 5, 7, 3, 1, 1),                                     # every border class; Q = 7: blocks straddle rows and images; M = 140
    'g_3s2p1_7x9': _case(24, 7, 9, 3, 2, 1),
    'g_3s2p0_7x9': _case(40, 7, 9, 3, 2, 0),
    'g_2s3p1_8x8': _case(24, 8, 8, 2, 3, 1),                                     # stride > kernel: the window overhangs at the top / left only
    'g_4s2p2_8x10': _case(64, 8, 10, 4, 2, 2),                                   # pad = kernel / 2
    'g_1s2_7x9': _case(24, 7, 9, 1, 2, 0),                                       # a subsampler; the walker on every leg
    'g_5s1p2_6x7': _case(40, 6, 7, 5, 1, 2),                                     # the runtime-K instance
    'g_6s6_12x12': _case(24, 12, 12, 6, 6, 0),
    'g_8s8_16x24': _case(40, 16, 24, 8, 8, 0),
    'g_15s15_15x30': _case(64, 15, 30, 15, 15, 0),                               # the wide kernel on the default leg; 225 taps over 64 lanes
    'g_12_12x12_global': _case(40, 12, 12, 12, 12, 0, forms=None),               # the global window: `avgpool_sum:`, no sumpool launch
    # ---- readers
    'r_two': _case(40, 5, 7, 3, 1, 1, forms=(0, 2), readers=[U, S], relu=False),
    'r_three': _case(64, 7, 9, 2, 2, 0, forms=(1, 2), readers=[U, S, (5, False)], relu=False),      # a third format: int32 + `requant:`
    'r_out': _case(24, 5, 7, 3, 1, 1, forms=(1, 0), readers=None, out=True),
    'r_out_f32': _case(40, 7, 9, 2, 2, 0, forms=(1, 0), readers=None, out=True, as_float=True),
    'r_out_reader': _case(64, 7, 9, 3, 2, 1, forms=(1, 1), out=True),
    'r_join': _case(40, 8, 8, 2, 2, 0, forms=(1, 0), build=_join),
    'r_concat_i8': _case(40, 8, 8, 2, 2, 0, build=_concat),
    'r_concat_i32': _case(40, 7, 9, 3, 2, 1, forms=(1, 0), build=_concat, opts={'concat_i8': 0}),
    'r_psp': _case(24, 12, 12, 6, 6, 0, build=_psp),
    'r_src_tap': _case(40, 7, 9, 2, 2, 0, build=_src_tap),
    # ---- the int32 wrap
    'w_wrap': _case(40, 5, 7, 3, 1, 1, forms=(1, 0), build=_wrap, cin=32),
}
POOLED = [k for k, c in CASES.items() if c['forms'] is not None]                 # the cases with a sumpool launch


def token(c):
    return f"sumpool{c['k']}x{c['k']}s{c['s']}:"


def symbol(c, leg):
    """The kernel of the case's pool with option sumpool_wide = leg."""
    k = c['k']
    if (leg == 2 and k >= 2) or (leg == 1 and k >= WIDE_FROM and c['s'] >= k):
        return 'f8::sumpool_wide_kernel'
    return f'f8::sumpool_i32_kernel<{k if k in (2, 3) else 0}>'


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'poolx{name}', (n or c['N'], c['cin'], c['H'], c['W']), 0, 255).astype(np.int32)


def pool_lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's windowed-pool launches, in launch order."""
    return launch_lines(net, 'sumpool')


graph_cases.bind_cases(sys.modules[__name__])      # build_graph, reference, plan, int_graph
