"""Case table, reference and graph builder of the tests of transposed convolutions (f8_net_conv_transpose / `F8Net.conv_transpose`, f8_deconv.hip):
tests/test_deconv_plan.py (acceptance, refusals, tokens, kernel symbols, forms, launch_info, the tap-cut comparison, ONNX / IntGraph round trips, tap
liveness; no GPU) and tests/test_gpu_deconv.py (every case bit for bit on the device).  No test functions here.

The reference (ref_ops.deconv_exact / deconv_ref) is numpy on int64 in the SCATTER form, wrapped to int32 at the end: every input pixel (ih, iw) adds x[ci] * w[ci, co, kh, kw] at
(s ih + kh, s iw + kw) of the full (H - 1) s + k + output_padding square, of which the output is the window [pad, pad + P).  It is pinned two ways
(tests/test_deconv_plan.py): to torch.nn.functional.conv_transpose2d in float64 with exact equality (`pin_to_torch`), and to `oracle.conv2d` over the
zero-stuffed input with flipped, in / out-swapped weights at pad' = k - 1 - pad (`pin_to_oracle`).

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> a 1x1 producer conv that reads it as it is, `cin` outputs at
fraclen 13 [ReLU] -> the transposed conv, which requantises them to unsigned fraclen 4 behind the ReLU (shift 9) or to signed fraclen 3 (shift 10)
-> readers: one 32-output 1x1 conv per (input_fl, signed), summed (concat_cases.readers).  src = 'input': the transposed conv reads the net input
(cin channels, 0 .. 255 at fraclen 8) as it is, no requantisation.

The expected plan token, kernel symbol and the forms the launch writes are WRITTEN BY HAND; nothing here asks the planner for them."""
import sys

import numpy as np

import graph_cases
from concat_cases import FUSE_ALL, X_FL, producer, readers  # noqa: F401  (the tests take them from here)
from f8net_amd import synth
from graph_cases import launch_lines
from ir_cases import _b, _w
from oracle import oracle
from ref_ops import deconv_exact, deconv_ref


def symbol(cout):
    """Two cout tiles per wave where the padded output has two (cout > 32), else one."""
    return 'f8::deconv_kernel<2>' if cout > 32 else 'f8::deconv_kernel<1>'


def out_size(n, k, s, pad, op):
    return (n - 1) * s - 2 * pad + k + op


def stuffed_input(x, s, op):
    """s - 1 zeros between the pixels, `op` zero rows / columns at the bottom / right."""
    N, C, H, W = x.shape
    z = np.zeros((N, C, (H - 1) * s + 1 + op, (W - 1) * s + 1 + op), x.dtype)
    z[:, :, :(H - 1) * s + 1:s, :(W - 1) * s + 1:s] = x
    return z


def conv_weights(w):
    """[cin, cout, k, k] -> the plain conv's [cout, cin, k, k], flipped in both axes."""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def pin_to_torch(x, w, b, s, pad, op):
    import torch
    import torch.nn.functional as F
    want = F.conv_transpose2d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)),
                              None if b is None else torch.from_numpy(np.asarray(b, np.float64)), stride=s, padding=pad, output_padding=op)
    got = deconv_exact(x, w, b, s, pad, op)
    assert np.abs(got).max() < 2 ** 52
    np.testing.assert_array_equal(got.astype(np.float64), want.numpy())


def pin_to_oracle(x, w, b, s, pad, op):
    k = w.shape[2]
    want = oracle.conv2d(stuffed_input(np.asarray(x, np.int32), s, op), conv_weights(w).astype(np.int32), b, 1, k - 1 - pad, 1)
    np.testing.assert_array_equal(deconv_ref(x, w, b, s, pad, op), want)


# ---- weights.  Accumulators around 2^6 x 100, which a reader's shift of 6 (fraclen 10 -> 4) turns into 8 bits
def weights(c, seed=40):
    k, s, cin, cout = c['k'], c['s'], c['cin'], c['cout']
    taps = max(1.0, (k / s) ** 2) * cin                              # taps one output meets
    xrms = 90.0 if c['src'] == 'input' else 40.0
    sig = float(np.clip(6400.0 / (xrms * taps ** 0.5), 0.7, 40.0))
    w = _w(seed, (cin, cout, k, k), sig)
    if c['bias_big']:                                                # next to +-2^31: sums that leave int32 and wrap
        b = np.where(np.arange(cout) % 2 == 0, 2 ** 31 - 1 - 50 * np.arange(cout), -2 ** 31 + 50 * np.arange(cout)).astype(np.int64).astype(np.int32)
    else:
        b = _b(seed + 1, cout, 2.0 ** 11, 2.0 ** 12 if c['relu'] else 0.0)
    return w, b


def deconv_of(g, t, c, w_eval=None, label='up'):
    w, b = weights(c)
    if c['src'] == 'input':
        fmt = dict(input_fl=X_FL, input_signed=False, quant_input=False)
    elif c['src'] == 'signed':
        fmt = dict(input_fl=3, input_signed=True, quant_input=True)
    else:
        fmt = dict(input_fl=4, input_signed=False, quant_input=True)
    return g.conv_transpose(t, w, b, stride=c['s'], pad=c['pad'], output_padding=c['op'], weight_fl=6, relu=c['relu'], label=label, w_eval=w_eval, **fmt)


def _source(g, x0, c):
    if c['src'] == 'input':
        return x0
    return producer(g, x0, 0, c['cin'], 9 if c['src'] == 'conv' else 10, w_fl=5, relu=c['src'] == 'conv')


# ---- the builders.  Each returns (output tensor ids in output order, [transposed conv tensor ids])
def _plain(g, x0, c, w_eval=None):
    up = deconv_of(g, _source(g, x0, c), c, w_eval)
    outs = []
    if c['readers']:
        outs.append(readers(g, up, c['readers']))
        g.output(outs[0])
    if c['out']:
        outs.append(up)
        g.output(up, as_float=c.get('as_float', False))
    return outs, [up]


def _fcn(g, x0, c, w_eval=None):
    """FCN skip: a score conv on the coarse level (the input max-pooled by the stride), upsampled by the transposed conv (fraclen 10), joined with a
    lateral 1x1 score conv of the fine level (fraclen 9: the join shifts it by 1); the join is the output.  The transposed conv is the join's LATER
    producer: the join stays an `add:` launch."""
    s = c['s']
    lateral = producer(g, x0, 1, c['cout'], 5, w_fl=1, relu=False)
    top = producer(g, g.maxpool(x0, s, s, 0), 0, c['cin'], 9, w_fl=5, relu=True)
    up = deconv_of(g, top, c, w_eval)
    assert g.v[up][0].shape == g.v[lateral][0].shape
    out = g.add(up, lateral, relu=False)
    g.output(out)
    return [out], [up]


def _unet(g, x0, c, w_eval=None):
    """U-Net decoder step: the transposed conv of the coarse level concatenated with a skip of the fine level at its fraclen, one int8 reader behind
    the concat.  c['opts'] chooses the concat's mode; the byte-gather mode asks the transposed conv for the concat's int8 format."""
    s = c['s']
    top = producer(g, g.maxpool(x0, s, s, 0), 0, c['cin'], 9, w_fl=5, relu=True)
    up = deconv_of(g, top, c, w_eval)
    skip = producer(g, x0, 1, 24, 6, w_fl=2, relu=True)
    assert g.v[up][0].shape[2:] == g.v[skip][0].shape[2:] and g.v[up][1] == g.v[skip][1]
    out = readers(g, g.concat([up, skip], label='cat'), [(4, False)])
    g.output(out)
    return [out], [up]


def _case(k, s, pad, op, H, W, cin, cout, *, forms=(0, 1), build=_plain, **kw):
    """H x W: the SOURCE map.  forms: (int32 forms, int8 forms) the launch writes — by hand."""
    c = dict(k=k, s=s, pad=pad, op=op, H=H, W=W, cin=cin, cout=cout, N=3, forms=forms, build=build, src='conv', relu=True, readers=[(4, False)],
             out=False, bias_big=False, opts={})
    c.update(kw)
    c['tok'] = f'deconv{k}x{k}s{s}:' if s > 1 else f'conv{k}x{k}s1_'
    assert out_size(H, k, s, pad, op) >= 1 and out_size(W, k, s, pad, op) >= 1 and 0 <= op < max(s, 1) and 0 <= pad < k
    return c


U, S = (4, False), (3, True)
CASES = {
    # ---- geometry (k, s, pad, op) x maps x channels
    'g_2200': _case(2, 2, 0, 0, 3, 5, 8, 8),                                           # one K step (k = s = 2, cin 8 -> CK 32): shorter than any ring
    'g_2200_7x7': _case(2, 2, 0, 0, 7, 7, 64, 64, src='signed', relu=False, readers=[S]),
    'g_4210': _case(4, 2, 1, 0, 7, 7, 40, 21),
    'g_4210_9x11': _case(4, 2, 1, 0, 9, 11, 96, 40),                                   # 99 pixels per image and phase: tiles straddle images
    'g_3211': _case(3, 2, 1, 1, 3, 5, 64, 130),                                        # coutP 160: five cout tiles, the last workgroup half empty
    'g_3200': _case(3, 2, 0, 0, 3, 1, 40, 8, src='signed', relu=False),
    'g_4400': _case(4, 4, 0, 0, 1, 3, 8, 40),
    'g_5321': _case(5, 3, 2, 1, 3, 5, 160, 21, forms=(0, 2), readers=[U, S], relu=False),
    'g_8420': _case(8, 4, 2, 0, 3, 5, 40, 64),
    'g_7231': _case(7, 2, 3, 1, 7, 7, 8, 130, src='input'),
    'g_7231_3x5': _case(7, 2, 3, 1, 3, 5, 96, 8, forms=(1, 2), readers=[U, S, (5, False)], relu=False),      # a third format: int32 + `requant:`
    # ---- phases without a tap (k < s): their outputs are the bias
    'e_1201': _case(1, 2, 0, 1, 3, 5, 40, 40),
    'e_1201_1x1': _case(1, 2, 0, 1, 1, 1, 8, 8, src='input'),                          # 2 x 2 outputs per image, three of them bias only
    'e_2300': _case(2, 3, 0, 0, 3, 5, 64, 21, src='signed', relu=False, readers=[S]),
    'e_3412': _case(3, 4, 1, 2, 7, 7, 8, 64, src='input'),
    # ---- stride 1: planned as a conv
    's_3110': _case(3, 1, 1, 0, 7, 7, 40, 40),
    's_3100': _case(3, 1, 0, 0, 3, 5, 8, 21, src='signed', relu=False),
    # ---- formats
    'f_input_160': _case(4, 2, 1, 0, 3, 5, 160, 40, src='input'),                      # the net input as it is
    'f_norelu_two': _case(4, 2, 1, 0, 7, 7, 64, 40, forms=(0, 2), readers=[U, S], relu=False),
    'f_out': _case(2, 2, 0, 0, 7, 7, 40, 21, forms=(1, 0), readers=None, out=True),
    'f_out_f32': _case(3, 2, 1, 1, 3, 5, 8, 8, forms=(1, 0), readers=None, out=True, as_float=True),
    'f_out_reader': _case(4, 2, 1, 0, 3, 5, 64, 64, forms=(1, 1), out=True),           # int32 next to an int8 reader
    'f_wrap': _case(4, 2, 1, 0, 3, 5, 40, 40, forms=(1, 0), readers=None, out=True, relu=False, bias_big=True),
    'f_wrap_u8': _case(3, 2, 0, 0, 3, 5, 8, 40, forms=(1, 1), out=True, relu=False, bias_big=True, src='input'),
    'f_fcn': _case(4, 2, 1, 0, 3, 5, 21, 21, forms=(1, 0), build=_fcn, relu=False),
    'f_unet_i8': _case(2, 2, 0, 0, 3, 5, 64, 40, build=_unet),
    'f_unet_i32': _case(2, 2, 0, 0, 3, 5, 64, 40, forms=(1, 0), build=_unet, opts={'concat_i8': 0}),
}


def input_hw(c):
    """The input's map: the source map, except where the case pools the input down to its coarse level first."""
    if c['build'] in (_fcn, _unet):
        assert out_size(c['H'], c['k'], c['s'], c['pad'], c['op']) == c['H'] * c['s']
        return c['H'] * c['s'], c['W'] * c['s']
    return c['H'], c['W']


def input_channels(c):
    return c['cin'] if c['src'] == 'input' else 8


def make_input(name, n=None):
    c = CASES[name]
    return synth.rand_uniform_int(5, f'dcx{name}', (n or c['N'], input_channels(c)) + input_hw(c), 0, 255).astype(np.int32)


def deconv_lines(net, label='up'):
    """[(launch index, plan token, kernel symbol)] of the launches that write the tensor labelled `label`, in launch order."""
    return [ln for ln in launch_lines(net, label=label) if ln[1] not in ('output:', 'tap:', 'requant:')]


def check_lines(c, lines, describe=''):
    """The case's one launch: `deconv{k}x{k}s{s}:` on f8::deconv_kernel<1 / 2>, or — stride 1 — a conv{k}x{k}s1_* token on a conv kernel."""
    assert len(lines) == 1, describe
    (_, tok, sym), = lines
    if c['s'] > 1:
        assert (tok, sym) == (c['tok'], symbol(c['cout'])), describe
    else:
        assert tok.startswith(c['tok']) and sym.startswith('f8::conv') and 'deconv' not in tok + sym, describe


# (the reference runs over N images and the handle is planned for N: no spare image)
graph_cases.bind_cases(sys.modules[__name__], spare_image=False)      # build_graph(..., w_eval=None), reference, plan, int_graph
