#!/usr/bin/env python3
"""A/B of the dilated depthwise 5x5 / 7x7 launches (option dw_dilated): f8::dwconvk_dil_dot4_kernel<K, ROWS> (dw_dilated = 1; ROWS by the rule, and forced
to 1 and to 2 through option dwdil_rows) against f8::dwconvk_kernel (dw_dilated = 2), against what a caller could run before the option existed — the
zero-stuffed (d (K - 1) + 1)-square kernel under dw_large = 1 (f8::dwlk_kernel where dwlk_rule says so) and dw_large = 2 (f8::dwconvk_kernel) — and
against the UNDILATED f8::dwconvk_dot4_kernel<K, 1> on the same map, the yardstick per multiply-add.

    python tools/ab_dwdil.py --shape I [--reps 30] [--batch 128]       (one shape per process: give each its own time limit)

Per shape a net `input (C ch) -> depthwise K x K at dilation d, stride 1, pad d (K / 2), ReLU -> 1x1 conv to 32` is planned once per variant with split = 1;
the measured value is the depthwise step's own time from f8_net_run_profiled (HIP events around the launch), the variants alternating inside one process,
`--reps` repetitions each after two warm-up runs; the median is reported.  MACs = K K C P Q N for every variant (the stuffed kernels multiply
(d (K - 1) + 1)^2 taps for them).  Every variant but the undilated yardstick must give the same values, bit for bit, before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# K, d, C, map: MobileNet-V3-Large at output stride 16 (672 / 960 x 14^2) and 8 (240 x 28^2 d2, 672 / 960 x 28^2 d4), a MnasNet-class 7x7 at d2,
# VAN-B2's 7x7 at d3 / pad 9 on its four stages
SHAPES = [(5, 2, 672, 14), (5, 2, 960, 14), (5, 2, 240, 28), (5, 4, 672, 28), (5, 4, 960, 28), (7, 2, 480, 14),
          (7, 3, 64, 56), (7, 3, 128, 28), (7, 3, 320, 14), (7, 3, 512, 7)]


def dw_net(K, d, C, H, N, opts, stuffed=False):
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    w = np.clip(synth.rand_normal_int(1, f'w.{K}.{C}', (C, 1, K, K), 90.0 / K), -127, 127).astype(np.int32)
    pad = d * (K // 2)
    if stuffed:                                                     # the same conv at dilation 1: zeros between the taps
        E = d * (K - 1) + 1
        ws = np.zeros((C, 1, E, E), np.int32)
        ws[:, :, ::d, ::d] = w
        w, d = ws, 1
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    t = net.conv(t, w, b, stride=1, pad=pad, groups=C, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True, dilation=d)
    r = net.conv(t, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    return net.finalize(N)                                          # launches: input, the conv under test (1), the reader, output


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shape', type=int, required=True, help=f'0 .. {len(SHAPES) - 1}')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_dwdil.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    K, d, C, H = SHAPES[args.shape]
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| shape | variant | kernel | µs median (min .. max) | GMAC | ns / MMAC |')
    print('|---|---|---|---|---:|---:|')
    x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
    variants = [('dw_dilated=1', d, {'dw_dilated': 1}, False), ('dw_dilated=1, ROWS 1', d, {'dw_dilated': 1, 'dwdil_rows': 1}, False),
                ('dw_dilated=1, ROWS 2', d, {'dw_dilated': 1, 'dwdil_rows': 2}, False), ('dw_dilated=2', d, {'dw_dilated': 2}, False),
                ('stuffed, dw_large=1', d, {'dw_large': 1}, True), ('stuffed, dw_large=2', d, {'dw_large': 2}, True), ('undilated dot4', 1, {}, False)]
    nets, outs = {}, {}
    for name, dil, opts, stuffed in variants:
        nets[name] = dw_net(K, dil, C, H, N, opts, stuffed)
        for _ in range(2):                                           # warm-up (upload, code objects)
            outs[name], _ = nets[name].run_profiled(x)
    for name in nets:
        print(f'<!-- {name}: {nets[name].launch_info(1, N)[0]} on {nets[name].launch_kernel(1)} -->')
    assert nets['dw_dilated=1, ROWS 1'].launch_kernel(1) == f'f8::dwconvk_dil_dot4_kernel<{K}, 1>'
    assert nets['dw_dilated=1, ROWS 2'].launch_kernel(1) == f'f8::dwconvk_dil_dot4_kernel<{K}, 2>'
    assert nets['dw_dilated=2'].launch_kernel(1) == 'f8::dwconvk_kernel<false>' and nets['undilated dot4'].launch_kernel(1) == f'f8::dwconvk_dot4_kernel<{K}, 1>'
    for name in list(nets)[1:-1]:
        assert torch.equal(outs['dw_dilated=1'], outs[name]), f'{name} disagrees with dw_dilated=1'
    us = {name: [] for name in nets}
    for _ in range(args.reps):
        for name, net in nets.items():
            _, ms = net.run_profiled(x)
            us[name].append(ms[1] * 1e3)
    macs = K * K * C * H * H * N                                     # (pad d (K / 2): the map keeps its size)
    for name in nets:
        med = statistics.median(us[name])
        print(f'| {K}x{K} d{d}, {C} x {H} x {H} | {name} | {nets[name].launch_kernel(1)} | {med:.1f} ({min(us[name]):.1f} .. {max(us[name]):.1f}) | '
              f'{macs / 1e9:.2f} | {med * 1e3 / (macs / 1e6):.3f} |')


if __name__ == '__main__':
    main()
