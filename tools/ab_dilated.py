#!/usr/bin/env python3
"""A/B of the dilated 3x3 launches (f8_net_conv_dilated) against what the library could do without them: the zero-stuffed (2d + 1)-square conv through
the unchanged f8_net_conv, and — plain convs — against the same layer undilated on the same kernel.

    python tools/ab_dilated.py [--reps 30] [--batch 128] [--md profiles/dilated_r08.md]

Per shape (the dilated layers of ResNet-50 at output stride 16 / 8 and of MobileNet-V2 at output stride 16 / 8, 224 x 224) a net
`input (C ch) -> 3x3 conv, ReLU -> 1x1 conv to 32` is planned once per leg with split = 1 (one launch per step: the step's time is one kernel's); the
measured value is the 3x3 step's own time from f8_net_run_profiled (HIP events around the launch), the legs alternating inside one process, `--reps`
repetitions each after two warm-up runs; median (min .. max) is reported.  Legs:

    dilated     the new path: conv_igemm_kernel with dilated taps / dwconv3x3_dil_dot4_kernel
    generic     depthwise only: the same conv with dwk_dot4 = 0 (dwconvk_kernel)
    stuffed     the (2d + 1)-square kernel, zero except at [::d, ::d], as a plain / depthwise conv through f8_net_conv: 25/9 (d = 2) or 81/9 (d = 4) of
                the multiply-adds and weight bytes.  A depthwise d = 4 has no such leg: a depthwise kernel of 9 is refused
    undilated   plain only, twice (undilated, undilated'): the same layer at dilation 1, pad 1, patch3x3 = 0 — the same instruction stream as `dilated`
                on other addresses; the gap between its two copies is the spread `dilated` is to be read against

The outputs of `dilated`, `generic` and `stuffed` are compared bit for bit before anything is timed.  MMAC = the real multiply-adds of the dilated
conv, 9 * cin/groups * C * P * Q * N / 10^6, for every leg: ns / MMAC compares the legs at equal useful work."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

PLAIN = [(512, 14, 2), (256, 28, 2), (512, 28, 2), (512, 28, 4)]                # C, map, dilation: ResNet-50 OS16 stage 3; OS8 stage 2, stage 3
DEPTHWISE = [(576, 14, 2), (960, 14, 2), (384, 28, 2), (384, 28, 4)]            # MobileNet-V2 OS16 stage 5 / 6; OS8 stage 3 .. 4


def stuffed(w, d):
    s = np.zeros(w.shape[:2] + (2 * d + 1, 2 * d + 1), w.dtype)
    s[:, :, ::d, ::d] = w
    return s


def d_net(C, H, d, N, depthwise, leg):
    net = F8Net().set_option('split', 1)
    if leg == 'generic':
        net.set_option('dwk_dot4', 0)
    if leg.startswith('undilated'):
        net.set_option('patch3x3', 0)
    cin_g = 1 if depthwise else C
    w = np.clip(synth.rand_normal_int(1, f'w.{C}.{cin_g}', (C, cin_g, 3, 3), 150.0 / (9 * cin_g) ** 0.5), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    kw = dict(stride=1, groups=C if depthwise else 1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    if leg == 'stuffed':
        c = net.conv(t, stuffed(w, d), b, pad=d, **kw)
    elif leg.startswith('undilated'):
        c = net.conv(t, w, b, pad=1, **kw)
    else:
        c = net.conv(t, w, b, pad=d, dilation=d, **kw)
    r = net.conv(c, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].split('x')[0] in ('conv3', 'conv5', 'conv9', 'dwconv3', 'dwconv5')]
    assert len(step) == 1, net.describe()
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_dilated.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| shape | leg | plan token | kernel | µs median (min .. max) | MMAC | ns / MMAC | dilated / leg |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for depthwise, shapes in ((False, PLAIN), (True, DEPTHWISE)):
        for C, H, d in shapes:
            legs = ['dilated'] + (['generic'] if depthwise else []) + (['stuffed'] if not (depthwise and d > 3) else []) + \
                   ([] if depthwise else ['undilated', "undilated'"])
            x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
            nets, outs = {}, {}
            for leg in legs:
                nets[leg] = d_net(C, H, d, N, depthwise, leg)
                for _ in range(2):                                       # warm-up (upload, code objects)
                    outs[leg], _ = nets[leg][0].run_profiled(x)
                nets[leg][0].check()
            tok = nets['dilated'][0].launch_info(nets['dilated'][1], N)[0]
            assert tok.startswith(f'dwconv3x3s1d{d}:' if depthwise else f'conv3x3s1d{d}_t'), tok
            for leg in ('generic', 'stuffed'):
                assert leg not in outs or torch.equal(outs['dilated'], outs[leg]), f'{leg} disagrees with the dilated leg'
            us = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, (net, step) in nets.items():
                    _, ms = net.run_profiled(x)
                    us[leg].append(ms[step] * 1e3)
            mmac = nets['dilated'][0].launch_info(nets['dilated'][1], N)[2] / 2e6
            base = statistics.median(us['dilated'])
            for leg in legs:
                net, step = nets[leg]
                med = statistics.median(us[leg])
                row = (f'| {"dw " if depthwise else ""}{C} x {H} x {H}, d {d} | {leg} | {net.launch_info(step, N)[0].split(":")[0]} | {net.launch_kernel(step)} | '
                       f'{med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | {mmac:.0f} | {med * 1e3 / mmac:.4f} | {base / med:.2f} |')
                print(row, flush=True)
                lines.append(row)
            del nets, outs, x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
