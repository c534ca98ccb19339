#!/usr/bin/env python3
"""A/B of the rectangular conv launches (f8_net_conv_rect) against what the library could do without them: the kernel zero-embedded in the enclosing
square through the unchanged f8_net_conv / f8_net_conv_dilated, and — depthwise strips — the two kernels against each other and against a copy.

    python tools/ab_rect.py [--reps 30] [--batch 128] [--md profiles/rect_r18.md] [--only plain|strips]

Per shape a net `input (C ch) -> the conv, ReLU -> 1x1 conv to 32` is planned once per leg with split = 1 (one launch per step: the step's time is one
kernel's); the measured value is the conv step's own time from f8_net_run_profiled (HIP events around the launch), the legs alternating inside one
process, `--reps` repetitions each after two warm-up runs; median (min .. max) is reported.

Plain (Inception-v3's 1x7 / 7x1 at 17 x 17 with 128 / 160 / 192 channels, 1x3 / 3x1 at 8 x 8 with 384, ERFNet's 3x1 / 1x3 at dilation 2 at 64 x 128 with
128), legs:
    rect        the new path: conv_igemm_kernel over the kh x kw real taps
    embedded    the same taps in the centre row / column of a max(kh, kw) square of zeros at the same dilation, through f8_net_conv[_dilated]:
                max(kh, kw) / 1 times the K steps on the same kernel
Strips (C = 64 @ 64 x 64, 160 @ 32 x 32, 256 @ 16 x 16; k = 7 / 11 / 21, both orientations), legs:
    dot4        dwstrip_dot4_kernel (option dwk_dot4 = 1, the default)
    scalar      dwconvk_kernel (dwk_dot4 = 0)
    embedded    k = 7 only: the strip in the centre of a 7x7 depthwise kernel of zeros, which the library ran before (dwconvk_dot4_kernel<7, 1>)
    copy        torch.Tensor.copy_ of the int8 bytes the launch reads (N x H x W x Cs): the floor of a launch that reads its input and writes as much
The outputs of the legs of one shape are compared bit for bit before anything is timed.  MMAC = the real multiply-adds of the rectangular conv,
kh kw * cin/groups * cout * P * Q * N / 10^6, for every leg; Top/s = 2 MMAC / µs."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# C, H, W, kh, kw, dilation
PLAIN = [(C, 17, 17, kh, kw, 1) for C in (128, 160, 192) for kh, kw in ((1, 7), (7, 1))] + \
        [(384, 8, 8, 1, 3, 1), (384, 8, 8, 3, 1, 1), (128, 64, 128, 3, 1, 2), (128, 64, 128, 1, 3, 2)]
STRIPS = [(C, H, H, kh, kw, 1) for C, H in ((64, 64), (160, 32), (256, 16)) for k in (7, 11, 21) for kh, kw in ((1, k), (k, 1))]


def embedded(w):
    kh, kw = w.shape[2:]
    K = max(kh, kw)
    s = np.zeros(w.shape[:2] + (K, K), w.dtype)
    s[:, :, (K - kh) // 2:(K - kh) // 2 + kh, (K - kw) // 2:(K - kw) // 2 + kw] = w
    return s


def r_net(shape, N, depthwise, leg):
    C, H, W, kh, kw, d = shape
    net = F8Net().set_option('split', 1)
    if leg == 'scalar':
        net.set_option('dwk_dot4', 0)
    cin_g = 1 if depthwise else C
    w = np.clip(synth.rand_normal_int(1, f'w.{C}.{cin_g}.{kh}.{kw}', (C, cin_g, kh, kw), 150.0 / (kh * kw * cin_g) ** 0.5), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, W, 8)
    kwargs = dict(stride=1, groups=C if depthwise else 1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True, dilation=d)
    if leg == 'embedded':
        c = net.conv(t, embedded(w), b, pad=d * (max(kh, kw) // 2), **kwargs)
    else:
        c = net.conv(t, w, b, pad=(d * (kh // 2), d * (kw // 2)), **kwargs)
    r = net.conv(c, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(('conv', 'dwconv')) and not net.launch_info(i, N)[0].startswith('conv1x1')]
    assert len(step) == 1, net.describe()
    return net, step[0]


def copy_us(nbytes, reps, dev):
    a, b = torch.empty(nbytes, dtype=torch.int8, device=dev), torch.empty(nbytes, dtype=torch.int8, device=dev)
    out = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--only', choices=('plain', 'strips'), default=None)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_rect.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| shape | leg | plan token | kernel | µs median (min .. max) | MMAC | Top/s | first leg / leg |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for depthwise, shapes in ((False, PLAIN), (True, STRIPS)):
        if args.only and (args.only == 'strips') != depthwise:
            continue
        for shape in shapes:
            C, H, W, kh, kw, d = shape
            legs = (['dot4', 'scalar'] + (['embedded'] if max(kh, kw) == 7 else [])) if depthwise else ['rect', 'embedded']
            x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}.{W}', (N, C, H, W), 0, 255).astype(np.int32)).to(dev)
            nets, outs = {}, {}
            for leg in legs:
                nets[leg] = r_net(shape, N, depthwise, leg)
                for _ in range(2):                                       # warm-up (upload, code objects)
                    outs[leg], _ = nets[leg][0].run_profiled(x)
                nets[leg][0].check()
            for leg in legs[1:]:
                assert torch.equal(outs[legs[0]], outs[leg]), f'{leg} disagrees with {legs[0]} on {shape}'
            us = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg, (net, step) in nets.items():
                    _, ms = net.run_profiled(x)
                    us[leg].append(ms[step] * 1e3)
            mmac = nets[legs[0]][0].launch_info(nets[legs[0]][1], N)[2] / 2e6
            base = statistics.median(us[legs[0]])
            name = f'{"dw " if depthwise else ""}{C} x {H} x {W}, {kh}x{kw}{f" d{d}" if d > 1 else ""}'
            for leg in legs:
                net, step = nets[leg]
                med = statistics.median(us[leg])
                row = (f'| {name} | {leg} | {net.launch_info(step, N)[0].split(":")[0]} | {net.launch_kernel(step)} | '
                       f'{med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | {mmac:.0f} | {2 * mmac / med:.0f} | {base / med:.2f} |')
                print(row, flush=True)
                lines.append(row)
            if depthwise:
                cs = -(-C // 32) * 32
                cu = copy_us(N * H * W * cs, args.reps, dev)
                med = statistics.median(cu)
                row = f'| {name} | copy | | torch.Tensor.copy_ of {N * H * W * cs} B | {med:.1f} ({min(cu):.1f} .. {max(cu):.1f}) | | | {base / med:.2f} |'
                print(row, flush=True)
                lines.append(row)
            del nets, outs, x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
