#!/usr/bin/env python3
"""A/B of the grouped 3x3 launches: option grouped = 1 (f8::gconv3x3_kernel<S>, f8_gconv.hip) against grouped = 2 (the dense expansion: the plain
conv kernels over block-diagonal weights), built from the same commit — nothing else exists to compare against.

    python tools/ab_gconv.py [--reps 50] [--batch 128] [--md profiles/gconv_r07.md]

Per shape (the grouped layers of ResNeXt-50 32x4d at 224 x 224) a net `input (C ch) -> grouped 3x3 / S in 32 groups, ReLU -> 1x1 conv to 32` is
planned once per leg with split = 1 (one launch per step: the step's time is one kernel's); the measured value is the grouped step's own time from
f8_net_run_profiled (HIP events around the launch), the legs alternating inside one process, `--reps` repetitions each after two warm-up runs; the
median is reported.  Bytes = the int8 input read once + the int8 output written once + the groups' weights (f8_net_launch_info, the same for both
legs); MMAC = the grouped multiply-adds, 9 * cg * C * P * Q * N / 10^6.  The two legs' outputs are compared with each other before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

SHAPES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]      # C, input map, stride
GROUPS = 32
LEGS = [('grouped=1', 1), ('grouped=2', 2)]


def g_net(C, H, stride, N, grouped):
    net = F8Net().set_option('split', 1).set_option('grouped', grouped)
    cg = C // GROUPS
    w = np.clip(synth.rand_normal_int(1, f'w.{C}', (C, cg, 3, 3), 30.0 / cg ** 0.5), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    d = net.conv(t, w, b, stride=stride, pad=1, groups=GROUPS, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    r = net.conv(d, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('gconv')]
    assert len(step) == 1
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_gconv.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| shape | leg | plan token | kernel | µs median (min .. max) | MB | GB/s | MMAC | ns / MMAC |', '|---|---|---|---|---|---:|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for C, H, S in SHAPES:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
        nets, outs = {}, {}
        for name, grouped in LEGS:
            nets[name] = g_net(C, H, S, N, grouped)
            for _ in range(2):                                           # warm-up (upload, code objects)
                outs[name], _ = nets[name][0].run_profiled(x)
            nets[name][0].check()
        assert nets['grouped=1'][0].launch_kernel(nets['grouped=1'][1]) == f'f8::gconv3x3_kernel<{S}>'
        assert nets['grouped=2'][0].launch_info(nets['grouped=2'][1], N)[0].startswith(f'gconv3x3s{S}_dense:')
        assert torch.equal(outs['grouped=1'], outs['grouped=2']), 'the two legs disagree'
        us = {name: [] for name in nets}
        for _ in range(args.reps):
            for name, (net, step) in nets.items():
                _, ms = net.run_profiled(x)
                us[name].append(ms[step] * 1e3)
        for name, _ in LEGS:
            net, step = nets[name]
            tok, nbytes, ops = net.launch_info(step, N)
            med = statistics.median(us[name])
            row = (f'| {C} x {H} x {H} / {S}, cg {C // GROUPS} | {name} | {tok.split(":")[0]} | {net.launch_kernel(step)} | {med:.1f} ({min(us[name]):.1f} .. {max(us[name]):.1f}) | '
                   f'{nbytes / 1e6:.1f} | {nbytes / med / 1e3:.0f} | {ops / 2e6:.0f} | {med * 1e3 / (ops / 2e6):.3f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
