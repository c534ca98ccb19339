#!/usr/bin/env python3
"""The windowed average pool (f8_net_avgpool_window, f8_sumpool.hip) on its two kernels against a device-to-device copy of the SOURCE's bytes.

    python tools/ab_avgpool.py [--reps 20] [--batch 128] [--md profiles/sumpool_r12.md]

Per row a net `input (8 ch) -> 1x1 conv to C, ReLU (the source, int32) -> pool -> 1x1 conv to 32 (an int8 reader)` is planned with split = 1 (one
launch per step: the step's time is one kernel's), twice: option sumpool_wide = 0 (`walker`: f8::sumpool_i32_kernel<K>) and 2 (`wide`:
f8::sumpool_wide_kernel).  A global window is the avgpool_sum node and has the one leg.  The measured value is the pool step's own time from
f8_net_run_profiled (HIP events around the launch).  The yardstick is `torch.Tensor.copy_` between two device buffers of the bytes the launch must
READ (N x H x W x C int32; it writes 1 / stride^2 of that in int8), timed with events in the same process, once behind every leg (copy, copy'): the
gap between the two is the spread the ratios are to be read against.  Legs alternate inside one process, `--reps` repetitions each after two
warm-up runs; median (min .. max).  The outputs of the two legs are compared bit for bit before anything is timed.  There is no parent leg: the
library before this entry point has no such node.  Nothing here is asserted about the ratios: they are written down.

Rows for the walker: DenseNet-121's three transitions (56^2 x 128, 28^2 x 256, 14^2 x 512; 2x2 / 2), Inception-3a's 28^2 x 192 at 3x3 / 1 / 1,
ResNet-D's 56^2 x 256 at 2x2 / 2, and 5x5 / 1 / 2, 7x7 / 1 / 3 on the Inception map (overlapping windows).  Rows for the walker / wide crossover:
PSP bins on the 60 x 60 x 2048 stage-3 map of resnet50_os8 at a 480 x 480 input — bins 1 / 2 / 3 / 6 (kernels 60 = the global window, 30, 20, 10)
and, to place the crossover, bins 10 / 12 / 15 / 20 (kernels 6 / 5 / 4 / 3).  That map is 29.5 MB per image in int32: the batch of those rows is cut to 32
(0.94 GB) to stay under the 2 GiB a tensor may have."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# (title, C, source H = W, kernel, stride, pad, batch cap)
ROWS = [('DenseNet-121 transition1', 128, 56, 2, 2, 0, None), ('DenseNet-121 transition2', 256, 28, 2, 2, 0, None),
        ('DenseNet-121 transition3', 512, 14, 2, 2, 0, None), ('Inception-3a pool branch', 192, 28, 3, 1, 1, None),
        ('ResNet-D shortcut', 256, 56, 2, 2, 0, None), ('overlapping 5x5', 192, 28, 5, 1, 2, None), ('overlapping 7x7', 192, 28, 7, 1, 3, None),
        ('PSP bin 1', 2048, 60, 60, 60, 0, 32), ('PSP bins 2', 2048, 60, 30, 30, 0, 32), ('PSP bins 3', 2048, 60, 20, 20, 0, 32),
        ('PSP bins 6', 2048, 60, 10, 10, 0, 32), ('PSP bins 10', 2048, 60, 6, 6, 0, 32), ('PSP bins 12', 2048, 60, 5, 5, 0, 32),
        ('PSP bins 15', 2048, 60, 4, 4, 0, 32), ('PSP bins 20', 2048, 60, 3, 3, 0, 32)]


def pool_net(C, H, k, s, pad, N, wide):
    net = F8Net().set_option('split', 1).set_option('sumpool_wide', wide)
    x = net.input(8, H, H, 8)
    w = np.clip(synth.rand_normal_int(1, f'w.{C}', (C, 8, 1, 1), 14.0), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(20, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
    src = net.conv(x, w, b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    pl = net.avgpool(src, k, s, pad, label='pool')
    w2 = np.clip(synth.rand_normal_int(40, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    net.output(net.conv(pl, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(('sumpool', 'avgpool_sum:'))]
    assert len(step) == 1, net.describe()
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_avgpool.py measures on the GPU'
    dev = torch.device('cuda:0')
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {args.batch} (PSP rows: 32)  reps {args.reps}', '',
             '| row | batch | leg | plan token | kernel | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---:|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, C, H, k, s, pad, cap in ROWS:
        N = min(args.batch, cap or args.batch)
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = (('global', 1),) if (k == H and pad == 0) else (('walker', 0), ('wide', 2))
        nets, outs = {}, {}
        for leg, wide in legs:
            nets[leg] = pool_net(C, H, k, s, pad, N, wide)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
        if len(legs) == 2:
            assert torch.equal(outs['walker'], outs['wide']), 'the two kernels disagree'
        nbytes = N * H * H * C * 4
        src = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy_us():
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3
        for _ in range(2):
            copy_us()
        names = [l for l, _ in legs]
        copies = ['copy', "copy'"][:len(names)]
        us = {n: [] for n in names + copies}
        for _ in range(args.reps):
            for leg, cp in zip(names, copies):
                net, step = nets[leg]
                _, ms = net.run_profiled(x)
                us[leg].append(ms[step] * 1e3)
                us[cp].append(copy_us())
        base = statistics.median([v for cp in copies for v in us[cp]])
        for leg in names + copies:
            med = statistics.median(us[leg])
            if leg in nets:
                net, step = nets[leg]
                tok, moved = net.launch_info(step, N)[0].split(':')[0], net.launch_info(step, N)[1]
                kern = net.launch_kernel(step)
            else:
                tok, moved, kern = '-', 2.0 * nbytes, 'torch.Tensor.copy_'
            row = (f'| {title}: {C} x {H}^2, {k}x{k} / {s} / {pad} | {N} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f} | {moved / med / 1e3:.0f} | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x, src, dst
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
