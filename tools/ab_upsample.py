#!/usr/bin/env python3
"""The upsample launch (f8_net_upsample, f8_upsample.hip) in its modes against a device-to-device copy of the OUTPUT's bytes.

    python tools/ab_upsample.py [--reps 30] [--batch 128] [--md profiles/upsample_r10.md]

Per row a net `input (8 ch) -> 1x1 conv to C, ReLU (the source) -> upsample -> 1x1 conv to 32 (an int8 reader)` — the `logits` row: the upsample
itself is the output, int32 — is planned with split = 1 (one launch per step: the step's time is one kernel's), nearest rows twice: option
upsample_i8 = 1 (`upsample_nearest_i8:`, the byte copy) and 0 (`upsample_nearest_i32:`, the int32 source replicated and requantised in the launch).
The measured value is the upsample step's own time from f8_net_run_profiled (HIP events around the launch).  The yardstick is
`torch.Tensor.copy_` between two device buffers of the bytes the launch WRITES (N x P x Q x C int8, the logits row N x P x Q x Cs int32) — the
launch reads 1 / (sh sw) of that —, timed with events in the same process, once behind every leg (copy, copy'): the gap between the two is the
spread the ratios are to be read against.  Legs alternate inside one process, `--reps` repetitions each after two warm-up runs; median
(min .. max).  The outputs of the two nearest modes are compared bit for bit before anything is timed.  There is no parent leg: the library
before this entry point has no such node.

Rows: FPN top-down 256 x 14^2 -> 28^2 and 28^2 -> 56^2 (nearest x2), the ASPP broadcast 256 x 1^2 -> 14^2 and -> 28^2, DeepLab logits
21 x 14^2 -> 224^2 (bilinear x16, the output), a U-Net decoder step 64 x 56^2 -> 112^2 (bilinear x2, one int8 reader)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# (title, C, source H = W, scale, mode, the upsample is the output)
ROWS = [('FPN 14 -> 28', 256, 14, 2, 'nearest', False), ('FPN 28 -> 56', 256, 28, 2, 'nearest', False),
        ('ASPP broadcast 1 -> 14', 256, 1, 14, 'nearest', False), ('ASPP broadcast 1 -> 28', 256, 1, 28, 'nearest', False),
        ('DeepLab logits 14 -> 224', 21, 14, 16, 'bilinear', True), ('U-Net 56 -> 112', 64, 56, 2, 'bilinear', False)]


def up_net(C, H, scale, mode, is_out, N, i8):
    net = F8Net().set_option('split', 1).set_option('upsample_i8', i8)
    x = net.input(8, H, H, 8)
    w = np.clip(synth.rand_normal_int(1, f'w.{C}', (C, 8, 1, 1), 14.0), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(20, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
    src = net.conv(x, w, b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    up = net.upsample(src, scale, mode, label='up')
    if is_out:
        net.output(up, as_float=False)
    else:
        w2 = np.clip(synth.rand_normal_int(40, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
        net.output(net.conv(up, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('upsample_')]
    assert len(step) == 1, net.describe()
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_upsample.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| row | leg | plan token | kernel | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, C, H, scale, mode, is_out in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = (('i8', 1), ('i32', 0)) if mode == 'nearest' else (('i32', 1),)
        nets, outs = {}, {}
        for leg, i8 in legs:
            nets[leg] = up_net(C, H, scale, mode, is_out, N, i8)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
            assert nets[leg][0].launch_info(nets[leg][1], N)[0].startswith(f'upsample_{mode}_{leg}:'), nets[leg][0].describe()
        if len(legs) == 2:
            assert torch.equal(outs['i8'], outs['i32']), 'the two modes disagree'
        P = H * scale
        nbytes = N * P * P * ((C + 31) // 32 * 32 * 4 if is_out else C)
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
        us = {k: [] for k in names + copies}
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
            row = (f'| {title}: {C} ch, {mode} x{scale} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f} | {moved / med / 1e3:.0f} | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x, src, dst
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
