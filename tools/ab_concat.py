#!/usr/bin/env python3
"""The concat launch (f8_net_concat, f8_concat.hip) in both modes against a device-to-device copy of the same number of bytes.

    python tools/ab_concat.py [--reps 30] [--batch 128] [--md profiles/concat_r09.md]

Per row a net `input (8 ch) -> K 1x1 convs, ReLU (the operands) -> concat -> 1x1 conv to 32` is planned twice with split = 1 (one launch per step: the
step's time is one kernel's): option concat_i8 = 1 (`concat_i8:`, the byte gather) and 0 (`concat_i32:`, int32 operands aligned and requantised in the
launch).  The measured value is the concat step's own time from f8_net_run_profiled (HIP events around the launch).  The yardstick is
`torch.Tensor.copy_` between two device buffers of N x H x W x sum(C_i) bytes — what the i8 mode moves, it being a copy with a permuted destination —
timed with events in the same process, twice per repetition (copy, copy'): the gap between the two is the spread the ratios are to be read against.
Legs alternate inside one process, `--reps` repetitions each after two warm-up runs; median (min .. max).  The outputs of the two modes are compared
bit for bit before anything is timed.  There is no parent leg: the library before this entry point refuses the graph.

Rows: 5 x 256 on 28 x 28 (ASPP at output stride 8), (64, 128, 32, 32) on 28 x 28 (Inception 3a), (64, 32) on 56 x 56 (a DenseNet layer),
(58, 58) on 28 x 28 (ShuffleNet-class widths: the general kernel instance)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

ROWS = [('ASPP, OS 8', (256,) * 5, 28), ('Inception 3a', (64, 128, 32, 32), 28), ('DenseNet layer', (64, 32), 56), ('ShuffleNet widths', (58, 58), 28)]


def cat_net(Cs, H, N, i8):
    net = F8Net().set_option('split', 1).set_option('concat_i8', i8)
    x = net.input(8, H, H, 8)
    ts = []
    for k, c in enumerate(Cs):
        w = np.clip(synth.rand_normal_int(1 + k, f'w.{c}.{k}', (c, 8, 1, 1), 14.0), -127, 127).astype(np.int32)
        b = (synth.rand_normal_int(20 + k, f'b.{c}.{k}', (c,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
        ts.append(net.conv(x, w, b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True))
    cat = net.concat(ts, label='cat')
    w2 = np.clip(synth.rand_normal_int(40, f'w2.{sum(Cs)}', (32, sum(Cs), 1, 1), 8.0), -127, 127).astype(np.int32)
    net.output(net.conv(cat, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('concat_')]
    assert len(step) == 1, net.describe()
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_concat.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| row | leg | plan token | kernel | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, Cs, H in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        nets, outs = {}, {}
        for leg, i8 in (('i8', 1), ('i32', 0)):
            nets[leg] = cat_net(Cs, H, N, i8)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
            assert nets[leg][0].launch_info(nets[leg][1], N)[0].startswith(f'concat_{leg}:'), nets[leg][0].describe()
        assert torch.equal(outs['i8'], outs['i32']), 'the two modes disagree'
        nbytes = N * H * H * sum(Cs)
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
        us = {k: [] for k in ('i8', 'copy', 'i32', "copy'")}
        for _ in range(args.reps):
            for leg in ('i8', 'i32'):
                net, step = nets[leg]
                _, ms = net.run_profiled(x)
                us[leg].append(ms[step] * 1e3)
                us['copy' if leg == 'i8' else "copy'"].append(copy_us())
        base = statistics.median(us['copy'] + us["copy'"])
        for leg in ('i8', 'i32', 'copy', "copy'"):
            med = statistics.median(us[leg])
            if leg in nets:
                net, step = nets[leg]
                tok, moved = net.launch_info(step, N)[0].split(':')[0], net.launch_info(step, N)[1]
                kern = net.launch_kernel(step)
            else:
                tok, moved, kern = '-', 2.0 * nbytes, 'torch.Tensor.copy_'
            row = (f'| {title}: {Cs if len(set(Cs)) > 1 else f"{len(Cs)} x {Cs[0]}"} on {H} x {H} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f} | {moved / med / 1e3:.0f} | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x, src, dst
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
