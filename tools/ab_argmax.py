#!/usr/bin/env python3
"""The argmax output launches (f8_net_output_argmax, f8_argmax.hip): the fused upsample + argmax launch against the two launches it replaces, and both
against what the library offered before — the upsample, the int32 copy-out of the full logits and torch.argmax(dim=1) on the device.

    python tools/ab_argmax.py [--reps 20] [--batch 128] [--md profiles/argmax_r16.md]

Per row a net `input (C x H x H, int32) -> [bilinear x s ->] class map` is planned with split = 1 once per leg:
    fused    fuse_argmax = 1: `upsample_bilinear+argmax_u8:` (rows with an upsample only)
    two      fuse_argmax = 0: `upsample_bilinear_i32:` + `argmax_u8:`; rows without an upsample: the `argmax_*:` launch alone
    parent   no argmax output: the upsampled logits are output 0 as int32 (`upsample_bilinear_i32:` + `output:`), then torch.argmax(dim=1) on the
             device over the [N, C, 224, 224] buffer.  Its time is the two steps' own times plus torch.argmax timed by events in the same repetition.
The input launch (NCHW -> the arena's int32 form) is the same on every leg and is not counted.  The measured value is the steps' own time from
f8_net_run_profiled (HIP events around each launch).  Legs alternate inside one process, `--reps` repetitions each after two warm-up runs; median
(min .. max).  The class maps of a row's legs are compared bit for bit before anything is timed (parent: torch.argmax's map; a tie may differ from
the lowest-index rule there, so the data is drawn without ties: distinct random values per pixel are overwhelmingly likely at 2^31 range and the
comparison would show one).  A row whose full int32 logits pass the library's 2 GiB-per-tensor bound at the batch runs every leg at the largest
halving of the batch that fits; the batch stands in the row."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# (title, C, source side, scale (0: no upsample), index type)
ROWS = [('DeepLab os16', 21, 14, 16, 'u8'), ('DeepLab os8', 21, 28, 8, 'u8'), ('ADE20K os8', 150, 28, 8, 'u8'), ('Cityscapes os4', 19, 56, 4, 'u8'),
        ('unfused 21 x 224^2', 21, 224, 0, 'u8'), ('classifier 1000', 1000, 1, 0, 'i32')]
TOKENS = ('upsample_', 'argmax_', 'output:')


def op_net(C, H, scale, dtype, N, leg):
    net = F8Net().set_option('split', 1).set_option('fuse_argmax', 1 if leg == 'fused' else 0)
    t = net.input(C, H, H, 8)
    if scale:
        t = net.upsample(t, scale, 'bilinear', label='seg')
    if leg == 'parent':
        net.output(t, as_float=False)
    else:
        net.output_argmax(t, dtype)
    net.finalize(N)
    steps = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(TOKENS)]
    assert steps, net.describe()
    return net, steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_argmax.py measures on the GPU'
    dev = torch.device('cuda:0')
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {args.batch}  reps {args.reps}', '',
             '| row | leg | plan tokens | kernels | µs median (min .. max) | MB moved (algorithmic) | leg / fused (or / two) |', '|---|---|---|---|---|---:|---:|']
    print('\n'.join(lines), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for title, C, H, scale, dtype in ROWS:
        # the two-launch and parent legs lay the full logits out in int32, channels padded to 32, below 2 GiB a tensor: such a row runs every leg at the
        # largest halving of the batch that fits (150 classes at 224 x 224: 32 images; the fused leg alone would take 128)
        N = args.batch
        while ((C + 31) // 32 * 32) * (H * (scale or 1)) ** 2 * 4 * N >= 2 ** 31:
            N //= 2
        lim = 2 ** 31 // (4 * scale * scale) - 1 if scale else 2 ** 31 - 1       # no interpolated sum wraps: the parent leg's torch.argmax sees the same order
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), -lim, lim).astype(np.int32)).to(dev)
        legs = (('fused',) if scale else ()) + ('two', 'parent')
        nets, maps = {}, {}
        for leg in legs:
            nets[leg] = op_net(C, H, scale, dtype, N, leg)
            for _ in range(2):                                       # warm-up (upload, code objects)
                y, _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
            P = H * (scale or 1)
            maps[leg] = torch.argmax(y.view(N, C, P, P), dim=1) if leg == 'parent' else y.view(N, P, P).to(torch.int64)
        for leg in legs[1:]:
            assert torch.equal(maps[legs[0]], maps[leg]), f'{title}: legs {legs[0]} and {leg} disagree'
        assert len(torch.unique(maps[legs[0]])) >= min(C, 10), 'the row computes next to nothing'
        del maps
        us = {leg: [] for leg in legs}
        for _ in range(args.reps):
            for leg in legs:
                net, steps = nets[leg]
                y, ms = net.run_profiled(x)
                t = sum(ms[i] for i in steps) * 1e3
                if leg == 'parent':
                    P = H * (scale or 1)
                    e0.record()
                    torch.argmax(y.view(N, C, P, P), dim=1)
                    e1.record()
                    e1.synchronize()
                    t += e0.elapsed_time(e1) * 1e3
                us[leg].append(t)
        base = statistics.median(us[legs[0]])
        for leg in legs:
            net, steps = nets[leg]
            med = statistics.median(us[leg])
            tok = ' + '.join(net.launch_info(i, N)[0].split(':')[0] for i in steps) + (' + torch.argmax' if leg == 'parent' else '')
            kern = ' + '.join(net.launch_kernel(i) for i in steps)
            moved = sum(net.launch_info(i, N)[1] for i in steps)
            row = (f'| {title}: {C} x {H}^2' + (f' x{scale}' if scale else '') + f' @ {N} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f}' + (' + torch' if leg == 'parent' else '') + f' | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, x
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
