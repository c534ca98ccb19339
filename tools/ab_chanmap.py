#!/usr/bin/env python3
"""The slice / channel-shuffle launches (f8_net_slice, f8_net_channel_shuffle, f8_chanmap.hip) against a device-to-device copy of the OUTPUT's bytes,
and the fused concat+shuffle launch against the two launches it replaces.

    python tools/ab_chanmap.py [--reps 30] [--batch 128] [--md profiles/chanmap_r13.md]

Per row a net `input (8 ch) -> 1x1 conv(s) to C, ReLU (the source / the concat's operands) -> op -> 1x1 conv to 32 (an int8 reader)` is planned with
split = 1 (one launch per step: the step's time is one kernel's) once per leg:
    shuffle rows   chanmap_i8 = 1 (`shuffle{g}_i8:`, bytes moved) and 0 (`shuffle{g}_i32:`, the int32 source gathered and requantised in the launch)
    slice rows     the same two legs of `slice_i8:` / `slice_i32:`, for the first half (offset 0: the 16-byte instance) and the second half of the channels
    fused rows     concat(C / 2, C / 2) -> shuffle 2 with fuse_shuffle = 1 (`concat+shuffle2_i8:`, one launch) and 0 (`concat_i8:` + `shuffle2_i8:`; the
                   value is the SUM of the two steps' times)
The measured value is the step's own time from f8_net_run_profiled (HIP events around the launch).  The yardstick is `torch.Tensor.copy_` between two
device buffers of N x H x W x C_out bytes, timed with events in the same process, twice per repetition (copy, copy'): the gap between the two is the
spread the ratios are to be read against.  Legs alternate inside one process, `--reps` repetitions each after two warm-up runs; median (min .. max).
The outputs of a row's legs are compared bit for bit before anything is timed.  There is no parent leg: the library before these entry points refuses
the graphs.

Shapes: ShuffleNet-V2 1.0x / 1.5x stage outputs — 116 @ 28^2, 232 @ 14^2, 464 @ 7^2, 176 @ 28^2, 352 @ 14^2 — and a 4-group shuffle of 232 @ 14^2 for the
general kernel instance."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

SHAPES = [(116, 28), (232, 14), (464, 7), (176, 28), (352, 14)]
# (title, kind, C, H, groups)
ROWS = ([('shuffle 2', 'shuffle', C, H, 2) for C, H in SHAPES] + [('shuffle 4', 'shuffle', 232, 14, 4)] +
        [('slice, first half', 'slice0', C, H, 0) for C, H in SHAPES] + [('slice, second half', 'slice1', C, H, 0) for C, H in SHAPES] +
        [('concat + shuffle 2', 'fused', C, H, 2) for C, H in SHAPES])


def _conv(net, src, cout, cin, seed, **kw):
    w = np.clip(synth.rand_normal_int(seed, f'w.{cout}.{cin}', (cout, cin, 1, 1), 14.0 if cin == 8 else 8.0), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(20 + seed, f'b.{cout}', (cout,), 2.0 ** 9) + 2 ** 13).astype(np.int32) if cin == 8 else None
    return net.conv(src, w, b, stride=1, pad=0, groups=1, **kw)


def op_net(kind, C, H, groups, N, opts):
    """Returns (net, [indices of the launches whose times are summed])."""
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    x = net.input(8, H, H, 8)
    first = dict(weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    if kind == 'fused':
        t = net.channel_shuffle(net.concat([_conv(net, x, C // 2, 8, 1 + k, **first) for k in range(2)], label='cat'), groups, label='op')
    else:
        src = _conv(net, x, C, 8, 1, **first)
        t = net.channel_shuffle(src, groups, label='op') if kind == 'shuffle' else net.slice(src, 0 if kind == 'slice0' else C // 2, C // 2 if kind == 'slice0' else C, label='op')
    cout = net.tensor_info(t)[0]
    net.output(_conv(net, t, 32, cout, 40, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(N)
    steps = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(('slice_', 'shuffle', 'concat'))]
    assert steps, net.describe()
    return net, steps, cout


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_chanmap.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| row | leg | plan tokens | kernels | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, kind, C, H, groups in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = (('fused', dict(fuse_shuffle=1)), ('two', dict(fuse_shuffle=0))) if kind == 'fused' else (('i8', dict(chanmap_i8=1)), ('i32', dict(chanmap_i8=0)))
        nets, outs = {}, {}
        for leg, opts in legs:
            nets[leg] = op_net(kind, C, H, groups, N, opts)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
        (la, _), (lb, _) = legs
        assert torch.equal(outs[la], outs[lb]), 'the two legs disagree'
        nbytes = N * H * H * nets[la][2]
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
        us = {k: [] for k in (la, 'copy', lb, "copy'")}
        for _ in range(args.reps):
            for leg, cp in ((la, 'copy'), (lb, "copy'")):
                net, steps, _ = nets[leg]
                _, ms = net.run_profiled(x)
                us[leg].append(sum(ms[i] for i in steps) * 1e3)
                us[cp].append(copy_us())
        base = statistics.median(us['copy'] + us["copy'"])
        for leg in (la, lb, 'copy', "copy'"):
            med = statistics.median(us[leg])
            if leg in nets:
                net, steps, _ = nets[leg]
                tok = ' + '.join(net.launch_info(i, N)[0].split(':')[0] for i in steps)
                moved = sum(net.launch_info(i, N)[1] for i in steps)
                kern = ' + '.join(net.launch_kernel(i) for i in steps)
            else:
                tok, moved, kern = '-', 2.0 * nbytes, 'torch.Tensor.copy_'
            row = (f'| {title}: {C} on {H} x {H} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f} | {moved / med / 1e3:.0f} | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x, src, dst
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
