#!/usr/bin/env python3
"""The multiply / hard-gate launches (f8_net_mul, f8_net_hard_gate, f8_mul.hip) against a device-to-device copy of the same bytes, and the launch with
the gate fused in against the two launches it replaces.

    python tools/ab_mul.py [--reps 30] [--batch 128] [--md profiles/mul_r14.md]

Per row a net `input (8 ch) -> 1x1 conv to C (the map x) -> op -> 1x1 conv to 32 (an int8 reader)` is planned with split = 1 (one launch per step: the
step's time is one kernel's) once per leg:
    SE rows        x (ReLU) -> avgpool_sum -> linear C -> C -> hard gate -> channel gate of x: fuse_hgate = 1 (`hgate+chmul_i8:`, one launch that reads the
                   N x C int32 gate sources) and 0 (`hgate:` + `chmul_i8:`; the value is the SUM of the two steps' times)
    h-swish rows   x -> mul(x, hard_gate(x)): fuse_hgate = 1 (`hgate+mul_i8:` on the I32T walker: 4 + 1 bytes read, 1 written per value) and 0 (`hgate:`
                   writes the gate in int8, `mul_i8:` reads two int8 forms: at least 3 bytes per value more, and a launch)
The measured value is the step's own time from f8_net_run_profiled (HIP events around the launch).  The yardstick is `torch.Tensor.copy_` between two
device buffers sized so that the copy moves what the FUSED leg moves (its launch_info bytes: half read, half written), timed with events in the same
process, twice per repetition (copy, copy'): the gap between the two is the spread the ratios are to be read against.  Legs alternate inside one
process, `--reps` repetitions each after two warm-up runs; median (min .. max).  The outputs of a row's legs are compared bit for bit before anything
is timed.  There is no parent leg: the library before these entry points refuses the graphs.

Shapes: MobileNet-V3-Large's — SE on 72 / 120 @ 28^2, 480 / 672 @ 14^2, 960 @ 7^2; hard-swish on 16 @ 112^2, 240 @ 14^2, 960 @ 7^2."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

ROWS = ([('SE scale', 'se', C, H) for C, H in ((72, 28), (120, 28), (480, 14), (672, 14), (960, 7))] +
        [('hard-swish', 'hswish', C, H) for C, H in ((16, 112), (240, 14), (960, 7))])
TOKENS = ('hgate', 'mul_', 'chmul_')


def _w(seed, shape, sig):
    return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)


def op_net(kind, C, H, N, opts):
    """Returns (net, [indices of the launches whose times are summed])."""
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    x = net.input(8, H, H, 8)
    b = (synth.rand_normal_int(21, f'b.{C}', (C,), 2.0 ** 12) + (2 ** 13 if kind == 'se' else 0)).astype(np.int32)
    src = net.conv(x, _w(1, (C, 8, 1, 1), 14.0), b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False,
                   relu=kind == 'se')                             # fraclen 13
    if kind == 'se':
        shift = 6 if H <= 8 else 8 if H <= 16 else 10             # log2 of the pooled pixels, rounded: the pooled mean stays an 8-bit value
        v = net.linear(net.avgpool_sum(src, shift), _w(2, (C, C), 40.0 / C ** 0.5), None, weight_fl=5, input_fl=4, input_signed=False, quant_input=True)
        t = net.mul(src, net.hard_gate(v), a_fl=4, a_signed=False, b_fl=5, label='op')
    else:
        t = net.hard_swish(src, x_fl=4, x_signed=True, g_fl=5, label='op')
    net.output(net.conv(t, _w(40, (32, C, 1, 1), 8.0), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=2, input_signed=kind != 'se'), as_float=False)
    net.finalize(N)
    steps = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(TOKENS)]
    assert steps, net.describe()
    return net, steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_mul.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| row | leg | plan tokens | kernels | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, kind, C, H in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = (('fused', dict(fuse_hgate=1)), ('two', dict(fuse_hgate=0)))
        nets, outs = {}, {}
        for leg, opts in legs:
            nets[leg] = op_net(kind, C, H, N, opts)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
        (la, _), (lb, _) = legs
        assert torch.equal(outs[la], outs[lb]), 'the two legs disagree'
        assert len(torch.unique(outs[la])) > 100, 'the row computes next to nothing'
        nbytes = int(sum(nets[la][0].launch_info(i, N)[1] for i in nets[la][1])) // 2      # the copy reads and writes this many: the fused leg's bytes moved
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
                net, steps = nets[leg]
                _, ms = net.run_profiled(x)
                us[leg].append(sum(ms[i] for i in steps) * 1e3)
                us[cp].append(copy_us())
        base = statistics.median(us['copy'] + us["copy'"])
        for leg in (la, lb, 'copy', "copy'"):
            med = statistics.median(us[leg])
            if leg in nets:
                net, steps = nets[leg]
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
