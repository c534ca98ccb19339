#!/usr/bin/env python3
"""The transposed-conv launch (f8_net_conv_transpose, f8_deconv.hip) against the plain conv on conv_igemm_kernel that does the same multiply-adds.

    python tools/ab_deconv.py [--reps 20] [--batch 128] [--md profiles/deconv_r11.md]

Per row two nets over one source `input (8 ch) -> 1x1 conv to cin, ReLU`, planned with split = 1 (one launch per step: the step's time is one kernel's):
  deconv   source -> transposed conv k x k / s to cout [ReLU] -> a 1x1 int8 reader (leg `i8`), or the transposed conv itself as the int32 output (`i32`)
  conv     source -> the plain conv (k / s) x (k / s), stride 1, to s^2 cout channels at the input's resolution, options wstat = wreg = patch3x3 = 0 so
           that it runs conv_igemm_kernel: 1x1 to 4 cout for 2x2 / 2, 2x2 / pad 1 (an (H + 1)^2 map) for 4x4 / 2 / pad 1.  It reads the same input,
           does the same multiply-adds and writes the same number of output bytes (the 2x2 one (H + 1)^2 / H^2 of them).
The 3x3 / 2 / pad 1 / output_padding 1 row has no such twin (k / s is no integer): its achieved algorithmic ops/s stands beside the other rows'.
The measured value is the step's own time from f8_net_run_profiled (device events around the launch).  Legs alternate inside one process, `--reps`
repetitions each after two warm-up runs; median (min .. max).  The yardstick runs TWICE per repetition (conv, conv'): the gap between its two
medians is the spread the ratios are to be read against."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# (title, cin, cout, source H = W, k, s, pad, output_padding)
ROWS = [('U-Net 512x14 -> 256x28', 512, 256, 14, 2, 2, 0, 0), ('U-Net 256x28 -> 128x56', 256, 128, 28, 2, 2, 0, 0), ('U-Net 128x56 -> 64x112', 128, 64, 56, 2, 2, 0, 0),
        ('CenterNet 256x14 -> 256x28', 256, 256, 14, 4, 2, 1, 0), ('FCN scores 21x14 -> 21x28', 21, 21, 14, 4, 2, 1, 0),
        ('enc-dec 128x28 -> 64x56', 128, 64, 28, 3, 2, 1, 1)]


def _w(seed, shape, sig):
    return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)


def make_net(kind, cin, cout, H, k, s, pad, op, N, out32):
    net = F8Net().set_option('split', 1)
    for key in ('wstat', 'wreg', 'patch3x3'):
        net.set_option(key, 0)
    x = net.input(8, H, H, 8)
    b = (synth.rand_normal_int(20, f'b.{cin}', (cin,), 2.0 ** 9) + 2 ** 13).astype(np.int32)
    src = net.conv(x, _w(1, (cin, 8, 1, 1), 14.0), b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    fmt = dict(weight_fl=6, input_fl=4, input_signed=False, relu=True)
    if kind == 'deconv':
        t = net.conv_transpose(src, _w(2, (cin, cout, k, k), 4.0), None, stride=s, pad=pad, output_padding=op, label='step', **fmt)
        c2 = cout
    else:
        kc, c2 = k // s, s * s * cout
        t = net.conv(src, _w(2, (c2, cin, kc, kc), 4.0), None, stride=1, pad=kc - 1, groups=1, label='step', **fmt)
    if out32:
        net.output(t, as_float=False)
    else:
        net.output(net.conv(t, _w(3, (32, c2, 1, 1), 8.0), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False), as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].endswith(':step') and not net.launch_info(i, N)[0].startswith(('output', 'tap', 'requant'))]
    assert len(step) == 1, net.describe()
    if kind == 'conv':
        assert 'conv_igemm_kernel' in net.launch_kernel(step[0]), net.launch_kernel(step[0])
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_deconv.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
             '| row | form | leg | plan token | kernel | µs median (min .. max) | Gop (algorithmic) | Top/s | MB (algorithmic) | leg / conv |', '|---|---|---|---|---|---|---:|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, cin, cout, H, k, s, pad, op in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        twin = k % s == 0
        for form in ('i8', 'i32'):
            nets = {'deconv': make_net('deconv', cin, cout, H, k, s, pad, op, N, form == 'i32')}
            if twin:
                nets['conv'] = make_net('conv', cin, cout, H, k, s, pad, op, N, form == 'i32')
            for net, _ in nets.values():
                for _ in range(2):                                   # warm-up (upload, code objects)
                    net.run_profiled(x)
                net.check()
            legs = ['deconv'] + (['conv', "conv'"] if twin else [])
            us = {leg: [] for leg in legs}
            for _ in range(args.reps):
                for leg in legs:
                    net, step = nets[leg.rstrip("'")]
                    _, ms = net.run_profiled(x)
                    us[leg].append(ms[step] * 1e3)
            base = statistics.median(us['conv'] + us["conv'"]) if twin else None
            for leg in legs:
                net, step = nets[leg.rstrip("'")]
                name, moved, nops = net.launch_info(step, N)
                med = statistics.median(us[leg])
                row = (f'| {title}, {k}x{k} / {s} | {form} | {leg} | {name.split(":")[0]} | {net.launch_kernel(step)} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                       f'{nops / 1e9:.2f} | {nops / med / 1e6:.1f} | {moved / 1e6:.1f} | {"%.2f" % (med / base) if base else "-"} |')
                print(row, flush=True)
                lines.append(row)
            del nets
        del x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
