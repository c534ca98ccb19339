#!/usr/bin/env python3
"""A/B of the depthwise transposed-conv launches (option dw_deconv): f8::dwdeconv_dot4_kernel<T> (dw_deconv = 1) against f8::dwdeconv_kernel (dw_deconv = 2) and
against what a caller could run before the option existed — the dense f8::deconv_kernel over diagonal-expanded weights [C, C, k, k] — and the distance to a
device copy of the output's bytes.

    python tools/ab_dwdeconv.py --shape I [--reps 30] [--batch 128]       (one shape per process: give each its own time limit)

Per shape a net `input (C ch) -> depthwise transposed conv k x k / s, pad (k - s) / 2, ReLU -> 1x1 conv to 32` is planned once per variant with split = 1; the
measured value is the transposed conv's own step time from f8_net_run_profiled (HIP events around the launch), the variants and the copy alternating inside
one process, `--reps` repetitions each after two warm-up runs; the median is reported.  MACs = k k C H W N for every variant (the dense kernel multiplies C
times as many).  The copy is torch's copy_ of N P Q Cs int8 bytes, device to device, between HIP events: it reads and writes what the launch only writes
(the launch reads 1 / s^2 of that).  The variants must give the same values, bit for bit, before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# C, input map, k, s: DLA-34's IDAUp / DLAUp upsamplers at a 512 x 512 input
SHAPES = [(128, 64, 4, 2), (256, 32, 4, 2), (512, 16, 4, 2), (64, 64, 4, 2), (64, 32, 8, 4)]


def dwd_net(C, H, k, s, N, opts, dense=False):
    net = F8Net().set_option('split', 1)
    for key, v in opts.items():
        net.set_option(key, v)
    w = np.clip(synth.rand_normal_int(1, f'w.{k}.{C}', (C, 1, k, k), 40.0 * s / k), -127, 127).astype(np.int32)
    if dense:                                                       # the same op at groups = 1: zeros off the diagonal
        wd = np.zeros((C, C, k, k), np.int32)
        wd[np.arange(C), np.arange(C)] = w[:, 0]
        w = wd
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    t = net.conv_transpose(t, w, b, stride=s, pad=(k - s) // 2, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True,
                           groups=1 if dense else C)
    r = net.conv(t, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    return net.finalize(N)                                          # launches: input, the transposed conv under test (1), the reader, output


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shape', type=int, required=True, help=f'0 .. {len(SHAPES) - 1}')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_dwdeconv.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    C, H, k, s = SHAPES[args.shape]
    T = -(-k // s)
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| shape | variant | kernel | µs median (min .. max) | GMAC | output GB/s |')
    print('|---|---|---|---|---:|---:|')
    x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
    variants = [('dw_deconv=1', {'dw_deconv': 1}, False), ('dw_deconv=2', {'dw_deconv': 2}, False), ('dense, diagonal weights', {}, True)]
    nets, outs = {}, {}
    for name, opts, dense in variants:
        nets[name] = dwd_net(C, H, k, s, N, opts, dense)
        for _ in range(2):                                           # warm-up (upload, code objects)
            outs[name], _ = nets[name].run_profiled(x)
    for name in nets:
        print(f'<!-- {name}: {nets[name].launch_info(1, N)[0]} on {nets[name].launch_kernel(1)} -->')
    assert nets['dw_deconv=1'].launch_kernel(1) == f'f8::dwdeconv_dot4_kernel<{T}>' and nets['dw_deconv=2'].launch_kernel(1) == 'f8::dwdeconv_kernel<false>'
    assert nets['dense, diagonal weights'].launch_kernel(1).startswith('f8::deconv_kernel')
    for name in list(nets)[1:]:
        assert torch.equal(outs['dw_deconv=1'], outs[name]), f'{name} disagrees with dw_deconv=1'
    out_bytes = N * (H * s) ** 2 * ((C + 31) // 32 * 32)
    src, dst = torch.zeros(out_bytes, dtype=torch.int8, device=dev), torch.empty(out_bytes, dtype=torch.int8, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        dst.copy_(src)
    us = {name: [] for name in list(nets) + ['copy of the output bytes']}
    for _ in range(args.reps):
        for name, net in nets.items():
            _, ms = net.run_profiled(x)
            us[name].append(ms[1] * 1e3)
        ev0.record()
        dst.copy_(src)
        ev1.record()
        torch.cuda.synchronize()
        us['copy of the output bytes'].append(ev0.elapsed_time(ev1) * 1e3)
    macs = k * k * C * H * H * N
    for name in us:
        med = statistics.median(us[name])
        kern = nets[name].launch_kernel(1) if name in nets else 'torch copy_ (read + write)'
        print(f'| {k}x{k} / {s}, {C} x {H}^2 -> {H * s}^2 | {name} | {kern} | {med:.1f} ({min(us[name]):.1f} .. {max(us[name]):.1f}) | '
              f'{macs / 1e9:.2f} | {out_bytes / med / 1e3:.0f} |')


if __name__ == '__main__':
    main()
