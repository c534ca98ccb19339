#!/usr/bin/env python3
"""A/B of the large depthwise launches (kernel 8 .. 31, option dw_large): what dw_large = 1 plans (f8::dwlk_kernel<TC>, f8_dwlk.hip, where dwlk_rule
says so) against f8::dwconvk_kernel (dw_large = 2), with f8::dwconvk_dot4_kernel<7, 1> on the same map as a yardstick per multiply-add and, for the
one shape whose expanded weights fit (128 channels), the dense conv over diagonal-expanded weights — what a caller could run before the option existed.

    python tools/ab_dwlk.py --shape I [--reps 50] [--batch 128]       (one shape per process: give each its own time limit)

Per shape (RepLKNet-31B's four stages; 9x9 / 11x11 slices of a MixConv at 28 x 28 and 14 x 14) a net `input (C ch) -> depthwise K x K / 1, pad K / 2, ReLU ->
1x1 conv to 32` is planned once per variant with split = 1; the measured value is the depthwise step's own time from f8_net_run_profiled (HIP events around
the launch), the variants alternating inside one process, `--reps` repetitions each after two warm-up runs; the median is reported.  ops = 2 K K C P Q N.
For dwlk_kernel the issued matrix work is counted from its tile (dwlk_geom, f8_dwlk.hip, restated below): workgroups x CG channels x K rows x 2 TC MFMAs of
2 * 32^3 operations, over the nominal 5.03 POPS; LDS bytes per MFMA = (TC + 1) KB of B fragments per 2 TC MFMAs.  The dwlk / generic outputs are compared
with each other before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

SHAPES = [(31, 128, 56), (29, 256, 28), (27, 512, 14), (13, 1024, 7), (9, 96, 28), (11, 96, 28), (9, 160, 14), (11, 160, 14)]      # K, C, map
PEAK_OPS = 5.03e15                           # INT8 MFMA, nominal


def dw_net(K, C, H, N, opts, dense=False):
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    w = np.clip(synth.rand_normal_int(1, f'w.{K}.{C}', (C, 1, K, K), 90.0 / K), -127, 127).astype(np.int32)
    if dense:                                                       # [C][C][K][K], zero off the diagonal
        wd = np.zeros((C, C, K, K), np.int32)
        wd[np.arange(C), np.arange(C)] = w[:, 0]
        w = wd
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    d = net.conv(t, w, b, stride=1, pad=K // 2, groups=1 if dense else C, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    r = net.conv(d, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    return net, 1                                                   # launches: input, the conv under test, the reader, output


def dwlk_tile(K, Cs, P, Q, N, nq=1):
    """dwlk_geom's choice: (CG, TC, workgroups)."""
    RS = 16 if P <= 16 else 32
    G, IR = 32 // RS, RS + K - 1
    for budget in (80 << 10, 160 << 10):
        for cg in (32, 16):
            for tc in range(2 if Q > 32 else 1, 0, -1):
                if cg * G * IR * (32 * (tc + 1) + 16) + nq * 32 * (32 * tc * cg + 16) <= budget:
                    return cg, tc, -(-N // G) * (1 if G > 1 else -(-P // 32)) * -(-Q // (32 * tc)) * (Cs // cg)
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shape', type=int, required=True, help=f'0 .. {len(SHAPES) - 1}')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_dwlk.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    K, C, H = SHAPES[args.shape]
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| shape | variant | kernel | µs median (min .. max) | GMAC | ns / MMAC | issued MFMA share of peak | LDS B / MFMA |')
    print('|---|---|---|---|---:|---:|---:|---:|')
    x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
    variants = [('dw_large=1', K, {'dw_large': 1}, False), ('dw_large=2', K, {'dw_large': 2}, False), ('7x7 dot4', 7, {}, False)]
    if C * C * K * K <= 16 << 20:
        variants.append(('dense, expanded', K, {}, True))
    nets, outs = {}, {}
    for name, k, opts, dense in variants:
        nets[name] = dw_net(k, C, H, N, opts, dense)
        for _ in range(2):                                           # warm-up (upload, code objects)
            outs[name], _ = nets[name][0].run_profiled(x)
    for name in nets:
        print(f'<!-- {name}: {nets[name][0].launch_info(1, N)[0]} on {nets[name][0].launch_kernel(1)} -->')
    assert nets['dw_large=2'][0].launch_kernel(1) == 'f8::dwconvk_kernel<false>' and nets['7x7 dot4'][0].launch_kernel(1) == 'f8::dwconvk_dot4_kernel<7, 1>'
    assert torch.equal(outs['dw_large=1'], outs['dw_large=2']), 'the two kernels disagree'
    if 'dense, expanded' in outs:
        assert torch.equal(outs['dw_large=1'], outs['dense, expanded']), 'the dense expansion disagrees'
    us = {name: [] for name in nets}
    for _ in range(args.reps):
        for name, (net, step) in nets.items():
            _, ms = net.run_profiled(x)
            us[name].append(ms[step] * 1e3)
    for name, k, _, dense in variants:
        net, step = nets[name]
        macs = k * k * C * H * H * N
        med = statistics.median(us[name])
        share = lds = ''
        if net.launch_kernel(step).startswith('f8::dwlk_kernel'):
            cg, tc, wgs = dwlk_tile(K, -(-C // 32) * 32, H, H, N)
            share = f'{wgs * cg * K * 2 * tc * 2 * 32 ** 3 / (med * 1e-6) / PEAK_OPS:.3f}'
            lds = f'{(tc + 1) * 1024 // (2 * tc)}'
        print(f'| {k}x{k}, {C} x {H} x {H} | {name} | {net.launch_kernel(step)} | {med:.1f} ({min(us[name]):.1f} .. {max(us[name]):.1f}) | '
              f'{macs / 1e9:.2f} | {med * 1e3 / (macs / 1e6):.3f} | {share} | {lds} |')


if __name__ == '__main__':
    main()
