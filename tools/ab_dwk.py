#!/usr/bin/env python3
"""A/B of the general depthwise launches (f8_dwk.hip): option dwk_dot4 = 1 (f8::dwconvk_dot4_kernel<K, S>) against 0 (f8::dwconvk_kernel), with
the 3x3 / pad 1 launch on v_dot4 (dw_mma = 0: f8::dwconv3x3_dot4_kernel) on the same map as a yardstick per multiply-add.

    python tools/ab_dwk.py [--reps 50] [--batch 128]

Per shape (the 5x5 / 7x7 depthwise layers of MnasNet-B1 / ProxylessNAS-class nets at 224 x 224) a net `input (C ch) -> depthwise K x K / S, ReLU -> 1x1 conv to 32`
is planned once per variant with split = 1 (one launch per step: the step's time is one kernel's); the measured value is the depthwise step's own
time from f8_net_run_profiled (HIP events around the launch), the variants alternating inside one process, `--reps` repetitions each after two
warm-up runs; the median is reported.  Bytes = the int8 input read once + the int8 output written once + the weights (channels padded to 32);
ops = 2 * K * K * C * P * Q * N.  The two general variants' outputs are compared with each other before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

SHAPES = [(5, 72, 56, 2), (5, 120, 28, 1), (5, 576, 14, 2), (5, 1152, 7, 1), (7, 144, 28, 1), (7, 480, 14, 1)]      # K, C, map, stride
VARIANTS = [('dwk_dot4=1', {'dwk_dot4': 1}, None), ('dwk_dot4=0', {'dwk_dot4': 0}, None), ('3x3 dot4', {'dw_mma': 0}, 3)]


def dw_net(K, C, H, stride, N, opts):
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    w = np.clip(synth.rand_normal_int(1, f'w.{K}.{C}', (C, 1, K, K), 90.0 / K), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(2, f'b.{C}', (C,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{C}', (32, C, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(C, H, H, 8)
    d = net.conv(t, w, b, stride=stride, pad=K // 2, groups=C, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    r = net.conv(d, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('dwconv')]
    assert len(step) == 1
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_dwk.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| shape | variant | kernel | µs median (min .. max) | MB | GB/s | GMAC | ns / MMAC |')
    print('|---|---|---|---|---:|---:|---:|---:|')
    for K, C, H, S in SHAPES:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, C, H, H), 0, 255).astype(np.int32)).to(dev)
        nets, outs = {}, {}
        for name, opts, k in VARIANTS:
            nets[name] = dw_net(k or K, C, H, S, N, opts)
            for _ in range(2):                                           # warm-up (upload, code objects)
                outs[name], _ = nets[name][0].run_profiled(x)
        assert nets['dwk_dot4=1'][0].launch_kernel(nets['dwk_dot4=1'][1]) == f'f8::dwconvk_dot4_kernel<{K}, {S}>'
        assert nets['dwk_dot4=0'][0].launch_kernel(nets['dwk_dot4=0'][1]) == 'f8::dwconvk_kernel<false>'
        assert nets['3x3 dot4'][0].launch_kernel(nets['3x3 dot4'][1]) == f'f8::dwconv3x3_dot4_kernel<{S}, 2>'
        assert torch.equal(outs['dwk_dot4=1'], outs['dwk_dot4=0']), 'the two kernels disagree'
        us = {name: [] for name in nets}
        for _ in range(args.reps):
            for name, (net, step) in nets.items():
                _, ms = net.run_profiled(x)
                us[name].append(ms[step] * 1e3)
        for name, _, k in VARIANTS:
            net, step = nets[name]
            _, nbytes, ops = net.launch_info(step, N)
            med = statistics.median(us[name])
            print(f'| {K}x{K} / {S}, {C} x {H} x {H} | {name} | {net.launch_kernel(step)} | {med:.1f} ({min(us[name]):.1f} .. {max(us[name]):.1f}) | '
                  f'{nbytes / 1e6:.1f} | {nbytes / med / 1e3:.0f} | {ops / 2e9:.2f} | {med * 1e3 / (ops / 2e6):.3f} |')
        del nets, outs, x


if __name__ == '__main__':
    main()
