#!/usr/bin/env python3
"""A/B of the copy-out launch of a network output beyond the first: option tap_tiled = 1 (f8::tap_kernel, f8_tap.hip: walks the 4 KB blocks of the
int32 source) against 0 (f8::output_kernel, which walks the destination — what such an output would run on without the new kernel).

    python tools/ab_tap.py [--reps 5] [--batch 128] [--net-steps 30]

Per shape (C x H x H at `--batch` images: 256 x 56 x 56, 1024 x 14 x 14, 2048 x 7 x 7) a net `input (32 ch) -> 1x1 conv to C (tapped) -> 1x1 conv to 32`
is planned twice; the measured value is the tap step's own time from f8_net_run_profiled (HIP events around the launch), the two plans alternating,
`--reps` repetitions each after one warm-up run.  Bytes = the int32 source (channels padded to 32) read once + the NCHW destination written once;
the share is of the 8.0 TB/s HBM3E peak.  Both plans' tapped tensors are compared with each other before anything is timed.
Then ResNet-50 at `--batch`: step time (events around `--net-steps` runs, three alternating repetitions) of the default plan and of the plan with its
four stage outputs tapped — what a backbone user pays."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth, topology        # noqa: E402
from f8net_amd.net import F8Net, build_net   # noqa: E402

SHAPES = [(256, 56), (1024, 14), (2048, 7)]
HBM_PEAK = 8.0e12


def tap_net(C, H, N, tiled):
    net = F8Net().set_option('tap_tiled', tiled).set_option('split', 1)      # one launch per step: the step's time is one kernel's
    w1 = np.clip(synth.rand_normal_int(1, f'w1.{C}', (C, 32, 1, 1), 30.0), -127, 127).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(2, f'w2.{C}', (32, C, 1, 1), 30.0), -127, 127).astype(np.int32)
    b1 = synth.rand_normal_int(3, f'b1.{C}', (C,), 2.0 ** 12).astype(np.int32)
    t = net.input(32, H, H, 6)
    c1 = net.conv(t, w1, b1, stride=1, pad=0, groups=1, weight_fl=6, input_fl=6, input_signed=True, relu=False)
    c2 = net.conv(c1, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, relu=False)
    net.output(c2, as_float=False)
    net.output(c1, as_float=False)
    net.finalize(N)
    step = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('tap:')]
    assert len(step) == 1
    return net, step[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--net-steps', type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_tap.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| shape | bytes (MB) | tap_tiled=0 output_kernel µs (median; all) | tap_tiled=1 tap_kernel µs (median; all) | speed-up | tap_kernel TB/s | share of 8.0 TB/s |')
    print('|---|---:|---|---|---:|---:|---:|')
    for C, H in SHAPES:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}', (N, 32, H, H), -127, 127).astype(np.int32)).to(dev)
        nets = {tiled: tap_net(C, H, N, tiled) for tiled in (0, 1)}
        outs = {tiled: torch.empty((N, C, H, H), dtype=torch.int32, device=dev) for tiled in (0, 1)}
        for tiled, (net, _) in nets.items():
            assert net.launch_kernel(nets[tiled][1]).startswith('f8::tap_kernel' if tiled else 'f8::output_kernel')
            net.run_profiled(x, outs=[outs[tiled]])                       # warm-up (upload, code objects)
        assert torch.equal(outs[0], outs[1]), 'the two kernels disagree'
        us = {0: [], 1: []}
        for _ in range(args.reps):
            for tiled in (0, 1):
                net, step = nets[tiled]
                _, ms = net.run_profiled(x, outs=[outs[tiled]])
                us[tiled].append(ms[step] * 1e3)
        Cs = (C + 31) // 32 * 32
        nbytes = N * H * H * (Cs + C) * 4
        med = {k: statistics.median(v) for k, v in us.items()}
        rate = nbytes / (med[1] * 1e-6)
        fmt = lambda v: ' '.join(f'{t:.1f}' for t in v)
        print(f'| {C} x {H} x {H} | {nbytes / 1e6:.1f} | {med[0]:.1f}; {fmt(us[0])} | {med[1]:.1f}; {fmt(us[1])} | {med[0] / med[1]:.2f}x | {rate / 1e12:.2f} | {100 * rate / HBM_PEAK:.0f} % |')
        del nets, outs, x
    # ResNet-50 with and without its stage outputs
    spec = topology.get('resnet50', normalize=True)
    params = synth.reference_params(spec, seed=1234)
    stages = {}
    for b in spec.blocks:
        stages[b.name.rsplit('_layer_', 1)[0]] = b.name
    taps = list(stages.values())
    x, _ = synth.make_input(spec, params, N, 224, seed=1)
    xt = torch.from_numpy(x).to(dev)
    plans = {'default': build_net(spec, params, N, 224), 'stage taps': build_net(spec, params, N, 224, taps=taps)}
    bufs = {k: ([torch.empty((N,) + o[:3], dtype=torch.int32, device=dev) for o in n.outputs[1:]] or None) for k, n in plans.items()}
    out = torch.empty((N, spec.num_classes), dtype=torch.float32, device=dev)
    for k, n in plans.items():
        for _ in range(3):
            n.run(xt, out=out, outs=bufs[k])
    torch.cuda.synchronize()
    times = {k: [] for k in plans}
    for _ in range(3):
        for k, n in plans.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.net_steps):
                n.run(xt, out=out, outs=bufs[k])
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.net_steps)
    print()
    for k, n in plans.items():
        print(f'resnet50 bs {N} [{k}]: {n.num_launches} planned launches, arena {n.arena_bytes / 1e6:.0f} MB, step ms (3 repetitions of {args.net_steps} runs): '
              + ' '.join(f'{t:.3f}' for t in times[k]) + f'  median {statistics.median(times[k]):.3f}')


if __name__ == '__main__':
    main()
