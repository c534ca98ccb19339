#!/usr/bin/env python3
"""A/B of the stride-1 max pools: f8::maxpool_tile_kernel<LEVELS> (f8_maxpool.hip; options maxpool_tile = 2 and fuse_spp = 1) against the launches every such
pool had before — f8::maxpool_i8x16_kernel per pool, and for the SPP / SPPF pyramid three of them plus `concat_i8:` — and the distance to a device copy
of the output's bytes.

    python tools/ab_maxpool_tile.py [--reps 30] [--batch 128] [--md FILE]

Per row a net `input (32 ch) -> 1x1 conv to C, ReLU (x, read at unsigned fraclen 4) -> the pool, or the pools and their concat -> 1x1 conv to 32` is planned once per leg with split = 1; the
measured value is the sum of the step times of the leg's pool / concat launches from f8_net_run_profiled (HIP events around each launch), the legs and the
copy alternating inside one process, `--reps` repetitions each after two warm-up runs; the median is reported with its range.  The copy is torch's copy_
of the launches' output bytes (N H W C for a pool, four times that for a pyramid), device to device, between HIP events.  The legs must give the same
values, bit for bit, before anything is timed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# C, map side: YOLOv5s / v8 SPPF, YOLOv5l SPPF, YOLOv3-SPP / v4, Inception's 3x3 / 1 / 1 pool, one 80 x 80 map
MAPS = [(256, 20), (512, 20), (512, 19), (192, 28), (128, 80)]
PYRAMIDS = [(256, 20, (5, 5, 5), True), (512, 20, (5, 5, 5), True), (512, 19, (5, 9, 13), False), (128, 80, (5, 5, 5), True)]
POOLS = [(C, H, (k,), False) for C, H in MAPS for k in (3, 5, 9, 13)]
TOKENS = ('maxpool_', 'concat_', 'spp')


def pool_net(C, H, ks, chain, N, opts):
    net = F8Net().set_option('split', 1)
    for key, v in opts.items():
        net.set_option(key, v)
    w0 = np.clip(synth.rand_normal_int(1, f'w0.{C}', (C, 32, 1, 1), 12.0), -127, 127).astype(np.int32)
    b0 = (synth.rand_normal_int(2, f'b0.{C}', (C,), 2.0 ** 13) + 2 ** 15).astype(np.int32)
    x = net.conv(net.input(32, H, H, 8), w0, b0, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    ts = [x]
    for k in ks:
        ts.append(net.maxpool(ts[-1] if chain else x, k, 1, k // 2))
    t = net.concat(ts) if len(ks) > 1 else ts[1]
    cr = (len(ks) + 1 if len(ks) > 1 else 1) * C
    w = np.clip(synth.rand_normal_int(3, f'w.{cr}', (32, cr, 1, 1), 8.0), -127, 127).astype(np.int32)
    r = net.conv(t, w, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, quant_input=True, relu=False)
    net.output(r, as_float=False)
    return net.finalize(N)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_maxpool_tile.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    rows = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '',
            '| shape | windows | tile µs median (min .. max) | parent µs median (min .. max) | parent / tile | copy µs | tile / copy |', '|---|---|---|---|---:|---:|---:|']
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for C, H, ks, chain in PYRAMIDS + POOLS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{C}.{H}', (N, 32, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = {'tile': {'maxpool_tile': 2, 'fuse_spp': 1}, 'parent': {}}
        nets, outs, steps = {}, {}, {}
        for name, opts in legs.items():
            nets[name] = pool_net(C, H, ks, chain, N, opts)
            steps[name] = [i for i in range(nets[name].num_launches) if nets[name].launch_info(i, N)[0].startswith(TOKENS)]
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[name], _ = nets[name].run_profiled(x)
        kern = {name: [nets[name].launch_kernel(i) for i in steps[name]] for name in nets}
        assert kern['tile'] == [f'f8::maxpool_tile_kernel<{len(ks)}>'] and kern['parent'][:len(ks)] == ['f8::maxpool_i8x16_kernel'] * len(ks), kern
        assert torch.equal(outs['tile'], outs['parent']), f'{C} x {H}^2 {ks}: the legs disagree'
        out_bytes = N * H * H * C * (len(ks) + 1 if len(ks) > 1 else 1)
        src, dst = torch.zeros(out_bytes, dtype=torch.int8, device=dev), torch.empty(out_bytes, dtype=torch.int8, device=dev)
        for _ in range(2):
            dst.copy_(src)
        us = {name: [] for name in list(nets) + ['copy']}
        for _ in range(args.reps):
            for name, net in nets.items():
                _, ms = net.run_profiled(x)
                us[name].append(sum(ms[i] for i in steps[name]) * 1e3)
            ev0.record()
            dst.copy_(src)
            ev1.record()
            torch.cuda.synchronize()
            us['copy'].append(ev0.elapsed_time(ev1) * 1e3)
        med = {name: statistics.median(v) for name, v in us.items()}
        cell = lambda n: f'{med[n]:.1f} ({min(us[n]):.1f} .. {max(us[n]):.1f})'      # noqa: E731
        rows.append(f'| {C} x {H}^2 | {"·".join(map(str, ks)) if chain else " / ".join(map(str, ks))} | {cell("tile")} | {cell("parent")} | '
                    f'{med["parent"] / med["tile"]:.2f} | {med["copy"]:.1f} | {med["tile"] / med["copy"]:.2f} |')
        print(rows[-1], flush=True)
        del nets, outs, src, dst, x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
