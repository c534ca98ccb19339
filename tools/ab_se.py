#!/usr/bin/env python3
"""The fused squeeze path of an SE branch (option fuse_se, `avgpool+fc+fc:` on f8::se_kernel, f8_se.hip) against the three launches it replaces,
the latter run by the PARENT commit's library (not by this tree with the key off).

    python tools/ab_se.py --parent-lib PATH/libf8net.so [--reps 30] [--rounds 3] [--batch 128] [--md profiles/se_r21.md]

Per shape a net `input (8 ch) -> 1x1 conv to C, ReLU (the map x) -> avgpool_sum -> linear C -> mid -> linear mid -> C -> hard gate -> channel gate of x ->
1x1 conv to 32` is planned with split = 1.  A leg is a fresh child process (`--leg fused`: this library, fuse_se = 2, every match; `--leg three`: F8NET_LIB = the
parent's library, no key) that walks every shape: two warm-up runs, then `--reps` runs of f8_net_run_profiled, the value the step's own time (HIP
events around the launch) — of the one fused step, or the SUM of `avgpool_sum:` and the two conv launches of the linears.  The fused leg also times
`torch.Tensor.copy_` of the map's int32 bytes (half read, half written) after every run.  The driver alternates the legs `--rounds` times (fused,
three, fused, three, ...) and reports the median over all of a leg's runs (min .. max).  Each leg prints a checksum of the net's output per shape;
the driver requires them equal.  Below the table it prints, per shape and leg, the kernels and every run's time: the raw samples.

The SE shapes of MobileNet-V3-Large and EfficientNet-B0 (channels @ map / squeeze width) are quoted FROM MEMORY: torchvision is not installed here."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('mbv3-l', 72, 28, 24), ('mbv3-l', 120, 28, 32), ('mbv3-l', 480, 14, 120), ('mbv3-l', 672, 14, 168), ('mbv3-l', 672, 7, 168), ('mbv3-l', 960, 7, 240),
          ('effnet-b0', 32, 112, 8), ('effnet-b0', 96, 56, 4), ('effnet-b0', 144, 56, 6), ('effnet-b0', 240, 28, 10), ('effnet-b0', 480, 14, 20),
          ('effnet-b0', 672, 14, 28), ('effnet-b0', 1152, 7, 48)]


def leg_main(args):
    import numpy as np
    import torch
    from f8net_amd import synth
    from f8net_amd.net import F8Net
    dev, N, fused = torch.device('cuda:0'), args.batch, args.leg == 'fused'

    def w(seed, shape, sig):
        return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)
    for _, C, H, mid in SHAPES:
        net = F8Net().set_option('split', 1)
        if fused:
            net.set_option('fuse_se', 2)
        x0 = net.input(8, H, H, 8)
        b = (synth.rand_normal_int(21, f'b.{C}', (C,), 2.0 ** 12) + 2 ** 13).astype(np.int32)
        x = net.conv(x0, w(1, (C, 8, 1, 1), 14.0), b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
        shift = 6 if H <= 8 else 8 if H <= 16 else 10 if H <= 32 else 12 if H <= 64 else 14      # log2 of the pooled pixels, rounded
        f1 = net.linear(net.avgpool_sum(x, shift), w(2, (mid, C), 40.0 / C ** 0.5), None, weight_fl=5, input_fl=4, input_signed=False, label='fc1')      # 9
        f2 = net.linear(f1, w(3, (C, mid), 40.0 / mid ** 0.5), None, weight_fl=6, input_fl=3, input_signed=True, label='fc2')                              # 9
        t = net.mul(x, net.hard_gate(f2), a_fl=4, a_signed=False, b_fl=5)
        net.output(net.conv(t, w(40, (32, C, 1, 1), 8.0), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=2, input_signed=False), as_float=False)
        net.finalize(N)
        names = [net.launch_info(i, N)[0] for i in range(net.num_launches)]
        steps = [i for i, n in enumerate(names) if (n.startswith('avgpool+fc+fc:') if fused else n.startswith('avgpool_sum:') or n.endswith((':fc1', ':fc2')))]
        assert len(steps) == (1 if fused else 3), net.describe()
        xt = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        for _ in range(2):
            out, _ = net.run_profiled(xt)
        net.check()
        half = N * H * H * ((C + 31) // 32 * 32) * 4 // 2
        src = torch.randint(0, 255, (half,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us, cp = [], []
        for _ in range(args.reps):
            _, ms = net.run_profiled(xt)
            us.append(sum(ms[i] for i in steps) * 1e3)
            if fused:
                e0.record()
                dst.copy_(src)
                e1.record()
                e1.synchronize()
                cp.append(e0.elapsed_time(e1) * 1e3)
        print(json.dumps(dict(C=C, H=H, mid=mid, us=us, copy=cp, sum=int(out.to(torch.int64).sum()), uniq=int(torch.unique(out).numel()),
                              tokens=' + '.join(names[i].split(':')[0] for i in steps), kernels=' + '.join(net.launch_kernel(i) for i in steps),
                              bytes=[net.launch_info(i, N)[1] for i in steps])), flush=True)
        del net, xt, src, dst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--leg', choices=('fused', 'three'), default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    if args.leg:
        return leg_main(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), 'ab_se.py needs the parent commit\'s libf8net.so (--parent-lib)'
    rows = {'fused': {}, 'three': {}}
    for _ in range(args.rounds):
        for leg in ('fused', 'three'):
            env = dict(os.environ)
            if leg == 'three':
                env['F8NET_LIB'] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg, '--reps', str(args.reps), '--batch', str(args.batch)], env=env,
                               capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout + r.stderr
            for line in r.stdout.splitlines():
                d = json.loads(line)
                k = (d['C'], d['H'], d['mid'])
                if k in rows[leg]:
                    rows[leg][k]['us'] += d['us']
                    rows[leg][k]['copy'] += d['copy']
                else:
                    rows[leg][k] = d
    lines = [f'batch {args.batch}  reps {args.reps} x rounds {args.rounds}, legs alternating as fresh processes; three = the parent commit\'s library', '',
             '| net | C @ map / mid | fused µs median (min .. max) | three launches µs median (min .. max) | three / fused | map MB (pool phase) | weights KB (fc1 + fc2) | copy_ of the map µs | fused / copy |',
             '|---|---|---:|---:|---:|---:|---:|---:|---:|']
    for netname, C, H, mid in SHAPES:
        f, t = rows['fused'][(C, H, mid)], rows['three'][(C, H, mid)]
        assert f['sum'] == t['sum'] and f['uniq'] == t['uniq'] > 100, ('the legs disagree', C, H, mid)
        mf, mt, mc = statistics.median(f['us']), statistics.median(t['us']), statistics.median(f['copy'])
        Cs = (C + 31) // 32 * 32
        wkb = ((mid + 31) // 32 * 32 * ((C + 15) // 16 * 16 + 4) + Cs * ((mid + 15) // 16 * 16 + 4)) / 1e3
        lines.append(f'| {netname} | {C} @ {H}² / {mid} | {mf:.1f} ({min(f["us"]):.1f} .. {max(f["us"]):.1f}) | {mt:.1f} ({min(t["us"]):.1f} .. {max(t["us"]):.1f}) | '
                     f'{mt / mf:.2f} | {args.batch * H * H * Cs * 4 / 1e6:.1f} | {wkb:.1f} | {mc:.1f} | {mf / mc:.2f} |')
    print('\n'.join(lines), flush=True)
    for _, C, H, mid in SHAPES:                                # the raw samples, in run order (the rounds concatenated)
        for leg in ('fused', 'three'):
            d = rows[leg][(C, H, mid)]
            print(f'\n{C} @ {H}^2 / {mid} {leg}: {d["tokens"]} on {d["kernels"]}\n  us: ' + ' '.join(f'{v:.1f}' for v in d['us']))
            if leg == 'fused':
                print('  copy_ us: ' + ' '.join(f'{v:.1f}' for v in d['copy']))
    if args.md:
        with open(args.md, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
