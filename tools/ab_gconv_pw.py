#!/usr/bin/env python3
"""A/B of the grouped 1x1 launches with cin != cout: option gconv_pw = 2 under grouped = 1 (f8::gconvp1x1_kernel<SB, KSM>, f8_gconvp.hip) against
gconv_pw = 0 (the dense expansion: conv_igemm_kernel over block-diagonal weights — the route and kernels every such conv had before), same commit.

    python tools/ab_gconv_pw.py [--batch 128] [--seconds 0.3] [--md profiles/gconv_pw_r24.md]

Per shape a net `input (cin ch) -> grouped 1x1, ReLU -> 1x1 conv to 32` is planned once per leg with split = 1 (one launch per step); the grouped step writes
one int8 form.  The measured value is the grouped step's own time from f8_net_run_profiled (HIP events around the launch), the legs alternating inside one
process after two warm-up runs each, as many repetitions as fill `--seconds` of the slower leg's whole run (at least 30); the median and the quartiles are
reported.  `pw faster` says whether the new launch's upper quartile lies below the expansion's lower quartile — by more than the spread of the repeated legs;
a shape where it does not belongs in gconvp_rule (f8_gconvp.hip).  The two legs' outputs are compared with each other before anything is timed.

`floor` is the launch's HBM floor computed here from the shapes: (N H W (Cs_in + Cs_out) + cout (cgi + 4)) bytes — the int8 input once, the int8 output
once, the groups' weights and biases, rows at their stored stride Cs = channels rounded up to 32 — over the 8.0 TB/s HBM3E peak; `share` = floor / time.

Shapes: the two grouped 1x1 convs of a ShuffleNet-V1 1.0x unit at g = 3 and g = 8 in its three stages (28 x 28, 14 x 14, 7 x 7); two-group expand / project
pairs of the MixNet kind, labelled by shape (no model zoo here to confirm a net); one awkward width, cgi 20 -> cgo 80."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

PEAK_BPS = 8.0e12
# label, cin, cout, groups, map
SHAPES = [(f'shufflenet-v1 g{g}', a, b, g, hw) for g, widths in ((3, (240, 480, 960)), (8, (384, 768, 1536)))
          for c, hw in zip(widths, (28, 14, 7)) for a, b in ((c, c // 4), (c // 4, c))]
SHAPES += [('two-group pair', a, b, 2, hw) for c, e, hw in ((40, 240, 28), (80, 480, 14), (120, 720, 14)) for a, b in ((c, e), (e, c))]
SHAPES += [('awkward width', 60, 240, 3, 14)]


def pw_net(cin, cout, groups, hw, N, pw):
    net = F8Net().set_option('split', 1).set_option('grouped', 1).set_option('gconv_pw', pw)
    cgi = cin // groups
    w = np.clip(synth.rand_normal_int(1, f'w.{cin}.{cout}', (cout, cgi, 1, 1), 90.0 / cgi ** 0.5), -127, 127).astype(np.int32)
    b = (synth.rand_normal_int(2, f'b.{cout}', (cout,), 2.0 ** 9) + 2 ** 12).astype(np.int32)
    w2 = np.clip(synth.rand_normal_int(3, f'w2.{cout}', (32, cout, 1, 1), 8.0), -127, 127).astype(np.int32)
    t = net.input(cin, hw, hw, 8)
    d = net.conv(t, w, b, stride=1, pad=0, groups=groups, weight_fl=5, input_fl=8, input_signed=False, quant_input=False, relu=True)
    r = net.conv(d, w2, None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    step, = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith('gconv')]
    return net, step


def floor_bytes(cin, cout, groups, hw, N):
    r32 = lambda c: (c + 31) // 32 * 32      # noqa: E731
    return N * hw * hw * (r32(cin) + r32(cout)) + cout * (cin // groups + 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--seconds', type=float, default=0.3)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_gconv_pw.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  at least {args.seconds} s a leg', '',
             '| shape | cgi -> cgo | kernel | reps | pw µs median (quartiles) | dense µs median (quartiles) | dense / pw | pw faster | floor µs | share of floor |',
             '|---|---|---|---:|---:|---:|---:|---|---:|---:|']
    print('\n'.join(lines), flush=True)
    gen = torch.Generator(device=dev).manual_seed(5)
    for label, cin, cout, groups, hw in SHAPES:
        x = torch.randint(0, 256, (N, cin, hw, hw), dtype=torch.int32, device=dev, generator=gen)
        nets, outs, whole = {}, {}, 0.0
        for name, pw in (('pw', 2), ('dense', 0)):
            nets[name] = pw_net(cin, cout, groups, hw, N, pw)
            for _ in range(2):                                           # warm-up (upload, code objects)
                outs[name], ms = nets[name][0].run_profiled(x)
            nets[name][0].check()
            whole = max(whole, sum(ms) * 1e-3)
        kern = nets['pw'][0].launch_kernel(nets['pw'][1])
        assert kern.startswith('f8::gconvp1x1_kernel<') and nets['pw'][0].launch_info(nets['pw'][1], N)[0].startswith('gconvp1x1s1:')
        assert nets['dense'][0].launch_info(nets['dense'][1], N)[0].startswith('gconv1x1s1_dense:')
        assert torch.equal(outs['pw'], outs['dense']), 'the two legs disagree'
        reps = max(30, min(2000, int(args.seconds / max(whole, 1e-6))))
        us = {name: [] for name in nets}
        for _ in range(reps):
            for name, (net, step) in nets.items():
                _, ms = net.run_profiled(x)
                us[name].append(ms[step] * 1e3)
        q = {name: statistics.quantiles(v, n=4) for name, v in us.items()}
        floor = floor_bytes(cin, cout, groups, hw, N) / PEAK_BPS * 1e6
        row = (f'| {label}: {cin} -> {cout}, g {groups}, {hw} x {hw} | {cin // groups} -> {cout // groups} | {kern} | {reps} | '
               + ' | '.join(f'{q[n][1]:.1f} ({q[n][0]:.1f} .. {q[n][2]:.1f})' for n in ('pw', 'dense'))
               + f' | {q["dense"][1] / q["pw"][1]:.2f} | {"yes" if q["pw"][2] < q["dense"][0] else "NO"} | {floor:.1f} | {floor / q["pw"][1]:.2f} |')
        print(row, flush=True)
        lines.append(row)
        del nets, outs, x
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
