#!/usr/bin/env python3
"""A/B of the fused inverted-residual launch around a depthwise 5x5 / 7x7 (f8_irk.hip, option fuse_irk = 1) against the three launches it
replaces (fuse_irk = 0: conv1x1, dwconv<K>x<K>, conv1x1[_res]).

    python tools/ab_irk.py [--reps 50] [--batch 128]

Per shape (the 5x5 / 7x7 blocks of MnasNet-B1 / ProxylessNAS-class nets at 224 x 224) a net `input -> pre 1x1 -> block [joined with its input] -> 1x1
reader` is planned once per variant with split = 1 (one launch per step: a step's time is one kernel's), from the same library in the same process.
The measured values are the steps' own times from f8_net_run_profiled (HIP events around each launch): the fused step, and the SUM of the expand,
depthwise and project steps of the other plan.  The variants alternate, `--reps` repetitions each after three warm-up runs of each; medians are
reported (min .. max next to them).  The two plans' outputs are compared bit for bit before anything is timed.
recompute = expand rows the fused launch computes / rows of the map (row tiles recompute their halo rows; whole-image tiles do not)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth                  # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

# K, stride, map, cin, E, cout, joined
SHAPES = [(5, 2, 56, 24, 72, 40, False), (5, 1, 28, 40, 120, 40, True), (5, 2, 28, 40, 240, 80, False), (5, 1, 14, 80, 480, 80, True),
          (5, 2, 14, 96, 576, 192, False), (5, 1, 7, 192, 1152, 192, True), (7, 1, 28, 48, 144, 48, True), (7, 1, 14, 80, 480, 80, True)]


def _w(seed, shape, sig):
    return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)


def _b(seed, n, sig, mean):
    return (synth.rand_normal_int(seed, f'b{n}', (n,), sig) + int(mean)).astype(np.int32)


def block_net(K, S, H, cin, E, cout, join, N, fuse):
    net = F8Net().set_option('split', 1).set_option('fuse_irk', fuse)
    t = net.input(cin, H, H, 5)
    t = net.conv(t, _w(1, (cin, cin, 1, 1), 12.0 * (32.0 / cin) ** 0.5), _b(2, cin, 300.0, 0), stride=1, pad=0, groups=1, weight_fl=6, input_fl=5,
                 input_signed=True, quant_input=True, relu=False)
    e = net.conv(t, _w(3, (E, cin, 1, 1), 8.0 * (32.0 / cin) ** 0.5), _b(4, E, 2.0 ** 10, 2.0 ** 10), stride=1, pad=0, groups=1, weight_fl=6, input_fl=4,
                 input_signed=True, quant_input=True, relu=True)
    d = net.conv(e, _w(5, (E, 1, K, K), 60.0 / K), _b(6, E, 2.0 ** 9, 2.0 ** 12), stride=S, pad=K // 2, groups=E, weight_fl=6, input_fl=6,
                 input_signed=False, quant_input=True, relu=True)
    p = net.conv(d, _w(7, (cout, E, 1, 1), 6.0 * (192.0 / E) ** 0.5), _b(8, cout, 2.0 ** 11, 0), stride=1, pad=0, groups=1, weight_fl=6, input_fl=6,
                 input_signed=False, quant_input=True, relu=False)
    if join:
        p = net.add(p, t)
    r = net.conv(p, _w(9, (32, cout, 1, 1), 8.0), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, quant_input=True, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    toks = [net.launch_info(i, N)[0].split(':')[0] for i in range(net.num_launches)]
    if fuse:
        steps = [i for i, t in enumerate(toks) if t.startswith('fused_irk')]
        assert len(steps) == 1, toks
    else:
        dw = [i for i, t in enumerate(toks) if t.startswith(f'dwconv{K}x{K}')]
        assert len(dw) == 1 and toks[dw[0] - 1].startswith('conv1x1') and toks[dw[0] + 1].startswith('conv1x1'), toks
        steps = [dw[0] - 1, dw[0], dw[0] + 1]
    return net, steps, toks


def recompute(tok, K, S, H):
    """expand rows computed / rows of the map, from the tile token (R# rows per tile, G# whole images)."""
    if tok[0] == 'G':
        return 1.0
    R, Ho, pad = int(tok[1:]), (H - 1) // S + 1, K // 2
    rows = 0
    for p0 in range(0, Ho, R):
        r0 = p0 * S - pad
        rows += min(H, r0 + (R - 1) * S + K) - max(0, r0)
    return rows / H


def workgroups(tok, S, H, N):
    """grid of the fused launch: ceil(N / G) groups of whole images, or N * ceil(Ho / R) row tiles."""
    Ho = (H - 1) // S + 1
    return -(-N // int(tok[1:])) if tok[0] == 'G' else N * -(-Ho // int(tok[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_irk.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    print(f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}')
    print('| block | E x map / stride | tile | workgroups | chunks | recompute | fused kernel | fused µs median (min .. max) | three launches µs median (min .. max) '
          '| expand + depthwise + project µs | three / fused |')
    print('|---|---|---|---:|---:|---:|---|---|---|---|---:|')
    for K, S, H, cin, E, cout, join in SHAPES:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{cin}.{H}', (N, cin, H, H), -127, 127).astype(np.int32)).to(dev)
        on, s_on, t_on = block_net(K, S, H, cin, E, cout, join, N, 1)
        off, s_off, _ = block_net(K, S, H, cin, E, cout, join, N, 0)
        outs = {}
        for name, net in (('on', on), ('off', off)):
            for _ in range(3):                                           # warm-up (upload, code objects, the LDS opt-in)
                outs[name], _ = net.run_profiled(x)
        assert torch.equal(outs['on'], outs['off']), 'the two plans disagree'
        us_on, us_off, parts = [], [], [[], [], []]
        for _ in range(args.reps):
            _, ms = on.run_profiled(x)
            us_on.append(ms[s_on[0]] * 1e3)
            _, ms = off.run_profiled(x)
            us_off.append(sum(ms[i] for i in s_off) * 1e3)
            for k, i in enumerate(s_off):
                parts[k].append(ms[i] * 1e3)
        tok = t_on[s_on[0]].rsplit('_', 1)[1]
        m_on, m_off = statistics.median(us_on), statistics.median(us_off)
        print(f'| {K}x{K} / {S}, {cin} -> {E} -> {cout}{" + x" if join else ""} | {E} x {H} x {H} / {S} | {tok} | {workgroups(tok, S, H, N)} | {(E + 63) // 64} | '
              f'{recompute(tok, K, S, H):.2f} | {on.launch_kernel(s_on[0])} | {m_on:.1f} ({min(us_on):.1f} .. {max(us_on):.1f}) | '
              f'{m_off:.1f} ({min(us_off):.1f} .. {max(us_off):.1f}) | {" + ".join(f"{statistics.median(p):.1f}" for p in parts)} | {m_off / m_on:.2f} |', flush=True)
        del on, off, outs, x


if __name__ == '__main__':
    main()
