"""Case table, reference and graph builder of the tests of channel concatenation (f8_net_concat / `F8Net.concat`, f8_concat.hip):
tests/test_concat_plan.py (acceptance, refusals, mode tokens, kernel symbols, forms, launch_info, fused nets, the ONNX round trip; no GPU) and
tests/test_gpu_concat.py (every case on both legs, bit for bit on the device).  No test functions here.

The reference.  `ref_ops.concat_align(xs, fls)`: the result's fraclen is the largest operand fraclen and operand i contributes what the residual
join's alignment makes of it next to a zero partner, `oracle.add_align(zeros, x_i, out_fl, fl_i)` — shift left with the int32 wrap, clamp to
+-(2^31 - 1) — so nothing of that arithmetic is restated here; then `np.concatenate` along C.  `oracle/` stays as it is: refgraph.graph_forward
walks an imported ONNX graph with the same function.

Unless a builder says otherwise a case is  input (8 channels, 0 .. 255, fraclen 8) -> K 1x1 producer convs that read it as it is, couts C_i, weight
fraclens chosen to give the stated output fraclens -> concat -> readers: one 32-output 1x1 conv per (input_fl, signed), summed (as dil_cases).

The expected mode token and the ALIGNED flag of the kernel symbol of every case are WRITTEN BY HAND (the rule: DESIGN.md 4.5i); nothing here asks
the planner for them."""
import sys

import numpy as np

import graph_cases
from dil_cases import FUSE_ALL  # noqa: F401  (the tests take it from here)
from f8net_amd import synth
from graph_cases import launch_lines
from ir_cases import _b, _w

X_FL = 8


def producer(g, t, k, cout, n, *, w_fl, relu, in_fl=X_FL, in_signed=False, quant_input=False, kernel=1, seed=0, dilation=1):
    """Conv number k of a case: `cout` outputs from tensor t, scaled so that a right shift by n (the reader's, less the operand's alignment)
    fills 8 bits: accumulators around 2^n x 100 where 8-bit weights can reach that."""
    cin = g.v[t][0].shape[1]
    taps = kernel * kernel
    sig = float(np.clip(2.0 ** n * 100 / (128 * (cin * taps) ** 0.5), 0.4, 40.0))
    w = _w(100 + 7 * k + seed, (cout, cin, kernel, kernel), sig)
    b = _b(200 + 7 * k + seed, cout, 2.0 ** n * 20, 2.0 ** n * 40 if relu else 0.0)
    return g.conv(t, w, b, pad=dilation * (kernel // 2), groups=1, weight_fl=w_fl, input_fl=in_fl, input_signed=in_signed, relu=relu,
                  quant_input=quant_input, dilation=dilation)


def readers(g, t, fmts):
    """One 32-output 1x1 conv per (fraclen, signed) over tensor t, summed."""
    out = None
    C = g.v[t][0].shape[1]
    for k, (fl, sgn) in enumerate(fmts):
        r = g.conv(t, _w(90 + k, (32, C, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=fl, input_signed=sgn, relu=False, label=f'reader{k}')
        out = r if out is None else g.add(out, r)
    return out


# ---- the builders.  Each returns (output tensor ids in output order, [concat tensor ids])
def _plain(g, x0, c):
    """K producers -> concat -> readers (or the concat itself as the output)."""
    fmts = c['readers']
    shift = (max(c['w_fl']) + X_FL) - (fmts[0][0] if fmts else 4)            # the first reader's requant shift of the concat
    ps = [producer(g, x0, k, ci, shift - (max(c['w_fl']) - wf), w_fl=wf, relu=c['relu']) for k, (ci, wf) in enumerate(zip(c['C'], c['w_fl']))]
    cat = g.concat(ps, label='cat')
    if not fmts:
        g.output(cat, as_float=c.get('as_float', False))
        return [cat], [cat]
    out = readers(g, cat, fmts)
    g.output(out)
    return [out], [cat]


def _vec(g, x0, c):
    """[C, 1, 1] tensors: the input's average pool (fraclen 14) -> producers that requantise it to unsigned fraclen 8 (shift 6) -> concat -> reader."""
    p = g.avgpool_sum(x0)
    ps = [producer(g, p, k, ci, 9, w_fl=5, relu=True, quant_input=True) for k, ci in enumerate(c['C'])]
    cat = g.concat(ps, label='cat')
    out = readers(g, cat, c['readers'])
    g.output(out)
    return [out], [cat]


def _to_add(g, x0, c):
    """concat(32, 32) joined with a 64-channel conv of the input: the join reads int32."""
    ps = [producer(g, x0, k, 32, 9, w_fl=5, relu=True) for k in range(2)]
    cat = g.concat(ps, label='cat')
    other = producer(g, x0, 5, 64, 8, w_fl=4, relu=False)                  # fraclen 12 against 13: the join shifts it by 1
    out = readers(g, g.add(cat, other, relu=True), [(4, False)])
    g.output(out)
    return [out], [cat]


def _to_pool(g, x0, c):
    """concat(32, 17) read by the average pool (int32; output 1) and by a 3 / 1 / 1 max-pool with one int8 reader (output 0)."""
    ps = [producer(g, x0, k, ci, 9, w_fl=5, relu=True) for k, ci in enumerate(c['C'])]
    cat = g.concat(ps, label='cat')
    out = readers(g, g.maxpool(cat, 3, 1, 1), [(4, False)])
    g.output(out)
    pooled = g.avgpool_sum(cat)
    g.output(pooled)
    return [out, pooled], [cat]


def _raw(g, x0, c):
    """The net input itself (8 channels up to +-2^28 at fraclen 2) next to a conv of it at fraclen 9: nothing bounds the input, and its alignment
    shift of 7 wraps and clamps."""
    p = producer(g, x0, 0, 24, 5, w_fl=9, relu=False, in_fl=0, in_signed=True, quant_input=True)
    cat = g.concat([x0, p], label='cat')
    out = readers(g, cat, [(4, True)])
    g.output(out)
    return [out], [cat]


def _nested(g, x0, c):
    """DenseNet: 64 channels, then four times a 3x3 conv (32 outputs, fraclen 12) of the running concat (fraclen 13) appended to it.  The convs read
    it at unsigned fraclen 4 and 3 in turn, so every inner concat is a source in two formats."""
    run = producer(g, x0, 0, 64, 9, w_fl=5, relu=True)
    cats = []
    for k in range(4):
        fl = 4 - (k & 1)
        grow = producer(g, run, 1 + k, 32, 8, w_fl=12 - fl, relu=True, in_fl=fl, quant_input=True, kernel=3)
        run = g.concat([run, grow], label=f'dense{k}')
        cats.append(run)
    out = readers(g, run, [(4, False)])
    g.output(out)
    return [out], cats


def _shared(g, x0, c):
    """concat(A, B) and concat(B, C): B is read by two concats, A also by a conv in another format (signed fraclen 3)."""
    A, B, C = (producer(g, x0, k, 32, 9, w_fl=5, relu=False) for k in range(3))
    c1, c2 = g.concat([A, B], label='cat1'), g.concat([B, C], label='cat2')
    out = g.add(readers(g, c1, [(4, False)]), readers(g, c2, [(4, False)]))
    side = g.conv(A, _w(95, (32, 32, 1, 1), 8.0), None, pad=0, groups=1, weight_fl=6, input_fl=3, input_signed=True, relu=False)
    out = g.add(out, side)
    g.output(out)
    return [out], [c1, c2]


def _inception(g, x0, c):
    """Inception-3a on 192 input channels: 1x1 (64); 1x1 (96) -> 3x3 (128); 1x1 (16) -> 5x5 (32, a plain conv); max-pool 3 / 1 / 1 -> 1x1 (32)."""
    b1 = producer(g, x0, 0, 64, 9, w_fl=5, relu=True)
    b2 = producer(g, producer(g, x0, 1, 96, 9, w_fl=5, relu=True), 2, 128, 9, w_fl=9, relu=True, in_fl=4, quant_input=True, kernel=3)
    b3 = producer(g, producer(g, x0, 3, 16, 9, w_fl=5, relu=True), 4, 32, 9, w_fl=9, relu=True, in_fl=4, quant_input=True, kernel=5)
    b4 = producer(g, g.maxpool(x0, 3, 1, 1), 5, 32, 9, w_fl=5, relu=True)
    cat = g.concat([b1, b2, b3, b4], label='inception_3a')
    out = readers(g, cat, c['readers'])
    g.output(out)
    return [out], [cat]


def aspp_head(g, t):
    """DeepLab's ASPP without the image-pooling branch on tensor t: a 1x1 and three 3x3 at dilation 6 / 12 / 18, 64 outputs each, read at unsigned
    fraclen 4 -> concat -> 1x1 projection to 64 (its int32 result is the head's output).  Returns (projection, concat)."""
    bs = [producer(g, t, 0, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True)]
    bs += [producer(g, t, 1 + k, 64, 5, w_fl=5, relu=True, in_fl=4, quant_input=True, kernel=3, dilation=d) for k, d in enumerate((6, 12, 18))]
    cat = g.concat(bs, label='aspp.cat')
    return producer(g, cat, 6, 64, 9, w_fl=5, relu=True, in_fl=4, quant_input=True), cat


def _gapneg(g, x0, c):
    """Operands whose own shift is NEGATIVE: the producers read the input at lower fraclens (c['fmt']: (input_fl, weight_fl) per operand, input_fl 8 =
    as it is), so that n_i = n - (out.fl - fl_i) < 0 for the operands below the reader's fraclen — their producers write through the left-shift branch."""
    fls = [i + w for i, w in c['fmt']]
    n = max(fls) - c['readers'][0][0]
    ps = []
    for k, (ci, (i, w)) in enumerate(zip(c['C'], c['fmt'])):
        ni = n - (max(fls) - (i + w))
        cin = g.v[x0][0].shape[1]
        # 0 .. 255 >> (8 - i) in, times weights around +-2, summed over 8 channels: results that fill 8 bits once shifted by -ni
        wt = _w(300 + k, (ci, cin, 1, 1), float(np.clip(2.0 ** (ni + (8 - i)) * 0.3, 0.5, 20.0)))
        ps.append(g.conv(x0, wt, _b(310 + k, ci, 2.0 ** max(ni, 0) * 10, 2.0 ** max(ni, 0) * 20), pad=0, groups=1, weight_fl=w, input_fl=i, input_signed=False, relu=True,
                         quant_input=i != X_FL))
    cat = g.concat(ps, label='cat')
    out = readers(g, cat, c['readers'])
    g.output(out)
    return [out], [cat]


def _case(C, H, W, N, mode, aligned, build=_plain, **kw):
    """mode / aligned: the expected token and kernel instance with option concat_i8 = 1, by hand."""
    c = dict(C=list(C), H=H, W=W, N=N, mode=mode, aligned=aligned, build=build, w_fl=[5] * len(C), relu=True, readers=[(4, False)], cin=8, x_fl=X_FL)
    c.update(kw)
    return c


I8, I32 = 'concat_i8:', 'concat_i32:'
CASES = {
    'aligned2': _case((32, 64), 8, 8, 2, I8, True),
    'aligned5': _case((64,) * 5, 6, 6, 2, I8, True, relu=False, readers=[(4, True)]),
    'k8': _case((16,) * 8, 4, 4, 1, I8, True),                                  # offsets multiples of 16, not of 32
    'off8': _case((24, 40), 8, 8, 2, I8, False),
    'bytes': _case((3, 5, 9), 5, 5, 3, I8, False, cin=3),                       # 17 real channels, 15 pad channels; 75 pixels
    'shuffle': _case((58, 58), 7, 7, 3, I8, False),                             # 147 pixels; pad 12
    'straddle': _case((17, 32, 15), 7, 7, 2, I8, False),
    'vec': _case((40, 24), 7, 7, 4, I8, False, build=_vec),                     # the concat's map is 1 x 1: M = 4
    # operand fraclens 14 / 11 / 8, the reader at unsigned fraclen 8: n = 6 and n_i = 6, 3, 0
    'gap': _case((32, 32, 32), 8, 8, 2, I8, True, w_fl=[6, 3, 0], readers=[(8, False)]),
    # operand fraclens 11 / 7 / 4, the reader at unsigned fraclen 8: n = 3 and n_i = 3, -1, -4 (0 < n, n_i < 0)
    'gapneg': _case((32, 32, 32), 8, 8, 2, I8, True, build=_gapneg, fmt=[(8, 3), (5, 2), (4, 0)], readers=[(8, False)]),
    # operand fraclens 8 / 6 / 4, the reader at fraclen 8: n = 0 and n_i = 0, -2, -4 (n <= 0: both sides shift left)
    'gapneg0': _case((32, 32, 32), 8, 8, 2, I8, True, build=_gapneg, fmt=[(6, 2), (5, 1), (4, 0)], readers=[(8, False)]),
    'twoforms': _case((32, 48), 8, 8, 2, I8, True, relu=False, readers=[(3, True), (4, False)]),
    'threeforms': _case((32, 48), 8, 8, 2, I32, None, relu=False, readers=[(3, True), (4, False), (5, False)]),
    'to_add': _case((32, 32), 8, 8, 2, I32, None, build=_to_add),
    'to_out': _case((24, 40), 7, 7, 3, I32, None, readers=None),
    'to_out_f32': _case((24, 40), 7, 7, 3, I32, None, readers=None, as_float=True),
    'to_pool': _case((32, 17), 7, 7, 2, I32, None, build=_to_pool),
    'raw': _case((8, 24), 6, 6, 2, I32, None, build=_raw, x_fl=2, raw=True),
    'nested': _case((64, 32, 32, 32, 32), 8, 8, 2, I8, True, build=_nested),
    'shared': _case((32, 32, 32), 8, 8, 2, I8, True, build=_shared),
    'inception': _case((64, 128, 32, 32), 12, 12, 2, I8, True, build=_inception, cin=192),
}
I8_CASES = [k for k, c in CASES.items() if c['mode'] == I8]


def make_input(name, n=None):
    c = CASES[name]
    shape = (n or c['N'], c['cin'], c['H'], c['W'])
    if c.get('raw'):                                                           # up to +-2^28, and a band of small values
        x = synth.rand_uniform_int(5, f'catx{name}', shape, -2 ** 28, 2 ** 28).astype(np.int64)
        small = synth.rand_uniform_int(6, f'cats{name}', shape, -300, 300).astype(np.int64)
        x = np.where(small % 3 == 0, small, x)
        x.reshape(-1)[:4] = [2 ** 28, -2 ** 28, 2 ** 24, -2 ** 24]           # 2^24 << 7 = 2^31 wraps to -2^31, which the clamp moves
        return x.astype(np.int32)
    return synth.rand_uniform_int(5, f'catx{name}', shape, 0, 255).astype(np.int32)


def concat_lines(net):
    """[(launch index, plan token 'concat_i8:' / 'concat_i32:', kernel symbol)] of the handle's concat launches, in launch order."""
    return launch_lines(net, 'concat_')


def symbol(mode, aligned):
    return 'f8::concat_i32_kernel' if mode == I32 else f'f8::concat_i8_kernel<{"true" if aligned else "false"}>'


graph_cases.bind_cases(sys.modules[__name__])      # build_graph, reference, plan, int_graph
