"""Case table of tests/test_gconv_pw_plan.py and tests/test_gpu_gconv_pw.py: grouped 1x1 convolutions, cin != cout allowed (f8_gconvp.hip).  Graph, reference
(the CPU oracle per group), input and `plan` (with its `tap` cases) are tests/gconv_cases.py's and tests/gconv_wide_cases.py's: `C` is cin, `cg` is
cgi = cin / groups, `cout` is given, cgo = cout / groups.  Every case carries gconv_pw = 2, so its leg `grouped = 2` is the dense expansion.

`inst`, BY HAND from f8_gconvp.hip: (16-byte slots where cgi % 8 == 0, else 4; KS = ceil(cgi / 32) rounded up to 1 / 2 / 4 / 8 / 16); None: outside the set,
dense on every leg.  Maps are 5 x 7 with N = 3 unless noted: 105 flat pixels in tiles of 32 that straddle the images, the last with 9 live."""
import numpy as np

import gconv_cases
from gconv_cases import _case
from ir_cases import _b, _w
from refgraph import RefGraph

OPTS = {'gconv_pw': 2}


def expect(case):
    """[(plan token, kernel symbol or its prefix)] of the case's grouped conv on leg grouped = 1, by hand."""
    if case['inst'] is None:
        return gconv_cases.expect(case, leg=2)
    return [('gconvp1x1s1:', 'f8::gconvp1x1_kernel<%d, %d>' % case['inst'])]


def _c(cin, cout, groups, inst, H=5, W=7, **kw):
    kw = dict(dict(K=1, pad=0, w_sig=120.0), **kw)
    return _case(H, W, C=cin, cg=cin // groups, cout=cout, inst=inst, opts=OPTS, on_kernel=inst is not None, **kw)


_SGN = dict(in_fl=7, in_signed=True, relu=False, b_mean=0.0, b_sig=2.0 ** 11)
_A, _B = (96, 384, 8, (4, 1)), (240, 60, 3, (16, 4))        # the two format shapes: cgi 12 -> cgo 48 / cgi 80 (KS 3) -> cgo 20, 4 pad channels
CASES = {
    # loaders, K steps: cgi 16 / 24, odd groups 8 mod 16 / 12 <-> 48 / 20 <-> 80, KS 3, 4 pad channels / cgi 40, KS 2; subtiles: cgo 12, 32 (c48_96), 48, 80
    'c48_48_g3': _c(48, 48, 3, (16, 1)), 'c72_24_g3': _c(72, 24, 3, (16, 1)), 'c96_384_g8': _c(*_A), 'c384_96_g8': _c(384, 96, 8, (16, 2)),
    'c60_240_g3': _c(60, 240, 3, (4, 1)), 'c240_60_g3': _c(*_B), 'c80_160_g2': _c(80, 160, 2, (16, 2)), 'c48_96_g3': _c(48, 96, 3, (16, 1)),
    # pixels: one / 578 in 19 tiles, the last with 2 live / one handle for 3 images at 1, 2, 3 / 32768, int32 only: the one size here with 64-pixel tiles (gconvp_plan)
    'p_1x1': _c(*_A, H=1, W=1, N=1), 'p_17x17': _c(*_B, H=17, W=17, N=2), 'batches': _c(*_A, max_batch=3, batches=[1, 2, 3]),
    'p_tile64': _c(8, 16, 2, (4, 1), H=128, W=128, N=2, readers=None, w_sig=60.0),
    # cross-talk: a signed input that is zero outside one group, int32 out: every output channel outside the group is its bias
    'x_g5': _c(*_A, readers=None, only_group=5, **_SGN),
    # outside the set, dense on every leg: cgi 6 / 516 / stride 2 / K 3 with cin != cout (cgo 20 with an int32 form: f_i32_c240, f_i32_and_i8_c240)
    'd_cgi6': _c(12, 8, 2, None), 'd_cgi516': _c(1032, 8, 2, None), 'd_s2': _c(48, 48, 3, None, stride=2, w_sig=80.0), 'd_k3': _c(48, 96, 3, None, K=3, pad=1, w_sig=40.0),
}
for _k in (_A, _B):                                         # formats; the int32 form is written per 8-channel group: cgo 20 stays on the expansion
    _i = _k[3] if _k[1] // _k[2] % 8 == 0 else None
    CASES.update({f'f_signed_c{_k[0]}': _c(*_k, readers=[(4, True)], **_SGN), f'f_two_forms_c{_k[0]}': _c(*_k, readers=[(4, False), (3, False)]),
                  f'f_i32_c{_k[0]}': _c(*_k[:3], _i, readers=None), f'f_i32_and_i8_c{_k[0]}': _c(*_k[:3], _i, tap=True),
                  f'f_bias_big_c{_k[0]}': _c(*_k, bias_big=True), f'f_no_relu_c{_k[0]}': _c(*_k, relu=False, readers=[(3, True)], b_mean=-2.0 ** 13, b_sig=2.0 ** 12)})

UNIT_EXPECT = [('gconvp1x1s1:', 'f8::gconvp1x1_kernel<16, 4>'), ('gconvp1x1s1:', 'f8::gconvp1x1_kernel<4, 1>')]


def unit(leg, opts=OPTS):
    """One ShuffleNet-V1 unit on 7 x 7, N = 2: grouped 1x1 240 -> 60 (g 3, ReLU) -> channel shuffle 3 -> depthwise 3x3 -> grouped 1x1 60 -> 240 (g 3) -> add with
    the unit's input.  The first conv writes int8 only (cgo 20); the second one's int32 form feeds the add: launch.  Returns (finalized graph, output)."""
    x = gconv_cases.make_input('unit', _c(240, 240, 3, None, H=7, W=7, N=2))
    g = RefGraph(x, 8, grouped=leg)
    t = next(iter(g.v))
    kw = dict(pad=0, groups=3, weight_fl=5, relu=True)
    a = g.conv(t, _w(60, (60, 80, 1, 1), 40.0), _b(61, 60, 2.0 ** 9, 2.0 ** 13), input_fl=8, input_signed=False, quant_input=False, **kw)
    d = g.conv(g.channel_shuffle(a, 3), _w(62, (60, 1, 3, 3), 30.0), _b(63, 60, 2.0 ** 9), pad=1, groups=60, weight_fl=5, input_fl=4, input_signed=False, relu=False)
    c = g.conv(d, _w(64, (240, 20, 1, 1), 60.0), _b(65, 240, 2.0 ** 9), input_fl=4, input_signed=True, **dict(kw, relu=False))
    out = g.add(c, t)
    g.net.output(out, as_float=False)
    for k, v in opts.items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    return g, out, x


def outside(case):
    """Output channels outside the live group of a cross-talk case: the mask is cgo's."""
    return np.arange(case['cout']) // (case['cout'] // (case['C'] // case['cg'])) != case['only_group']
