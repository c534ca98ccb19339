"""Case table of tests/test_gconv_wide_plan.py and tests/test_gpu_gconv_wide.py: grouped 3x3 convolutions at group widths 24 .. 64 (f8_gconvw.hip).  Graph,
reference (the CPU oracle per group) and input are tests/gconv_cases.py's; every case carries gconv_wide = 1, so its leg `grouped = 2` is the dense expansion."""
import gconv_cases
from gconv_cases import _case

SHAPES = ((48, 24), (80, 40), (96, 48), (112, 56), (128, 64))      # (C, cg): Cs 64 with a 16-channel pad unit / KS 2, an 8-channel live subtile, Cs 96 / . / Cs 128 / .


def expect(case):
    """[(plan token, kernel symbol)] of the case's grouped convs on leg grouped = 1, WRITTEN BY HAND: KS = ceil(cg / 32)."""
    return [(f'gconvw3x3s{s}:', f'f8::gconvw3x3_kernel<{s}, {(case["cg"] + 31) // 32}>')
            for s in [case['stride']] + ([case['second']['stride']] if case.get('second') else [])]


def plan(name, case, x, leg=1):
    """gconv_cases.plan; a `tap` case (for gconv_cases' join_i32, which holds at C = 32 only) marks the conv's own tensor as output 1: int32 next to int8."""
    g, out, ids = gconv_cases.build_graph(case, x, leg)
    if case.get('tap'):
        assert g.net.output(ids[0], as_float=False) == 1
    for k, v in case['opts'].items():
        g.net.set_option(k, v)
    g.net.finalize(case.get('max_batch') or x.shape[0])
    return g, out, ids


def _c(H=9, W=11, stride=1, C=48, cg=24, **kw):
    return _case(H, W, stride, C=C, cg=cg, opts={'gconv_wide': 1}, **kw)


_SGN = dict(in_fl=7, in_signed=True, relu=False, b_mean=0.0, b_sig=2.0 ** 11)
CASES = {f'cg{cg}_s{s}': _c(stride=s, C=C, cg=cg) for C, cg in SHAPES for s in (1, 2)}
CASES.update({
    # more units than a workgroup: five groups, the second workgroup with one live group and 8 pad channels / three groups, a half-live last workgroup
    'c120_cg24': _c(C=120, cg=24), 'c192_cg64': _c(C=192, cg=64),
    # geometry at C = 48, cg = 24 (the tiles: gconv_cases.GEOMETRY)
    'g_1x1': _c(1, 1, w_sig=120.0), 'g_pad0_9x9': _c(9, 9, pad=0), 'g_3x70': _c(3, 70), 'g_41x33': _c(41, 33, N=2), 'g_7x7_n5': _c(7, 7, N=5),
    'g_s2_37x63': _c(37, 63, 2, N=2),
    # cross-talk: a signed input that is zero outside one group, int32 out: every output channel outside the group is its bias
    'x_cg24': _c(C=96, cg=24, readers=None, only_group=2, **_SGN), 'x_cg40': _c(C=120, cg=40, readers=None, only_group=1, **_SGN),
    # the producer writes the int8 form the next launch fetches: grouped -> 1x1 -> grouped / 2
    'chain_cg24': _c(14, 14, readers=[(3, False)], second=dict(stride=2, m_in_fl=4, m_sig=8.0, m_bsig=2.0 ** 10, m_bmean=2.0 ** 11, in_fl=5, w_fl=5)),
})
for _k in (dict(C=48, cg=24), dict(stride=2, C=80, cg=40)):         # formats
    CASES.update({f'f_signed_cg{_k["cg"]}': _c(readers=[(4, True)], **_k, **_SGN), f'f_two_forms_cg{_k["cg"]}': _c(readers=[(4, False), (3, False)], **_k),
                  f'f_i32_and_i8_cg{_k["cg"]}': _c(tap=True, **_k), f'f_i32_cg{_k["cg"]}': _c(readers=None, **_k),
                  f'f_bias_big_cg{_k["cg"]}': _c(bias_big=True, **_k)})
CASES['batches'] = _c(stride=2, C=80, cg=40, max_batch=3, batches=[1, 2, 3])      # planned for 3 images, run with 1, 2 and 3 from the one handle
