"""Case table of tests/test_gconv_xwide_plan.py and tests/test_gpu_gconv_xwide.py: grouped 3x3 convolutions at group widths 72 .. 256 (f8_gconvx.hip).  Graph,
reference (the CPU oracle per group), input and `plan` (with its `tap` cases) are tests/gconv_cases.py's and tests/gconv_wide_cases.py's; every case carries
gconv_wide = 0 and gconv_xwide = 1, so its leg `grouped = 2` is the dense expansion.

`npg` is the kernel instance's second argument, WRITTEN BY HAND from gconvx_tile: the patch pixel is 32 KS + 16 bytes (KS = ceil(cg / 32)), 64 KB hold
585 (cg 72) / 409 (cg 112 .. 128) / 315 (cg 168) / 240 (cg 232 .. 256) patch pixels; a tile is at most 256 output pixels (stride 2: 128, always <…, 4>); the
instance is 4 where a wave's share of the tile is at most four 32-pixel groups, else 8."""
import gconv_cases
from gconv_cases import _case

# (C, cg): odd groups start 8 mod 16 (a source offset the 16-byte fetch is not aligned to), three subtiles, the last live 8 / . / Cs = C / aligned / 16 pad channels / KS 8, the last subtile live 8 / .
SHAPES = ((144, 72), (240, 120), (224, 112), (256, 128), (336, 168), (464, 232), (512, 256))


def expect(case):
    """[(plan token, kernel symbol or its prefix)] of the case's grouped convs on leg grouped = 1, by hand: a stride-2 launch is always <2, 4>."""
    if not case['on_kernel']:
        return gconv_cases.expect(case, leg=2)
    return [(f'gconvx3x3s{s}:', f'f8::gconvx3x3_kernel<{s}, {case["npg"] if s == 1 else 4}>')
            for s in [case['stride']] + ([case['second']['stride']] if case.get('second') else [])]


def _c(H=9, W=11, stride=1, C=144, cg=72, npg=8, **kw):
    return _case(H, W, stride, C=C, cg=cg, npg=npg, opts={'gconv_wide': 0, 'gconv_xwide': 1}, **kw)


_SGN = dict(in_fl=7, in_signed=True, relu=False, b_mean=0.0, b_sig=2.0 ** 11)
# 9 x 11 / 1: two images (198 pixels, 7 groups) fit a tile up to cg 168 — where five subtiles on four waves split it in two parts of 4 and 3 groups: <1, 4> — and
# one image (99 pixels) above.  / 2: 5 x 6 outputs, 4 .. 1 images a tile
CASES = {f'cg{cg}_s{s}': _c(stride=s, C=C, cg=cg, npg=8 if cg <= 128 else 4) for C, cg in SHAPES for s in (1, 2)}
CASES.update({
    # more groups than one workgroup handles (every workgroup handles one): five groups with 24 pad channels / three groups, Cs = C / four groups, Cs = C, the
    # last starts 8 mod 16: its last 16-byte fetch ends 8 bytes past the pixel — past the tensor at the last pixel of the last image
    'c360_cg72': _c(C=360, cg=72), 'c384_cg128': _c(C=384, cg=128), 'c288_cg72': _c(C=288, cg=72),
    # geometry at C = 144, cg = 72, pitch 112 (gconv_cases.GEOMETRY's shapes, re-derived): 65 one-pixel images a tile, three live / 7 x 7 outputs, five images
    # gathered, three live / two column tiles of 35 (70 > 64) / row tiles: 256 pixels allow 7 rows of 33, six tiles, the last with 6 live rows (the pixel
    # bound, no longer the patch) / five gathered images, all live, 245 pixels in 8 groups / stride 2, 19 x 32 outputs: 128 pixels allow 4 rows (65520
    # patch bytes), five row tiles, the last with 3 live — with three groups (c216); at two groups gconvx_kernel_applies keeps a stride-2 map of more than one
    # tile on the expansion (measured slower, profiles/gconv_xwide_r20.md): that case stays, both legs dense against the oracle
    'g_1x1': _c(1, 1, w_sig=120.0, npg=4), 'g_pad0_9x9': _c(9, 9, pad=0), 'g_3x70': _c(3, 70, npg=4), 'g_41x33': _c(41, 33, N=2), 'g_7x7_n5': _c(7, 7, N=5),
    'g_s2_37x63': _c(37, 63, 2, N=2, on_kernel=False), 'g_s2_37x63_c216': _c(37, 63, 2, N=2, C=216),
    # cross-talk: a signed input that is zero outside one group, int32 out: every output channel outside the group is its bias
    'x_cg120': _c(C=240, cg=120, readers=None, only_group=1, **_SGN), 'x_cg72': _c(C=216, cg=72, readers=None, only_group=2, **_SGN),
    # the producer writes the int8 form the next launch fetches: grouped -> 1x1 -> grouped / 2
    'chain_cg72': _c(14, 14, readers=[(3, False)], second=dict(stride=2, m_in_fl=4, m_sig=8.0, m_bsig=2.0 ** 10, m_bmean=2.0 ** 11, in_fl=5, w_fl=5)),
})
for _k in (dict(C=144, cg=72), dict(stride=2, C=240, cg=120)):      # formats
    CASES.update({f'f_signed_cg{_k["cg"]}': _c(readers=[(4, True)], **_k, **_SGN), f'f_two_forms_cg{_k["cg"]}': _c(readers=[(4, False), (3, False)], **_k),
                  f'f_i32_and_i8_cg{_k["cg"]}': _c(tap=True, **_k), f'f_i32_cg{_k["cg"]}': _c(readers=None, **_k),
                  f'f_bias_big_cg{_k["cg"]}': _c(bias_big=True, **_k)})
CASES['batches'] = _c(stride=2, C=240, cg=120, max_batch=3, batches=[1, 2, 3])    # planned for 3 images, run with 1, 2 and 3 from the one handle
