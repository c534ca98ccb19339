"""Rectangular convolutions (f8_net_conv_rect) without a GPU: the reference of tests/rect_cases.py pinned to torch's float64 conv with tuple arguments
behind F.pad, and to the zero-embedded square through oracle.conv2d; what the builder accepts and refuses, each with its status and the words of its
message; square + symmetric through the new entry point = the node f8_net_conv_dilated records; the plan token and kernel symbol of every case against
the hand-written table; the bias classes of the asymmetric 2x4 case from its masks; liveness of every case on the reference; the ONNX round trip."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import rect_cases
from f8net_amd import _lib, onnx_export, onnx_import, onnx_io, synth
from f8net_amd.net import F8Net
from oracle import oracle

F8_ERR_INVALID, F8_ERR_UNSUPPORTED, F8_ERR_STATE = -1, -2, -5
ALL = rect_cases.ALL
_w, _b = rect_cases._w, rect_cases._b


def _geometries():
    """(kh, kw, stride, pads, d) of every case of the table, once each."""
    return sorted({(c['kh'], c['kw'], c['stride'], c['pads'], c['d']) for c in ALL.values()})


# ---- the reference
@pytest.mark.parametrize('groups', [1, 8])
@pytest.mark.parametrize('kh, kw, stride, pads, d', _geometries())
def test_the_reference_is_torchs_float64_conv_behind_an_explicit_pad(kh, kw, stride, pads, d, groups):
    """float64 is exact here: |acc| <= 21 * 8 * 255 * 127 + 2^20 << 2^53."""
    C, H, W = 8, 11, 36
    x = synth.rand_uniform_int(1, f'rpin_x{kh}{kw}', (2, C, H, W), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(2, f'rpin_w{kh}{kw}{groups}', (C, C // groups, kh, kw), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(3, 'rpin_b', (C,), 3e5).astype(np.int32)
    got = rect_cases.rect_conv_ref(x, w, b, stride, pads, groups, d)
    t, l, bo, r = pads
    xp = torch.nn.functional.pad(torch.from_numpy(x).double(), (l, r, t, bo))
    want = torch.nn.functional.conv2d(xp, torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=stride, padding=0, dilation=d,
                                      groups=groups).numpy()
    assert got.shape == want.shape == (2, C, rect_cases.out_size(H, kh, stride[0], t, bo, d), rect_cases.out_size(W, kw, stride[1], l, r, d))
    np.testing.assert_array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize('groups', [1, 8])
@pytest.mark.parametrize('kh, kw', [(1, 7), (7, 1), (1, 3), (3, 1), (3, 5), (1, 15), (21, 1), (1, 11)])
def test_the_reference_is_the_kernel_zero_embedded_in_the_enclosing_square(kh, kw, groups):
    """Odd k, symmetric 'same' pads: the kh x kw taps in the centre of a max(kh, kw) square of zeros, at pad max(kh, kw) // 2, through oracle.conv2d —
    what a user could run before."""
    C, K = 8, max(kh, kw)
    x = synth.rand_uniform_int(1, f'remb_x{kh}{kw}', (2, C, 9, 13), 0, 255).astype(np.int32)
    w = synth.rand_uniform_int(2, f'remb_w{kh}{kw}{groups}', (C, C // groups, kh, kw), -127, 127).astype(np.int32)
    b = synth.rand_normal_int(3, 'remb_b', (C,), 3e5).astype(np.int32)
    sq = np.zeros((C, C // groups, K, K), np.int32)
    sq[:, :, (K - kh) // 2:(K - kh) // 2 + kh, (K - kw) // 2:(K - kw) // 2 + kw] = w
    got = rect_cases.rect_conv_ref(x, w, b, 1, (kh // 2, kw // 2), groups)
    np.testing.assert_array_equal(got, oracle.conv2d(x, sq, b, 1, K // 2, groups))


# ---- the builder
def _net(kh=1, kw=7, stride=1, pad=(0, 3), dilation=1, groups=1, C=16, H=16, W=16, grouped=None):
    net = F8Net()
    if grouped is not None:
        net.set_option('grouped', grouped)
    t = net.input(C, H, W, 8)
    t = net.conv(t, np.ones((C, C // groups, kh, kw), np.int32), None, stride=stride, pad=pad, groups=groups, weight_fl=4, input_fl=8, input_signed=False,
                 quant_input=False, relu=True, dilation=dilation)
    net.output(t, as_float=False)
    return net


def _tokens(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


@pytest.mark.parametrize('kh, kw, stride, pad, d, token', [
    (1, 7, 1, (0, 3), 1, 'conv1x7s1_t'), (7, 1, 1, (3, 0), 1, 'conv7x1s1_t'), (1, 31, 1, (0, 15), 1, 'conv1x31s1_t'), (31, 1, 2, (30, 0, 0, 0), 1, 'conv31x1s2_t'),
    (3, 1, 1, (2, 0), 2, 'conv3x1s1d2_t'), (1, 3, 1, (0, 0, 0, 128), 64, 'conv1x3s1d64_t'), (3, 5, (2, 1), (1, 2), 1, 'conv3x5s2x1_t'),
    (3, 5, (1, 3), (2, 4, 0, 1), 1, 'conv3x5s1x3_t'), (2, 4, 1, (0, 1, 1, 2), 1, 'conv2x4s1_t'), (3, 3, 2, (0, 0, 1, 1), 1, 'conv3x3s2_t'),
    (3, 3, 1, (1, 1, 1, 0), 3, 'conv3x3s1d3_t'), (1, 1, (2, 1), 0, 1, 'conv1x1s2x1_t'), (1, 1, (1, 5), 0, 7, 'conv1x1s1x5_t'), (5, 2, (4, 4), (4, 1, 0, 0), 1, 'conv5x2s4_t'),
])
def test_plain_rectangles_are_accepted(kh, kw, stride, pad, d, token):
    H, W = 16, 16 if d < 64 else 140
    net = _net(kh, kw, stride, pad, d, H=H, W=W).finalize(2)
    tok = [t for t in _tokens(net) if t.startswith('conv')]
    assert len(tok) == 1 and tok[0].startswith(token), net.describe()
    (sh, sw), (t, l, b, r) = rect_cases.pair(stride), rect_cases.pads4(pad)
    d = 1 if kh == kw == 1 else d
    assert net.outputs[0][:3] == (16, rect_cases.out_size(H, kh, sh, t, b, d), rect_cases.out_size(W, kw, sw, l, r, d))
    assert 'f8::conv_igemm_kernel<' in net.launch_kernel([i for i, t in enumerate(_tokens(net)) if t.startswith('conv')][0])


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('kh, kw, pad', [(1, 3, (0, 1)), (3, 1, (2, 0, 0, 0)), (1, 7, 0), (21, 1, (10, 0)), (1, 31, (0, 30, 0, 30)), (11, 1, (5, 0, 3, 0))])
def test_depthwise_strips_are_accepted(stride, kh, kw, pad):
    net = _net(kh, kw, stride, pad, groups=16, H=32, W=32).finalize(2)
    tok = [t for t in _tokens(net) if t.startswith('dwconv')]
    assert len(tok) == 1 and tok[0].startswith(f'dwconv{kh}x{kw}s{stride}:'), net.describe()


@pytest.mark.parametrize('kw, status, words', [
    # depthwise rectangles that are no strip, a dilated strip, per-axis strides: not built, the message names the geometry
    (dict(kh=3, kw=5, pad=(1, 2), groups=16), F8_ERR_UNSUPPORTED, ('depthwise', 'strips', 'kernel 3 x 5')),
    (dict(kh=1, kw=3, pad=(0, 2), dilation=2, groups=16), F8_ERR_UNSUPPORTED, ('depthwise', 'kernel 1 x 3', 'dilation 2')),
    (dict(kh=1, kw=7, stride=(1, 2), groups=16), F8_ERR_UNSUPPORTED, ('depthwise', 'stride (1, 2)')),
    (dict(kh=1, kw=7, stride=(3, 3), pad=(0, 1, 0, 0), groups=16), F8_ERR_UNSUPPORTED, ('depthwise', 'stride (3, 3)')),
    (dict(kh=1, kw=2, pad=0, groups=16), F8_ERR_UNSUPPORTED, ('depthwise', 'kernel 1 x 2')),
    # grouped: whatever the option says
    (dict(groups=4, C=32), F8_ERR_UNSUPPORTED, ('grouped rectangular', 'groups 4', 'kernel 1 x 7')),
    (dict(groups=4, C=32, grouped=1), F8_ERR_UNSUPPORTED, ('grouped rectangular', 'groups 4')),
    (dict(groups=4, C=32, grouped=2), F8_ERR_UNSUPPORTED, ('grouped rectangular',)),
    # numbers outside the rules
    (dict(kh=1, kw=32, pad=(0, 3)), F8_ERR_INVALID, ('kernel 1 x 32', '1 .. 31')),
    (dict(kh=0, kw=3, pad=0), F8_ERR_INVALID, ('kernel 0 x 3',)),
    (dict(stride=(0, 1)), F8_ERR_INVALID, ('stride (0, 1)', 'strides')),
    (dict(pad=(0, -1, 0, 3)), F8_ERR_INVALID, ('left -1', 'pads')),
    (dict(pad=(0, 7, 0, 3)), F8_ERR_INVALID, ('left 7', 'extent', '6 columns')),
    (dict(pad=(1, 3, 0, 3)), F8_ERR_INVALID, ('top 1', 'extent', '0 rows')),          # a 1-wide axis takes no pad
    (dict(kh=3, kw=1, pad=(2, 0, 5, 0), dilation=2), F8_ERR_INVALID, ('bottom 5', 'dilation 2', '4 rows')),
    (dict(dilation=0), F8_ERR_INVALID, ('dilation 0',)),
    (dict(dilation=65, W=600), F8_ERR_UNSUPPORTED, ('dilation 65', '64')),
    (dict(kh=1, kw=7, pad=0, W=5), F8_ERR_INVALID, ('empty output', '1 x 7', '16 x 5')),
    (dict(kh=3, kw=1, pad=(2, 0, 2, 0), dilation=12, H=16), F8_ERR_INVALID, ('empty output', 'spans 25 x 1')),
])
def test_refusals_name_the_geometry(kw, status, words):
    with pytest.raises(_lib.F8Error) as e:
        _net(**kw)
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert 'f8_net_conv_rect' in str(e.value)


def _raw(net, t, desc, geom, w):
    return net._L.f8_net_conv_rect(net._h, t, None if desc is None else ctypes.byref(desc), None if geom is None else ctypes.byref(geom), w.ctypes.data, None)


def _desc(**kw):
    d = dict(cin=16, cout=16, kernel=0, stride=0, pad=0, groups=1, weight_fl=4, input_fl=8, input_signed=0, quant_input=0, relu=1)
    d.update(kw)
    return _lib.ConvDesc(**d)


def _geom(kh=1, kw=7, sh=1, sw=1, pads=(0, 3, 0, 3), d=1):
    return _lib.ConvGeom(kh=kh, kw=kw, stride_h=sh, stride_w=sw, pad_top=pads[0], pad_left=pads[1], pad_bottom=pads[2], pad_right=pads[3], dilation=d)


def test_null_desc_null_geom_a_desc_with_a_geometry_and_a_finalized_net():
    net = F8Net()
    t = net.input(16, 8, 8, 8)
    w = np.ones((16, 16, 1, 7), np.int32)
    assert _raw(net, t, None, _geom(), w) == F8_ERR_INVALID and 'null desc' in net._L.f8_last_error().decode()
    assert _raw(net, t, _desc(), None, w) == F8_ERR_INVALID and 'null geom' in net._L.f8_last_error().decode()
    for bad in (dict(kernel=7), dict(stride=1), dict(pad=3)):
        assert _raw(net, t, _desc(**bad), _geom(), w) == F8_ERR_INVALID
        msg = net._L.f8_last_error().decode()
        assert 'must be 0' in msg and f"{list(bad)[0]} {list(bad.values())[0]}" in msg, msg
    o = _lib.check(_raw(net, t, _desc(), _geom(), w))
    net.output(o, as_float=False)
    net.finalize(2)
    assert _raw(net, t, _desc(), _geom(), w) == F8_ERR_STATE


@pytest.mark.parametrize('groups, k, pad, d', [(1, 3, 1, 1), (1, 3, 2, 2), (1, 1, 0, 5), (16, 3, 1, 1), (16, 5, 2, 1), (16, 3, 2, 2), (1, 7, 3, 1)])
def test_square_and_symmetric_through_the_new_entry_point_is_the_old_node(groups, k, pad, d):
    def build(rect):
        net = F8Net()
        t = net.input(16, 12, 12, 8)
        w = (np.arange(16 * (16 // groups) * k * k, dtype=np.int32).reshape(16, 16 // groups, k, k) % 13) - 6
        if rect:
            t = _lib.check(_raw(net, t, _desc(groups=groups), _geom(k, k, 1, 1, (pad,) * 4, d), w))
        else:
            dd = _desc(kernel=k, stride=1, pad=pad, groups=groups)
            t = _lib.check(net._L.f8_net_conv_dilated(net._h, t, ctypes.byref(dd), d, w.ctypes.data, None))
        net.output(t, as_float=False)
        return net.finalize(4)
    a, b = build(True), build(False)
    assert a.describe() == b.describe()
    assert [a.launch_kernel(i) for i in range(a.num_launches)] == [b.launch_kernel(i) for i in range(b.num_launches)]
    assert a.weight_bytes == b.weight_bytes and a.arena_bytes == b.arena_bytes


def test_a_resnet_block_through_the_new_entry_point_fuses_as_ever():
    """An identity bottleneck (1x1 -> 3x3 -> 1x1, join, ReLU) recorded through f8_net_conv_rect with square, symmetric geometries: the same fused plan."""
    C, MID = 512, 128

    def build(rect):
        net = F8Net()
        x = net.input(C, 28, 28, 4)

        def conv(t, cin, cout, k, pad, relu, seed):
            w = _w(seed, (cout, cin, k, k), 30.0)
            if not rect:
                return net.conv(t, w, None, stride=1, pad=pad, groups=1, weight_fl=6, input_fl=4, input_signed=False, relu=relu)
            d = _desc(cin=cin, cout=cout, weight_fl=6, input_fl=4, quant_input=1, relu=int(relu))
            return _lib.check(_raw(net, t, d, _geom(k, k, 1, 1, (pad,) * 4), w))
        pre = conv(x, C, C, 1, 0, True, 1)
        t = conv(conv(conv(pre, C, MID, 1, 0, True, 2), MID, MID, 3, 1, True, 3), MID, C, 1, 0, False, 4)
        net.output(net.add(t, pre, relu=True), as_float=False)
        for k, v in rect_cases.FUSE_ALL.items():
            net.set_option(k, v)
        return net.finalize(4)
    a, b = build(True), build(False)
    assert a.describe() == b.describe() and any(t.startswith('fused_') for t in _tokens(a)), a.describe()
    assert [a.launch_kernel(i) for i in range(a.num_launches)] == [b.launch_kernel(i) for i in range(b.num_launches)]


# ---- plans of the case table
@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return rect_cases.plan(name, case, rect_cases.make_input(name, case))


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, ids = _planned(name)
    assert rect_cases.r_lines(g.net, case) == rect_cases.expect(case), g.net.describe()
    assert len(rect_cases.r_lines(g.net, case)) == len(ids)          # one launch per rectangular conv, the residual join and an int32 form included
    if case['kind'] == 'dw':                                         # the dwk_dot4 = 0 leg: the scalar kernel everywhere
        g0, _, _ = rect_cases.plan(name, case, rect_cases.make_input(name, case), dwk_dot4=0)
        assert rect_cases.r_lines(g0.net, case) == rect_cases.expect(case, dot4=False), g0.net.describe()
    if case['join_i32']:
        tok = rect_cases.expect(case)[0][0]
        line = [ln for ln in g.net.describe().splitlines() if tok in ln][0]
        assert 'out[i32=1 i8=1' in line, g.net.describe()
    if case['res']:
        assert not any(t.startswith('add:') for t in _tokens(g.net)), g.net.describe()      # the join rides in the conv's epilogue


@pytest.mark.parametrize('name', sorted(rect_cases.DW_GENERIC))
def test_stride_2_and_the_int32_form_plan_the_scalar_kernel_whatever_the_option_says(name):
    assert all(k.startswith('f8::dwconvk_kernel<') for _, k in rect_cases.expect(ALL[name], dot4=True))
    g, _, _ = _planned(name)
    assert all(k.startswith('f8::dwconvk_kernel<') for _, k in rect_cases.r_lines(g.net, ALL[name]))


@pytest.mark.parametrize('name', ['p_1x7_14x14_c40', 'p_3x5_s2x1', 'p_2x4_asymmetric', 'p_3x1_d2', 'd_1x21_5x35', 'd_7x1_pad3_1', 'dg_s2_1x7'])
def test_launch_info_and_valu_count_the_real_taps(name):
    case = ALL[name]
    g, _, _ = _planned(name)
    i = [k for k in range(g.net.num_launches) if g.net.launch_info(k, 1)[0].split(':')[0] + ':' == rect_cases.expect(case)[0][0]][0]
    (t, l, b, r), (sh, sw) = case['pads'], case['stride']
    P, Q = rect_cases.out_size(case['H'], case['kh'], sh, t, b, case['d']), rect_cases.out_size(case['W'], case['kw'], sw, l, r, case['d'])
    N, cin_g, taps = case['N'], case['C'] // rect_cases.groups_of(case), case['kh'] * case['kw']
    assert g.net.launch_info(i, N)[2] == 2.0 * taps * cin_g * case['cout'] * P * Q * N
    if case['kind'] == 'dw':                                         # one v_dot4 per four taps + three operations per requantised value
        assert g.net.launch_valu(i, N) == (taps * P * Q * case['C'] / 4.0 + 3.0 * P * Q * rect_cases._cs(case['C'])) * N


@pytest.mark.parametrize('tile', sorted(rect_cases.TILES))
def test_igemm_tile_forces_the_tile_of_a_rectangular_conv(tile):
    name = rect_cases.TILE_CASE
    g, _, _ = rect_cases.plan(name, ALL[name], rect_cases.make_input(name, ALL[name]), igemm_tile=tile)
    assert rect_cases.r_lines(g.net, ALL[name]) == rect_cases.expect(ALL[name], tile=rect_cases.TILES[tile]), g.net.describe()


def test_every_expected_kernel_is_an_exported_symbol():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for dot4 in (True, False) for _, k in rect_cases.expect(c, dot4)}
    names |= {k for t in rect_cases.TILES.values() for _, k in rect_cases.expect(ALL[rect_cases.TILE_CASE], tile=t)}
    assert {'f8::dwstrip_dot4_kernel<2>', 'f8::dwstrip_dot4_kernel<3>', 'f8::dwstrip_dot4_kernel<4>', 'f8::dwstrip_dot4_kernel<6>',
            'f8::dwconvk_kernel<true>', 'f8::dwconvk_kernel<false>'} <= names
    for k in sorted(names):
        arg = 'f8::DwArgs' if 'dw' in k else 'f8::ConvArgs'
        assert f'void {k}({arg})' in syms, k


def test_no_fused_or_chain_launch_takes_a_rectangular_conv_in():
    """1x1 -> 3x3 with pads (2, 1, 0, 1) -> 1x1, join: the shape of an identity bottleneck but for two pads; with every fusing pass on, the 3x3 stays a launch of
    its own on conv_igemm_kernel and no fused_ token appears."""
    C, MID = 512, 128
    net = F8Net()
    x = net.input(C, 28, 28, 4)
    kw = dict(groups=1, weight_fl=6, input_fl=4, input_signed=False)
    pre = net.conv(x, _w(1, (C, C, 1, 1), 30.0), None, stride=1, pad=0, relu=True, **kw)
    t = net.conv(pre, _w(2, (MID, C, 1, 1), 30.0), None, stride=1, pad=0, relu=True, **kw)
    t = net.conv(t, _w(3, (MID, MID, 3, 3), 30.0), None, stride=1, pad=(2, 1, 0, 1), relu=True, **kw)          # -> 28 x 28 too
    t = net.conv(t, _w(4, (C, MID, 1, 1), 30.0), None, stride=1, pad=0, relu=False, **kw)
    net.output(net.add(t, pre, relu=True), as_float=False)
    for k, v in rect_cases.FUSE_ALL.items():
        net.set_option(k, v)
    net.finalize(4)
    toks = _tokens(net)
    assert not any(t.startswith('fused_') or 'chain' in t.split(':')[0] or 'patch' in t.split(':')[0] for t in toks), net.describe()
    i = [k for k, t in enumerate(toks) if t.startswith('conv3x3s1_t')]
    assert len(i) == 1 and net.launch_kernel(i[0]).startswith('f8::conv_igemm_kernel<'), net.describe()


def test_bias_classes_of_the_asymmetric_2x4_case():
    """9 x 11 map, kernel 2 x 4, pads (top 0, left 1, bottom 1, right 2), stride 1, unsigned -> 9 x 11.  Output row p reads rows p, p + 1: masks 11 for
    p = 0 .. 7 and 01 for p = 8 — two row classes.  Output column q reads columns q - 1 .. q + 2: q = 0: 1110 (bit s = tap s: 0b1110), q = 1 .. 8: 1111,
    q = 9: 0111, q = 10: 0011 — four column classes; eight bias vectors.  The table is not visible through the ABI; its effect is: the reference's
    count of in-image taps, per pixel, with an input of ones — and the weight image grows by the seven further bias vectors (72 -> 96 int32 each) and
    the two class tables, against the one vector of a signed input."""
    rows = [2] * 8 + [1]
    cols = [3] + [4] * 8 + [3, 2]
    want = rect_cases.rect_conv_ref(np.ones((1, 40, 9, 11), np.int32), np.ones((72, 40, 2, 4), np.int32), None, 1, (0, 1, 1, 2), 1)
    assert (want[0, 0] == 40 * np.outer(rows, cols)).all()
    rmasks = sorted({sum(1 << r for r in range(2) if 0 <= p + r < 9) for p in range(9)})
    cmasks = sorted({sum(1 << s for s in range(4) if 0 <= q - 1 + s < 11) for q in range(11)})
    assert rmasks == [0b01, 0b11] and cmasks == [0b0011, 0b0111, 0b1110, 0b1111]

    def build(signed):
        net = F8Net()
        t = net.input(40, 9, 11, 7 if signed else 8)
        t = net.conv(t, np.ones((72, 40, 2, 4), np.int32), None, stride=1, pad=(0, 1, 1, 2), groups=1, weight_fl=0, input_fl=7 if signed else 8,
                     input_signed=signed, quant_input=False, relu=False)
        net.output(t, as_float=False)
        return net.finalize(1)
    grown = build(False).weight_bytes - build(True).weight_bytes
    extra = (len(rmasks) * len(cmasks) - 1) * 96 * 4 + 9 + 11
    assert extra <= grown <= extra + 3 * 256, grown                # (each table starts on a 256-byte boundary)


# ---- liveness on the reference
@pytest.mark.parametrize('name', rect_cases.LIVENESS + sorted(rect_cases.MAX_BATCH) + sorted(rect_cases.PIPELINED))
def test_every_case_is_live_on_the_reference(name):
    case = ALL[name]
    g, out, ids = rect_cases.reference(name)
    gc, outc, _ = rect_cases.reference(name, centre=True)
    y = g.v[out][0]
    assert np.unique(y).size > 16, name
    assert (y != gc.v[outc][0]).mean() > 0.25, name                 # the outer taps matter: not the same as the central tap alone
    for t in ids:                                                    # the conv's own result: neither all zero behind its ReLU nor constant
        v = g.v[t][0]
        assert (v != 0).mean() > 0.25 and np.unique(v).size > 16, name
    for label, xq, signed in g.taps:                                 # what the readers (and a second conv) read: 8 bits in use, not pinned at the clamps
        lo, hi = (-127, 127) if signed else (0, 255)
        assert ((xq == lo) | (xq == hi)).mean() < 0.6 and np.unique(xq).size > 16, (name, label)
    if case['bias_big']:
        assert (np.abs(g.raw[ids[0]].astype(np.int64)) > 2 ** 30).any(), name


# ---- ONNX
def _inception_like(g, t):
    """1x1 -> 1x7 -> 7x1 -> 3x1 at dilation 2 -> SAME-padded 3x3 / 2 -> depthwise 1x11, on 32 channels."""
    kw = dict(groups=1, weight_fl=5, input_signed=False, relu=True)
    t = g.conv(t, _w(1, (32, 32, 1, 1), 150.0 / 32 ** 0.5), _b(2, 32, 2.0 ** 9, 2.0 ** 12), pad=0, input_fl=8, quant_input=False, **kw)
    t = g.conv_rect(t, _w(3, (32, 32, 1, 7), 10.0), _b(4, 32, 2.0 ** 9, 2.0 ** 12), pads=(0, 3, 0, 3), input_fl=4, **kw)
    t = g.conv_rect(t, _w(5, (32, 32, 7, 1), 10.0), _b(6, 32, 2.0 ** 9, 2.0 ** 12), pads=(3, 0, 3, 0), input_fl=4, **kw)
    t = g.conv_rect(t, _w(7, (32, 32, 3, 1), 15.0), _b(8, 32, 2.0 ** 9, 2.0 ** 12), pads=(2, 0, 2, 0), dilation=2, input_fl=4, **kw)
    t = g.conv_rect(t, _w(9, (32, 32, 3, 3), 9.0), _b(10, 32, 2.0 ** 9, 2.0 ** 12), stride=2, pads=(0, 0, 1, 1), input_fl=4, **kw)
    return g.conv_rect(t, _w(11, (32, 1, 1, 11), 45.0), _b(12, 32, 2.0 ** 9, 2.0 ** 12), pads=(0, 5, 0, 5), input_fl=4, **dict(kw, groups=32))


def test_the_onnx_round_trip_preserves_the_geometry():
    x = synth.rand_uniform_int(5, 'rect_onnx_x', (2, 32, 10, 12), 0, 255).astype(np.int32)
    ig, g, out = rect_cases.record_int_graph(x, 8, _inception_like)
    want = g.v[out][0]
    assert np.unique(want).size > 16
    model = onnx_export.export_graph(ig)
    convs = [n for n in onnx_io.load_graph(model).nodes if n.op == 'Conv']
    assert [(tuple(n.attrs['kernel_shape']), tuple(n.attrs['strides']), tuple(n.attrs['pads']), tuple(n.attrs['dilations'])) for n in convs] == [
        ((1, 1), (1, 1), (0, 0, 0, 0), (1, 1)), ((1, 7), (1, 1), (0, 3, 0, 3), (1, 1)), ((7, 1), (1, 1), (3, 0, 3, 0), (1, 1)),
        ((3, 1), (1, 1), (2, 0, 2, 0), (2, 1)), ((3, 3), (2, 2), (0, 0, 1, 1), (1, 1)), ((1, 11), (1, 1), (0, 5, 0, 5), (1, 1))]
    back = onnx_import.import_graph(model)
    a = [o for o in ig.ops if o.kind == 'conv']
    b = [o for o in back.ops if o.kind == 'conv']
    assert [(o.rect, o.kernel, o.stride, o.pad, o.dilation, o.groups) for o in a] == [(o.rect, o.kernel, o.stride, o.pad, o.dilation, o.groups) for o in b]
    assert a[0].rect is None and a[1].rect == (1, 7, 1, 1, 0, 3, 0, 3) and a[4].rect == (3, 3, 2, 2, 0, 0, 1, 1)
    np.testing.assert_array_equal(graph_forward_rect(back, x), want)
    np.testing.assert_array_equal(graph_forward_rect(ig, x), want)
    da = ig.build_net(2).describe()
    assert da == back.build_net(2).describe() and all(t in da for t in ('conv1x7s1_t', 'conv7x1s1_t', 'conv3x1s1d2_t', 'conv3x3s2_t', 'dwconv1x11s1:')), da


def graph_forward_rect(ig, x):
    """refgraph.graph_forward evaluates square convs only and stays as it is: a chain of convs, rectangular or not, is walked here in its manner with the
    reference of rect_cases."""
    V, layer = ig.solve_fraclens(None)
    t = {}
    for i, o in enumerate(ig.ops):
        if o.kind == 'input':
            t[i] = np.ascontiguousarray(x, dtype=np.int32)
            continue
        assert o.kind == 'conv', o.kind
        s = t[o.src]
        if o.shift is not None:
            s = oracle.requant(s, layer[i][0], V[o.src], o.signed)
        g = o.conv_geometry()
        y = rect_cases.rect_conv_ref(s, o.weight, o.bias, g[2:4], g[4:], o.groups, o.dilation)
        t[i] = oracle.relu(y) if o.relu else y
    return t[ig.output]


@pytest.mark.parametrize('edit, words', [
    (lambda n: n.attrs.__setitem__('dilations', [2, 3]), ('equal dilations',)),
    (lambda n: n.attrs.__setitem__('auto_pad', b'SAME_UPPER'), ('auto_pad', 'SAME_UPPER')),
    (lambda n: n.attrs.__setitem__('pads', [0, 9, 0, 3]), ('pad exceeds', '6 columns')),
    (lambda n: n.attrs.__setitem__('group', 4), ('grouped rectangular',)),
])
def test_what_the_library_refuses_is_an_import_error_that_says_which(edit, words):
    x = synth.rand_uniform_int(5, 'rect_onnx_x', (2, 32, 10, 12), 0, 255).astype(np.int32)
    ig, _, _ = rect_cases.record_int_graph(x, 8, _inception_like)
    model = onnx_io.load_graph(onnx_export.export_graph(ig))
    n = [n for n in model.nodes if n.op == 'Conv'][1]                # the 1x7
    if words[0] == 'equal dilations':
        n = [n for n in model.nodes if n.op == 'Conv'][4]            # unequal dilations on the 3x3
    edit(n)
    if words[0] == 'grouped rectangular':                            # 32 -> 32 in 4 groups: the weight is [32, 8, 1, 7]
        model.initializers[n.inputs[1]] = np.ascontiguousarray(model.initializers[n.inputs[1]][:, :8])
    with pytest.raises(onnx_import.OnnxImportError) as e:
        onnx_import.import_graph(model)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
