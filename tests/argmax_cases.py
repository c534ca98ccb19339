"""Case table, reference and graph builder of the tests of channel argmax outputs (f8_net_output_argmax / `F8Net.output_argmax`, f8_argmax.hip):
tests/test_argmax_plan.py (tokens, kernel symbols, the fusion conditions, refusals, queries, arena; no GPU) and tests/test_gpu_argmax.py (every case,
every data kind, on three legs, bit for bit on the device).  No test functions here.

The reference.  `ArgmaxGraph` is RefGraph with `output_argmax`: `np.argmax(value.astype(np.int64), axis=1)` on the value RefGraph already holds for
the marked tensor — so a fused case's reference is ref_ops.upsample_ref (the int32 wrap included) followed by argmax; numpy returns the FIRST maximal
index.  `pin_to_torch` holds it against torch.argmax(dim=1) on the same int64 data, ties included (tests/test_argmax_plan.py runs it).

A case marks the NETWORK INPUT (any int32 values: the input launch writes its int32 form as it is) or the input upsampled, so the data of the marked
tensor is the test's to choose, value for value.  `linear1000` marks an f8_net_linear's result: its input is one-hot per image (x[n, i] = 1 where
i == n), so logits[n, c] = W[c, n] + b[c], and the data lives in the weights.

Data kinds (`data_kinds(name)`); `_logits` builds each so that its property holds and `reference` ASSERTS it on the reference (`_check_data`):
  neg       every real logit of every pixel < 0 (pad channels hold 0: they must not compete)
  equal     every channel equal everywhere: the class map is all 0
  ties      exact ties of the maximum at channels c and c + d, d in 4 (the two lane halves), 8 (two groups), 32 (two channel blocks) — d = 1 where C < 5;
            the reference gives the lower index at every pixel.  Unfused cases tie per pixel, with c and d moving over the pixels; fused cases tie whole
            channel maps per image (equal maps interpolate to equal maps)
  extremes  INT32_MIN in every channel of the even pixels (class 0), INT32_MAX ties on the odd ones (the marked tensor of an unfused case, the
            source of a fused one)
  wrap      bilinear fused cases only (nearest has no arithmetic): source values around 2^31 / (4 s^2), so interpolated sums pass 2^31 and wrap; at
            least one output value wrapped and the wrapped value decides at least one pixel (argmax of the exact sums differs there)
  random    the reference map holds at least min(C, 10) distinct classes — or as many as the data has pixels, where those are fewer (`linear1000`: 6
            images; the broadcast: 3 source pixels)
`linear1000` has neg, equal, ties and random (its logits are W + b with W in int8: no extremes).

The expected plan tokens and kernel symbols are WRITTEN BY HAND (the rule: DESIGN.md 4.5p); nothing here asks the planner for them."""
import functools

import numpy as np

from dil_cases import FUSE_ALL as _FUSE_ALL
from f8net_amd import synth
from graph_cases import launch_lines
from ref_ops import bilinear_exact
from refgraph import RefGraph

X_FL = 8
FUSE_ALL = dict(_FUSE_ALL, fuse_argmax=1)                          # every fusing pass on, the one this module is about included
LEGS = {'default': {}, 'fuse_all': FUSE_ALL, 'unfused': {'fuse_argmax': 0}}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

SYMBOL = {'argmax_u8:': 'f8::argmax_i32t_kernel<1>', 'argmax_i32:': 'f8::argmax_i32t_kernel<4>',
          'upsample_nearest+argmax_u8:': 'f8::upsample_argmax_kernel<false, 1>', 'upsample_nearest+argmax_i32:': 'f8::upsample_argmax_kernel<false, 4>',
          'upsample_bilinear+argmax_u8:': 'f8::upsample_argmax_kernel<true, 1>', 'upsample_bilinear+argmax_i32:': 'f8::upsample_argmax_kernel<true, 4>'}


def argmax_ref(value):
    """[N, C, H, W] int32 -> [N, H, W]: the smallest index of the largest value."""
    return np.argmax(np.asarray(value).astype(np.int64), axis=1)


def pin_to_torch(value):
    """argmax_ref against torch.argmax(dim=1) on the same int64 data."""
    import torch
    np.testing.assert_array_equal(argmax_ref(value), torch.argmax(torch.from_numpy(np.asarray(value).astype(np.int64)), dim=1).numpy())


class ArgmaxGraph(RefGraph):
    """RefGraph with argmax outputs.  `outs`: every output in the order of the calls — ('value', reference) or ('argmax', reference map, dtype)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.outs = []

    def output(self, t, as_float=False):
        super().output(t, as_float=as_float)
        self.outs.append(('value', self.v[t][0]))

    def output_argmax(self, t, dtype='u8'):
        if self.record:
            assert self.net.output_argmax(t, dtype) == len(self.outs)
        self.outs.append(('argmax', argmax_ref(self.v[t][0]), dtype))


# ---- the builders: build(g, x0, c, data) marks the outputs; returns the marked tensor's id
def _mark(g, t, c):
    g.output_argmax(t, c['dtype'])
    return t


def _plain(g, x0, c, data):
    return _mark(g, x0, c)


def _fused(g, x0, c, data):
    return _mark(g, g.upsample(x0, c['scale'], c['mode'], label='up'), c)


def _behind_value(g, x0, c, data):
    """Output 0 is a value output (the input max-pooled 2 x 2); the class map of the input is output 1."""
    g.output(g.maxpool(x0, 2, 2, 0))
    return _mark(g, x0, c)


def _both(g, x0, c, data):
    """Both marks on one tensor: its values as output 0, its class map as output 1."""
    g.output(x0)
    return _mark(g, x0, c)


def _up_second_reader(g, x0, c, data):
    """The upsampled tensor has a second reader (a 2 x 2 max-pool that is output 0): two launches whatever fuse_argmax says."""
    up = g.upsample(x0, c['scale'], c['mode'], label='up')
    g.output(g.maxpool(up, 2, 2, 0))
    return _mark(g, up, c)


def _up_value_output(g, x0, c, data):
    """The upsampled tensor is a value output as well: two launches whatever fuse_argmax says."""
    up = g.upsample(x0, c['scale'], c['mode'], label='up')
    g.output(up)
    return _mark(g, up, c)


def _linear(g, x0, c, data):
    """One-hot input -> linear: logits[n, j] = W[j, n] + b[j] (module docstring).  The data kind lives in W and b."""
    w, b = _linear_params(c, data)
    return _mark(g, g.linear(x0, w, b, weight_fl=0, input_fl=X_FL, input_signed=False, label='fc'), c)


def _case(C, H, W, N, dtype='u8', build=_plain, mode=None, scale=None, tok=None, tok_off=None, **kw):
    """C x H x W: the INPUT (the marked tensor, or the upsample's source).  tok / tok_off: the argmax launch's token with fuse_argmax = 1 / 0."""
    base = 'argmax_u8:' if dtype == 'u8' else 'argmax_i32:'
    fused = f'upsample_{mode}+{base}' if build is _fused else base
    c = dict(C=C, H=H, W=W, N=N, dtype=dtype, build=build, mode=mode, scale=scale, tok=tok or fused, tok_off=tok_off or base, opts={}, classes=C)
    c.update(kw)
    return c


CASES = {
    # ---- unfused
    'c2_1x1': _case(2, 1, 1, 1),
    'c3_5x3': _case(3, 5, 3, 2),
    'c21_7x7': _case(21, 7, 7, 3),                                 # 49-pixel maps straddle 32-pixel blocks and images
    'c32_4x8': _case(32, 4, 8, 2),
    'c33_6x6': _case(33, 6, 6, 2),                                 # a second channel block with one real channel
    'c150_3x3': _case(150, 3, 3, 2),
    'c255_2x2_u8': _case(255, 2, 2, 2),
    'c256_2x2_i32': _case(256, 2, 2, 2, 'i32'),
    'c21_7x7_i32': _case(21, 7, 7, 3, 'i32'),
    'linear1000': _case(8, 1, 1, 5, 'i32', build=_linear, classes=1000),
    'behind_value': _case(21, 5, 3, 2, build=_behind_value),
    'both_marks': _case(21, 5, 3, 2, build=_both),
    'split2': _case(21, 3, 3, 4, opts={'split': 2}),               # 9 pixels an image: the second sub-batch starts at byte 18 of the caller's buffer
    'split2_i32': _case(21, 3, 3, 4, 'i32', opts={'split': 2}),
    # ---- an upsample that something else reads: two launches on every leg
    'up_second_reader': _case(21, 3, 3, 2, build=_up_second_reader, mode='bilinear', scale=2),
    'up_value_output': _case(21, 3, 3, 2, build=_up_value_output, mode='nearest', scale=(2, 2)),
}
for _dt in ('u8', 'i32'):
    CASES.update({
        f'b2_21x5x3_{_dt}': _case(21, 5, 3, 2, _dt, _fused, 'bilinear', 2),
        f'b4_19x3x3_{_dt}': _case(19, 3, 3, 2, _dt, _fused, 'bilinear', 4),
        f'b8_33x2x3_{_dt}': _case(33, 2, 3, 2, _dt, _fused, 'bilinear', 8),
        f'b16_21x2x2_{_dt}': _case(21, 2, 2, 2, _dt, _fused, 'bilinear', 16),
        f'n23_21x3x2_{_dt}': _case(21, 3, 2, 2, _dt, _fused, 'nearest', (2, 3)),
        f'nbcast_21x1x1_{_dt}': _case(21, 1, 1, 2, _dt, _fused, 'nearest', (4, 5)),      # the broadcast
    })
FUSED = [n for n, c in CASES.items() if c['build'] is _fused]


def is_upsampled(c):
    return c['mode'] is not None


def data_kinds(name):
    c = CASES[name]
    if c['build'] is _linear:
        return ('neg', 'equal', 'ties', 'random')
    return ('neg', 'equal', 'ties', 'extremes', 'random') + (('wrap',) if c['mode'] == 'bilinear' else ())


def _rand(tag, shape, lo, hi):
    return synth.rand_uniform_int(23, tag, shape, lo, hi).astype(np.int64)


def _tie_steps(C):
    return [d for d in (4, 8, 32) if d < C] or [1]


def _logits(name, data, n):
    """[n, C, H, W] int64 values (inside int32) of the tensor the data kind is written into: the input, or `linear1000`'s logits."""
    c = CASES[name]
    C, H, W = c['classes'], c['H'], c['W']
    shape = (n, C, H, W)
    tag = f'amax{name}{data}'
    if data == 'neg':
        return _rand(tag, shape, -100 if c['build'] is _linear else -2 ** 20, -1)
    if data == 'equal':
        return np.full(shape, 7, np.int64)
    if data == 'random':
        lim = 100 if c['build'] is _linear else 2 ** 30
        for attempt in range(64):                                  # (a two-pixel map: the first draw may give both pixels one class)
            x = _rand(f'{tag}{attempt}', shape, -lim, lim)
            if np.unique(np.argmax(x, axis=1)).size >= min(C, 10, n * H * W):
                return x
        raise AssertionError(f'{name}: no random draw with enough classes')
    if data == 'wrap':
        s = c['scale']
        mid = 2 ** 31 // (4 * s * s)
        return _rand(tag, shape, mid - mid // 8, mid + mid // 8)
    steps = _tie_steps(C)
    x = _rand(tag, shape, -90, 90)
    top = 120 if c['build'] is _linear else 5000
    if data == 'ties':
        if is_upsampled(c) or c['build'] is _linear:               # whole channel maps per image
            for i in range(n):
                d = steps[i % len(steps)]
                ch = (5 * i + 3) % (C - d)
                x[i, ch] = top + (0 if c['build'] is _linear else _rand(tag + 'm', (H, W), 0, 50))
                x[i, ch + d] = x[i, ch]
        else:                                                      # per pixel, c and d moving over the pixels
            for m in range(n * H * W):
                i, h, w = m // (H * W), m // W % H, m % W
                d = steps[m % len(steps)]
                ch = (7 * m + 1) % (C - d)
                x[i, ch, h, w] = x[i, ch + d, h, w] = top
        return x
    assert data == 'extremes'
    x = _rand(tag, shape, -2 ** 30, 2 ** 30)
    for m in range(n * H * W):
        i, h, w = m // (H * W), m // W % H, m % W
        if m % 2 == 0:
            x[i, :, h, w] = I32_MIN
        else:
            d = steps[m % len(steps)]
            ch = (3 * m + 2) % (C - d)
            x[i, ch, h, w] = x[i, ch + d, h, w] = I32_MAX
    return x


def _linear_params(c, data):
    """W [1000, 8] int8-range and b [1000] with logits[n] = W[:, n] + b the data kind's values for image n (b carries nothing: 0)."""
    lg = _logits('linear1000', data, c['C'])[:, :, 0, 0]          # [8 images, 1000]
    return np.ascontiguousarray(lg.T).astype(np.int32), np.zeros(c['classes'], np.int32)


def make_input(name, data, n):
    c = CASES[name]
    if c['build'] is _linear:
        x = np.zeros((n, c['C'], 1, 1), np.int32)
        x[np.arange(n), np.arange(n)] = 1
        return x
    return _logits(name, data, n).astype(np.int32)


def build_graph(name, data, x, record=True):
    c = CASES[name]
    g = ArgmaxGraph(x, X_FL, record=record)
    t = c['build'](g, next(iter(g.v)), c, data)
    return g, t


def _check_data(name, data, g, t, x):
    """What the module docstring promises about the data, on the reference."""
    c = CASES[name]
    v = g.v[t][0].astype(np.int64)                                 # the marked tensor
    ref = argmax_ref(v)
    C = v.shape[1]
    top = v.max(axis=1)
    if data == 'neg':
        assert v.max() < 0
    elif data == 'equal':
        assert (v == v[:, :1]).all() and (ref == 0).all()
    elif data == 'ties':
        nmax = (v == top[:, None]).sum(axis=1)
        assert (nmax == 2).all(), 'every pixel has one exact tie of its maximum'
        second = C - 1 - np.argmax(v[:, ::-1].astype(np.int64), axis=1)      # the LAST maximal index
        assert (second > ref).all() and set(np.unique(second - ref)) == set(_tie_steps(C)), 'the tie steps of the structure, the reference on the lower index'
    elif data == 'extremes':
        s = x.astype(np.int64)                                     # the input: the marked tensor itself, or the upsample's source
        allmin = (s == I32_MIN).all(axis=1)
        maxtie = ((s == I32_MAX).sum(axis=1) == 2)
        assert allmin.any() and maxtie.any() and (allmin | maxtie).all()
        if not is_upsampled(c):
            assert (ref[allmin] == 0).all()
    elif data == 'wrap':
        exact = bilinear_exact(x, int(np.log2(c['scale'])))
        assert (np.abs(exact) >= 2 ** 31).any(), 'no interpolated sum leaves int32: the case shows nothing'
        assert (np.argmax(exact, axis=1) != ref).any(), 'the wrapped value decides no pixel'
    elif data == 'random':
        assert np.unique(ref).size >= min(C, 10, x.shape[0] * c['H'] * c['W']), np.unique(ref).size
    if c['dtype'] == 'u8':
        assert ref.max() < 255


@functools.lru_cache(maxsize=None)
def reference(name, data):
    """The case on the reference alone over N + 1 images, its data checked; once; read-only.  Returns (graph, marked tensor id, input)."""
    x = make_input(name, data, CASES[name]['N'] + 1)
    g, t = build_graph(name, data, x, record=False)
    _check_data(name, data, g, t, x)
    return g, t, x


def plan(name, data, x, max_batch=None, **opts):
    g, t = build_graph(name, data, x)
    for k, v in dict(CASES[name]['opts'], **opts).items():
        g.net.set_option(k, v)
    g.net.finalize(max_batch or x.shape[0])
    return g, t


def argmax_lines(net):
    """[(launch index, plan token, kernel symbol)] of the handle's argmax launches, fused or not, in launch order."""
    return [l for l in launch_lines(net) if 'argmax' in l[1]]


def upsample_lines(net):
    """... of its upsample launches (a fused argmax launch is none)."""
    return [l for l in launch_lines(net, 'upsample_') if 'argmax' not in l[1]]


def expected_token(name, opts):
    c = CASES[name]
    return c['tok'] if dict(c['opts'], **opts).get('fuse_argmax', 1) else c['tok_off']


# ---- a segmentation tail as an IntGraph (the ONNX tests): input (8 channels, 0 .. 255) -> 1x1 classifier to 21 classes -> bilinear x4 -> class map
def seg_tail_int_graph(dtype='u8', n=2):
    """Returns (IntGraph with output_argmax = dtype, input, reference class map)."""
    from refgraph import record_int_graph
    x = synth.rand_uniform_int(5, 'amaxseg', (n, 8, 5, 3), 0, 20).astype(np.int32)
    for m in range(n * 15):                                        # one loud channel per pixel, moving over the pixels: the winning class moves with it
        x[m // 15, m % 8, m // 3 % 5, m % 3] = 255
    w = synth.rand_uniform_int(7, 'amaxsegw', (21, 8, 1, 1), -127, 127).astype(np.int32)

    def build(g, x0):
        cls = g.conv(x0, w, None, pad=0, groups=1, weight_fl=5, input_fl=X_FL, input_signed=False, relu=False, quant_input=False)
        return g.upsample(cls, 4, 'bilinear')
    ig, g, out = record_int_graph(x, X_FL, build)
    ig.output_argmax = dtype
    want = argmax_ref(g.v[out][0])
    assert np.unique(want).size >= 5
    return ig, x, want
