"""The fused head launches (f8_stem.hip) at op level, without a GPU: the plan of every case of tests/stem_cases.py against the hand-written
expectation (token, kernel name, the wording of the input step), table A against the twelve instances, the boundaries of stem_pool_supported /
head2_supported one step either side, and the liveness of every case on the oracle's values (tests/test_gpu_stem.py runs the cases on the device)."""
import functools

import numpy as np
import pytest

import stem_cases as sc
from f8net_amd.net import F8Net

ALL = sc.CASES


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    data = sc.make_data(name, case)
    return (data,) + sc.plan(name, case, data['x'])


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    _, g, _, _ = _planned(name)
    plan = g.net.describe()
    assert sc.head_lines(g.net) == ([sc.expect(case)] if case['kernel'] else []), plan
    assert (sc.RAW_WORDING in plan) == case['raw_plan'], plan
    if not case['kernel']:                                       # the unfused convs are there instead
        assert ('conv7x7s2_' if case['form'] == 'resnet' else 'conv3x3s2_') in plan, plan


# Table A by hand: (token, kernel, the input step says the stem launch reads the raw input, KIND the entry's runs select)
_R, _H = 'stem7x7s2+maxpool3x3s2:', 'head3x3s2+dw3x3+1x1:'
_POOL, _ROWS = 'f8::stem_pool_kernel', 'f8::stem_rows_kernel'
TABLE_A_BY_HAND = {
    'a_tile_i32': (_R, _POOL, True, 0), 'a_tile_f32': (_R, _POOL, True, 1), 'a_tile_u8': (_R, _POOL, True, 2),
    'a_tile_halo': (_R, _POOL, False, -1), 'a_tile_nhwc': (_R, _POOL, True, -1), 'a_tile_cin1': (_R, _POOL, False, -1), 'a_tile_cin4': (_R, _POOL, False, -1),
    'a_rows_i32': (_R, _ROWS, True, 0), 'a_rows_f32': (_R, _ROWS, True, 1), 'a_rows_u8': (_R, _ROWS, True, 2),
    'a_rows_halo': (_R, _ROWS, False, -1), 'a_rows_nhwc': (_R, _ROWS, True, -1), 'a_rows_cin1': (_R, _ROWS, False, -1), 'a_rows_cin4': (_R, _ROWS, False, -1),
    'a_h2_i32': (_H, _ROWS, True, 0), 'a_h2_f32': (_H, _ROWS, True, 1), 'a_h2_u8': (_H, _ROWS, True, 2),
    'a_h2_halo': (_H, _ROWS, False, -1), 'a_h2_nhwc': (_H, _ROWS, True, -1), 'a_h2_cin1': (_H, _ROWS, False, -1), 'a_h2_cin4': (_H, _ROWS, False, -1),
}


def test_table_a_is_the_twelve_instances_by_hand():
    assert set(sc.TABLE_A) == set(TABLE_A_BY_HAND)
    seen = set()
    for name, (tok, kernel, raw, kind) in TABLE_A_BY_HAND.items():
        case = sc.TABLE_A[name]
        _, g, _, _ = _planned(name)
        assert sc.head_lines(g.net) == [(tok, kernel)] and (sc.RAW_WORDING in g.net.describe()) == raw and case['kind'] == kind, name
        assert case['N'] == 3 and case['max_batch'] == 3
        assert sc.pooled_hw(case) == {'tile': (7, 8), 'rows': (9, 30), 'h2': (16, 30)}[case['kernel']]
        seen.add((case['kernel'], kind))
    assert seen == sc.INSTANCES and len(seen) == 12
    # a uint8 NHWC run cannot be read by the launch: reads_raw_input sends it through the input step, so KIND -1 on a plan whose wording is raw
    assert sc.TABLE_A['a_rows_nhwc']['opts'].get('fuse_input', 1) == 1


def _fused(form, H, W, na=6, nb=6, cout=32, **opts):
    case = sc._resnet(H, W, 'rows', opts=opts, shift=6) if form == 'resnet' else sc._h2(H, W, na=na, nb=nb, cout=cout, opts=opts)
    g, _, _ = sc.plan('boundary', case, np.zeros((1, 3, H, W), np.int32), max_batch=1)
    ls = sc.head_lines(g.net)
    assert len(ls) <= 1
    return ls[0][1].split('::')[1] if ls else None


def test_support_boundaries_one_step_either_side():
    """stem_pool_supported and head2_supported (and pass 1h's shifts and channel counts) through the plans they decide."""
    # pooled width 1 | 2 and 56 | 57 (the row kernel: 2 <= Q <= 2 strips of 28)
    assert _fused('resnet', 8, 4) is None and _fused('resnet', 8, 8) == 'stem_rows_kernel'
    assert _fused('resnet', 8, 224) == 'stem_rows_kernel' and _fused('resnet', 8, 228) is None
    # sides 4k | 4k + 2: 20 x 24 against 22 x 24 and 20 x 26 (conv 11 / 13: no instance of either kernel)
    assert _fused('resnet', 20, 24) == 'stem_rows_kernel' and _fused('resnet', 22, 24) is None and _fused('resnet', 20, 26) is None
    # ... unless the pooled map is whole 7 x 8 tiles: 26 x 30 -> conv 13 x 15 -> pooled 7 x 8, the tile kernel; with stem_rows = 0 it is the only one
    assert _fused('resnet', 26, 30) == 'stem_pool_kernel' and _fused('resnet', 28, 32, stem_rows=0) == 'stem_pool_kernel'
    assert _fused('resnet', 28, 32) == 'stem_rows_kernel' and _fused('resnet', 20, 24, stem_rows=0) is None
    assert _fused('resnet', 28, 32, fuse_stem=0) is None
    # H2: width 224 | 228, sides 4k | 4k + 2, shifts 16 | 17, cout 32 | 40
    assert _fused('h2', 8, 224) == 'stem_rows_kernel' and _fused('h2', 8, 228) is None
    assert _fused('h2', 8, 8) == 'stem_rows_kernel' and _fused('h2', 10, 8) is None and _fused('h2', 8, 10) is None and _fused('h2', 4, 8) is None
    assert _fused('h2', 8, 8, na=16) == 'stem_rows_kernel' and _fused('h2', 8, 8, na=17) is None
    assert _fused('h2', 8, 8, nb=16) == 'stem_rows_kernel' and _fused('h2', 8, 8, nb=17) is None
    assert _fused('h2', 8, 8, cout=32) == 'stem_rows_kernel' and _fused('h2', 8, 8, cout=40) is None
    assert _fused('h2', 8, 8, fuse_head2=0) is None


def test_bias_next_to_int32_max_keeps_the_plan():
    """An accumulator the planner cannot bound (acc_ok = 0) moves nothing the plan shows — the kernel names carry no template arguments and
    describe() no requantisation form; quant_lane16 takes its integer branch on the launch argument.  What this pins on the CPU: the cases that aim
    at it do hold accumulators next to both ends of int32, and plan the fused launch under requant_float = 1.  The device test decides the rest: the
    converter form is exact only up to kAccLimit, so a launch that took it would differ from the oracle there."""
    for name in ('c_bias_big_rq1', 'c_bias_big_rq0', 'c_h2_bias_big_head', 'c_h2_bias_big_dw'):
        case = ALL[name]
        _, g, _, ids = _planned(name)
        assert sc.head_lines(g.net) == [sc.expect(case)]
        assert g.net.get_option('requant_float') == case['opts'].get('requant_float', 0)
        raw = g.raw[ids['conv' if case['form'] == 'resnet' else 'head' if case['bias_big'] == 'head' else 'dw']].astype(np.int64)
        assert (raw > 2 ** 31 - 2 ** 24).any() and (raw < -2 ** 31 + 2 ** 24).any(), name


# ---- liveness on the oracle's values

def _check_form(label, v, xq, n, sgn, floored):
    lo, hi = (-127, 127) if sgn else (0, 255)
    few = n >= 24                                                # hi * 2^n is no int32 from n = 24 on: a handful of quotients, no upper clamp
    assert np.unique(xq).size >= (2 if few else 16), (label, np.unique(xq).size)
    assert (xq == (0 if floored else lo)).any(), (label, 'lower end', int(xq.min()))
    if not few:
        assert (xq == hi).any(), (label, 'upper end', int(xq.max()))
    if n > 0:
        assert sc.tie_parities(v, n, lo, hi) == (True, True), (label, 'ties', n)


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure; no case is exempt.  Every int8 form the launch writes (the H2 form's two inner ones included) has 16 distinct
    values, reaches both ends of its clamp (behind a ReLU the lower end is the floor's 0; from shift 24 on no int32 reaches the upper one) and,
    under a right shift, holds exact ties above an even and above an odd quotient.  Every ReLU has accumulators on both sides.  ResNet form: the
    pool's border windows and the seams of the kernel's strips, bands and tiles (stem_cases.border_liveness / seam_liveness).  H2: the depthwise
    taps that cross a strip seam are non-zero and the conv column there varies.  fp32 entry: exact .5 ties of both parities and values beyond both
    clamps; uint8 entries: pixels 0 and 255 in every plane; int32 outputs: values above 2^24 (a float detour would show)."""
    case = ALL[name]
    data, g, outs, ids = _planned(name)
    for o in outs:
        assert np.unique(g.v[o][0]).size > 8
    x = data['x']
    lo, hi = (-127, 127) if case['x_signed'] else (0, 255)
    assert x.min() >= lo and x.max() <= hi
    if case['entry'] in ('u8', 'nhwc'):
        pix = data['raw']
        assert ((pix == 0).any(axis=(2, 3)) & (pix == 255).any(axis=(2, 3))).all()
    else:
        assert ((x == lo).any(axis=(2, 3)) & (x == hi).any(axis=(2, 3))).all()
    if case['entry'] == 'f32':
        s = data['raw'].astype(np.float64) * 2.0 ** case['x_fl']
        tie = (s - np.floor(s)) == 0.5
        inside = tie & (s > lo) & (s < hi)
        assert (inside & (np.floor(s) % 2 == 0)).any() and (inside & (np.floor(s) % 2 == 1)).any()
        assert (s > hi + 1).any() and (s < lo - 1).any() and (s == hi + 0.5).any() and (s == lo - 0.5).any()
    if case['form'] == 'resnet':
        conv, pool = ids['conv'], ids['pool']
        for label, v, xq, n, sgn in sc.reader_forms(case, g, pool):
            _check_form(label, v, xq, n, sgn, case['relu'])
        raw = g.raw[conv]
        if case['relu']:
            assert (raw < 0).mean() > 0.01 and (raw > 0).mean() > 0.25, ((raw < 0).mean(), (raw > 0).mean())
        else:
            assert (g.v[pool][0] < 0).mean() > 0.01, 'no pooled value below the floor a ReLU would set'
        v = g.v[conv][0].astype(np.int64)
        assert sc.border_liveness(v) == []
        if case['kernel']:
            assert sc.seam_liveness(case, v) == []
        if case['out32']:
            assert (g.v[pool][0] > 2 ** 24).any()
    else:
        forms = [('dw_in', g.v[ids['head']][0], case['na']), ('pw_in', g.v[ids['dw']][0], case['nb'])]
        taps = {tp[0]: tp[1] for tp in g.taps}
        for label, v, n in forms:
            _check_form(label, v.astype(np.int64), taps[label], n, False, True)
        for label, v, xq, n, sgn in sc.reader_forms(case, g, ids['pw']):
            _check_form(label, v, xq, n, sgn, False)
        for t in (ids['head'], ids['dw']):
            raw = g.raw[t]
            assert (raw < 0).mean() > 0.01 and (raw > 0).mean() > 0.25, ((raw < 0).mean(), (raw > 0).mean())
        wd = ids['wd']
        for q in sc.h2_seams(case) if case['kernel'] else []:
            assert (wd[:, 0, :, 0] != 0).any() and (wd[:, 0, :, 2] != 0).any()
            assert np.unique(taps['dw_in'][:, :, :, q - 1]).size > 8 and np.unique(taps['dw_in'][:, :, :, q]).size > 8, q
        pw = g.v[ids['pw']][0]
        assert pw.shape[1] == case['cout']


def test_tables_cover_what_they_name():
    """Table B: the issue's widths and heights of each kernel; table C: the four branches of quant_lane16 by their conditions."""
    rows = {sc.pooled_hw(c) for n, c in sc.TABLE_B.items() if c['kernel'] == 'rows' and c['entry'] == 'i32'}
    assert rows == {(1, 2), (2, 27), (3, 28), (7, 29), (8, 30), (9, 55), (15, 56), (25, 25)}
    assert {c['entry'] for n, c in sc.TABLE_B.items() if sc.pooled_hw(c) == (5, 6)} == {'halo', 'nhwc', 'cin1', 'cin4'}
    tile = {(c['H'], c['W'], c['opts'].get('stem_rows', 1)) for c in sc.TABLE_B.values() if c['kernel'] == 'tile'}
    assert tile == {(25, 29, 1), (26, 30, 1), (27, 31, 1), (28, 32, 0), (56, 64, 0), (28, 64, 0)}
    h2 = {sc.pooled_hw(c) for c in sc.TABLE_B.values() if c['kernel'] == 'h2'}
    assert h2 == {(4, 4), (8, 28), (14, 30), (16, 56), (30, 58), (4, 84), (16, 86), (4, 112)}
    branch = set()
    for c in sc.TABLE_C.values():
        if c['form'] != 'resnet' or c['kernel'] != 'rows':
            continue
        for rfl, sgn in c['readers']:
            n = c['x_fl'] + c['w_fl'] - rfl
            conv = c['opts'].get('requant_float', 0) == 1 and not c['bias_big']
            branch.add(1 if (conv and 0 < n <= 16 and not sgn) else 2 if (0 < n <= 30 and not sgn) else 3 if n > 0 else 4)
    assert branch == {1, 2, 3, 4}
    shifts = {(c['x_fl'] + c['w_fl'] - c['readers'][0][0], c['opts'].get('requant_float', 0)) for c in sc.TABLE_C.values() if c['form'] == 'resnet' and c['readers']}
    assert {(1, 0), (1, 1), (9, 0), (9, 1), (16, 0), (16, 1), (17, 1), (30, 1), (0, 0), (-2, 0)} <= shifts
    assert {(c['na'], c['nb'], c['opts'].get('requant_float', 0)) for c in sc.TABLE_C.values() if c['form'] == 'h2'} >= {
        (a, b, r) for a, b in ((1, 1), (16, 16), (1, 16), (7, 3)) for r in (0, 1)}
    assert {c['cout'] for c in sc.TABLE_C.values() if c['form'] == 'h2'} == {8, 16, 24, 32}


def test_schedule_cases_have_the_tiles_they_name():
    for name, (ntiles, rem) in {'s_rows_9x60x8': (27, 3), 's_rows_8x56x120': (16, 0), 's_rows_24x28x8': (24, 0)}.items():
        c = sc.SCHED_ROWS[name]
        P = c['H'] // 4
        assert c['N'] * -(-P // sc.RB) == ntiles and ntiles % 8 == rem
    c = sc.SCHED_H2
    assert c['N'] * -(-(c['H'] // 2) // sc.H2_RB) == 27
    # 256 compute units under stem_grid_div = 32: 8 workgroups; 27 tiles: it = 0 .. 3 on the first three
    assert sc.row_grid(256, 32, 27) == 8 and sc.row_grid(304, 32, 27) == 16 and sc.row_grid(256, 32, 5) == 5
