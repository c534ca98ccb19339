"""The standalone depthwise 3x3 launches (dwconv3x3_mma_kernel of f8_dwmma.hip, dwconv3x3_dot4_kernel and dwconv3x3_kernel of f8_kernels.hip) at op
level, without a GPU: the plan of every case of tests/dw_cases.py against the hand-written table on all three legs, the kernel instances as exported
symbols, and the liveness of every case on the oracle's values — the aimed-at strips, bands and borders included."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dw_cases
from f8net_amd import _lib

ALL = dict(dw_cases.CASES, band14=dw_cases.BAND14_CASE, max_batch=dw_cases.MAX_BATCH_CASE, pipelined=dw_cases.PIPELINED_CASE)


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return dw_cases.plan(name, case, dw_cases.make_input(name, case))


def _is_mma(case):
    return dw_cases.leg_kernels(case, 'own')[0].startswith('f8::dwconv3x3_mma_kernel')


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, ids = _planned(name)
    assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case), g.net.describe()
    lines = [ln for ln in g.net.describe().splitlines() if 'dwconv3x3s' in ln]
    assert len(lines) == len(ids), g.net.describe()                 # one launch per depthwise conv, an int32 form next to int8 ones included
    if case['join_i32']:                                           # the planner keeps the int32 form and the int8 form on the one launch
        assert 'out[i32=1 i8=1' in lines[0], g.net.describe()
    if name == 'band14':                                          # (the other legs of this one: test_gpu_dw.py plans them anyway)
        return
    x = dw_cases.make_input(name, case)
    for leg in ('dot4', 'generic'):
        other, _, _ = dw_cases.plan(name, case, x, leg)
        assert [ln[1:] for ln in dw_cases.dw_lines(other.net)] == dw_cases.expect(case, leg), (leg, other.net.describe())
        assert other.net.num_launches == g.net.num_launches


def test_every_expected_kernel_is_an_exported_symbol_and_the_table_covers_the_instances():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for leg in dw_cases.LEGS for k in dw_cases.leg_kernels(c, leg)}
    for k in sorted(names):
        assert f'void {k}(f8::DwArgs)' in syms, k
    own = {k for c in ALL.values() for k in dw_cases.leg_kernels(c, 'own')}
    for s in (1, 2):
        for fq in (0, 1, 2):
            for subs in (1, 2):
                assert dw_cases.mma(s, fq, subs) in own, (s, fq, subs)
        assert dw_cases.dot4(s) in own, s
    for sgn in (False, True):
        assert dw_cases.generic(sgn) in own, sgn


def test_the_band_14_case_is_one_launch_of_4096_items():
    """launch_dwconv_mma keeps DW_BAND = 14 only from 4096 wave items on: N x bands x strips x channel tiles of ONE launch.  The case has exactly
    that many with a ragged band (14 + 1 rows) and a ragged strip (28 + 1 columns); half of the batch (the default split) would run band 8."""
    case = dw_cases.BAND14_CASE
    g, _, _ = _planned('band14')
    (i, tok, kern), = dw_cases.dw_lines(g.net)
    assert g.net.step_launches(i, case['N']) == 1
    assert g.net.num_parts(case['N']) == 1
    P, Q = dw_cases.out_hw(case)
    items = case['N'] * ((P + 13) // 14) * ((Q + 27) // 28) * (case['C'] // 32)
    assert items == 4096 and (P + 13) // 14 == 2 and P % 14 == 1 and (Q + 27) // 28 == 2 and Q % 28 == 1
    assert dw_cases.mma_tiling(case, case['N']) == (28, 14, 4096)
    assert dw_cases.mma_tiling(case, case['N'] // 2)[1] == 8


def test_the_small_cases_run_band_8_or_one_band():
    for name, case in ALL.items():
        if name == 'band14' or not _is_mma(case):
            continue
        P, _ = dw_cases.out_hw(case)
        vw, band, items = dw_cases.mma_tiling(case, case['N'])
        assert items < 4096 and band == (8 if P > 8 else 14), name


def _regions(case):
    """[(label, row slice, column slice)] of the depthwise output map a kernel of the case's own leg could leave unwritten or wrong: the border rows
    and columns; for the MMA kernel the last strip's columns and the last band's rows, for the v_dot4 kernel the last pixel pair."""
    P, Q = dw_cases.out_hw(case)
    one = lambda i: slice(i, i + 1)
    rs = [('row 0', one(0), slice(None)), ('last row', one(P - 1), slice(None)), ('column 0', slice(None), one(0)), ('last column', slice(None), one(Q - 1))]
    if _is_mma(case):
        vw, band, _ = dw_cases.mma_tiling(case, case['N'])
        rs += [('last strip', slice(None), slice((Q - 1) // vw * vw, Q)), ('last band', slice((P - 1) // band * band, P), slice(None))]
        if Q > vw:
            rs += [('strip seam', slice(None), slice(vw - 1, vw + 1))]
    elif dw_cases.leg_kernels(case, 'own')[0].startswith('f8::dwconv3x3_dot4'):
        rs += [('last pixel pair', slice(None), slice((Q - 1) // 2 * 2, Q))]
    return rs


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure: the final value has more than 8 distinct values; every int8 tensor a reader (or the second depthwise conv and
    the 1x1 in front of it) reads has at least 16 distinct values and fewer than half of its entries at a clamp bound; in every image, each border row
    and column, the last strip, the last band and the strip seam of what the depthwise conv hands on holds more than one value and is not all 0, so a
    kernel that left it unwritten, zero or constant cannot pass; a case that aims at a wrap shows it."""
    case = ALL[name]
    g, out, ids = _planned(name)
    assert np.unique(g.v[out][0]).size > 8
    assert len(g.taps) == len(case['readers'] or []) + (2 if case.get('second') else 0)
    for label, xq, sgn in g.taps:
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        assert ((xq == lo) | (xq == hi)).mean() < 0.5, label
    # what the first depthwise launch writes: its int8 forms (the readers' inputs; the 1x1's in the pipelined case), or its int32 result
    first = [xq for label, xq, _ in g.taps if label.startswith('mid' if case.get('second') else 'reader')] or [g.v[ids[0]][0]]
    for y in first:
        assert y.shape[2:] == dw_cases.out_hw(case)
        for label, rows, cols in _regions(case):
            for n in range(y.shape[0]):
                r = y[n, :, rows, cols]
                assert np.unique(r).size > 1 and (r != 0).any(), (label, n)
    if case['aim'] == 'bias_big':
        (fl, _), = case['readers']
        n = case['in_fl'] + case['w_fl'] - fl
        r = g.raw[ids[0]].astype(np.int64)
        assert (r > 2 ** 31 - 2 ** 13).any(), 'no accumulator next to 2^31'
        # the accumulator itself wrapped past 2^31, or the rounding add `v + 2^(n-1)` of the requantisation does: the reference then clamps to 0
        wraps = (r < -2 ** 30) | (r + (1 << (n - 1)) > 2 ** 31 - 1)
        assert wraps[:, [3, 17]].any(), 'nothing wraps'
        assert (g.taps[0][1][wraps] == 0).all()
    else:
        assert case['aim'] is None


def test_the_relu_floor_matters_where_a_signed_reader_follows_it():
    """Behind a ReLU an unsigned reader's clamp at 0 does what the floor does; a signed reader's does not.  Those cases have accumulators below 0
    that a signed reader would keep, so a missing floor shows."""
    seen = 0
    for name, case in ALL.items():
        if not (case['relu'] and any(sgn for _, sgn in case['readers'] or [])):
            continue
        g, _, ids = _planned(name)
        fl = min(fl for fl, sgn in case['readers'] if sgn)
        assert (g.raw[ids[0]] < -(1 << (case['in_fl'] + case['w_fl'] - fl))).mean() > 0.01, name
        seen += 1
    assert seen >= 4
