"""The operand-stationary conv launches (conv1x1_wstat_kernel, conv1x1_wreg_kernel, conv3x3s2_wreg_kernel, conv3x3_patch_kernel) at
op level, without a GPU: the plan of every case of tests/ostat_cases.py against the hand-written table, the kernel instances as exported symbols,
table A against the list of instances launch_conv1x1_wstat can dispatch, the schedules the cases name (for 256 compute units), the planner's
wstat threshold, option wstat_grid_div, and the liveness of every case on the oracle's values."""
import functools
import os
import subprocess

import numpy as np
import pytest

import igemm_cases as ic
import ostat_cases as oc
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

ALL = dict(oc.CASES, w_max_batch=oc.WSTAT_MAX_BATCH, w_pipelined=oc.WSTAT_PIPELINED)
F8_ERR_INVALID = -1


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return ic.plan(name, case, ic.make_input(name, case))


def _m(case, n=None):
    P, Q = ic.out_hw(case)
    return (n or case['N']) * P * Q


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, _, _ = _planned(name)
    assert ic.under_test(g.net) == [(case['token'], case['kernel'])], g.net.describe()


def _symbols():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    return subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout


def _exported(syms, kernel):
    return {ln.split('void ')[1].split('(f8::ConvArgs')[0] for ln in syms.splitlines() if f'void f8::{kernel}<' in ln}


def test_every_expected_kernel_is_an_exported_symbol():
    syms = _symbols()
    for k in sorted({c['kernel'] for c in ALL.values()} | oc.all_wstat_instances()):
        assert f'void {k}(f8::ConvArgs' in syms, k
    # ... and the library exports no instance of the four kernels the tables do not run
    assert _exported(syms, 'conv1x1_wstat_kernel') == oc.all_wstat_instances()
    for kernel, table in (('conv1x1_wreg_kernel', oc.WREG), ('conv3x3s2_wreg_kernel', oc.S2WREG), ('conv3x3_patch_kernel', oc.PATCH)):
        assert _exported(syms, kernel) == {c['kernel'] for c in table.values()}, kernel


def test_table_a_is_exactly_the_dispatchable_instances():
    """50 = five bases x five output forms x FAST, one case each, every one reachable from a graph."""
    want = oc.all_wstat_instances()
    assert len(want) == 50 and len(oc.WSTAT_A) == 50
    assert {c['kernel'] for c in oc.WSTAT_A.values()} == want
    for c in oc.WSTAT_A.values():
        assert c['N'] == 3 and 100 <= _m(c) <= 200 and c['opts']['wstat_min_tiles'] == 0
        assert (c['cout'] + 31) // 32 * 32 == (128 if c['base'] == 'd1024' else 256)


def _inst_by_hand(case, g, t):
    """conv1x1_wstat_inst re-derived from the case: (RES, OUT32, NQ, FAST)."""
    c = case
    joined = bool(c['join'] or c['dual'])
    fl = c['in_fl'] + c['w_fl']
    out_fl = g.v[t][1] if joined else fl
    nq = len(c['readers'] or [])
    out32 = c['out_i32'] or not c['readers']
    shifts = [out_fl - rfl for rfl, _ in (c['readers'] or [])]
    # with the shortcut as the host the ReLU behind the conv is the host's: none
    relu0 = c['relu'] and not (c['dual'] and c['dual'].get('host') == 'shortcut')
    fast = bool(c['opts'].get('wstat_fast', 1)) and all(n > 0 for n in shifts) and (not relu0 or (not joined and not out32))
    return bool(c['join']), out32, nq, fast


@pytest.mark.parametrize('name', sorted(k for k, c in ALL.items() if c['family'] == 'wstat'))
def test_wstat_instance_follows_from_the_case(name):
    """The FAST / output-form fields of the kernel name the table states are those the case's formats, ReLUs and outputs give by
    conv1x1_wstat_inst's rule, and the dense bits those its strides give."""
    case = ALL[name]
    g, _, _, t = _planned(name)
    res, out32, nq, fast = _inst_by_hand(case, g, t)
    assert case['kernel'] == oc.wstat_kern(case['base'], out32, nq, fast), (res, out32, nq, fast)
    assert res == oc.BASES[case['base']][3]
    k1 = oc.BASES[case['base']][1]
    if k1:
        host_sc = case['dual'].get('host') == 'shortcut'
        s_host, s_other = (case['dual']['stride'], 1) if host_sc else (1, case['dual']['stride'])
        assert case['dense'] == (s_host == 1) | (s_other == 1) << 1
    else:
        assert case['dense'] == (case['stride'] == 1)


# ---- schedules

def test_schedule_cases_walk_the_tile_counts_they_name():
    """For 256 compute units under wstat_grid_div = 32: MG = 8 pixel groups (NG = 1); over the launches of a base the groups walk 1, 2, S - 1, S,
    S + 1 and 2 S + 1 tiles, and one launch has T % MG != 0 (neighbouring groups with nt and nt + 1)."""
    seen = {}
    for name, c in dict(oc.WSTAT_SCHED, w_pipelined=oc.WSTAT_PIPELINED).items():
        assert c['opts']['wstat_grid_div'] == 32 and c['opts']['whole_batch_launches'] == 1 and c['opts']['split'] == 1
        T, MG, NG, grid, nts = oc.schedule(_m(c), (c['cout'] + 31) // 32 * 32, c['nw'], 256, 32)
        assert (T, MG, NG, grid) == (c['T'], 8, 1, 8) and set(nts) == oc.SCHED_NT[T] and sum(nts) == T, (name, T, nts)
        assert c['kernel'].split(', ')[4] == 'true' and int(c['kernel'].split(', ')[5]) >= 1        # int32 + int8 stores in the counted waits
        seen.setdefault(c['base'], set()).update(nts)
        seen.setdefault((c['base'], 'uneven'), set()).add(T % MG != 0)
    for base in ('p512', 'r512', 'd512', 'd1024'):
        S = oc.ring(base)
        assert S == (3 if base == 'd1024' else 4)
        assert {1, 2, S - 1, S, S + 1, 2 * S + 1} <= seen[base], (base, seen[base])
        assert True in seen[(base, 'uneven')]


def test_table_b_covers_the_geometry():
    """With the whole device (wstat_grid_div = 0, 256 compute units) every case of table B has T < 256 / NG: MG = T."""
    rem, mgs, ngs, dense, nws = set(), set(), set(), set(), set()
    for name, c in oc.WSTAT_B.items():
        coutP = (c['cout'] + 31) // 32 * 32
        T, MG, NG, grid, nts = oc.schedule(_m(c), coutP, c['nw'], 256, 0)
        assert MG == T and T < 256 // NG and set(nts) == {1} and grid == (T + 7) // 8 * 8 * NG
        rem.add(_m(c) % 32)
        mgs.add(MG)
        ngs.add((c['nw'], NG))
        dense.add((oc.BASES[c['base']][1] > 0, c['dense']))
        P, Q = ic.out_hw(c)
        if c['dense'] != (3 if c['dual'] else 1):
            nws.add((P != Q, Q == 1, P * Q == 1))
    assert {1, 31, 0} <= rem
    assert any(m % 8 for m in mgs) and any(m >= 4 for m in mgs)
    assert {(8, 1), (8, 2), (8, 3), (4, 3)} <= ngs
    assert {(False, 0), (False, 1), (True, 1), (True, 2), (True, 3)} <= dense
    assert (True, False, False) in nws and any(q1 and not one for _, q1, one in nws) and any(one for _, _, one in nws)      # gathered: P != Q, Q == 1, 1 x 1
    assert oc.WSTAT_MAX_BATCH['max_batch'] == 8


def test_ragged_tiles_hold_live_and_dead_lanes():
    ragged = 0
    for name, c in ALL.items():
        tile = {'wstat': 32, 'wreg': 64}.get(c['family'])
        if tile and _m(c) % tile:
            ragged += 1
            assert 0 < _m(c) % tile < tile
    assert ragged > 40
    # conv1x1_wreg_kernel: the second 32-pixel tile of the last workgroup is wholly dead at M % 64 = 1 .. 32
    for ck in (512, 1024):
        assert {_m(c) % 64 for n, c in oc.WREG.items() if n.startswith(f'wr{ck}_M')} == {1, 31, 32, 33, 63, 0}
        grids = {-(-_m(c) // 64) for n, c in oc.WREG.items() if n.startswith(f'wr{ck}')}
        assert any(gr >= 16 for gr in grids) and any(gr % 8 for gr in grids)
        gr = max(grids)
        assert {(w * 2 + b * 3) & 15 for w in range(8) for b in range(gr)} == set(range(16))
    # conv3x3_patch_kernel: the odd image of the 7 x 7 instance's last pair; a grid that is no multiple of 8; 64 live channels on BN = 128
    assert any(c['cin'] == 512 and c['N'] % 2 for c in oc.PATCH.values()) and any(c['grid'] % 8 for c in oc.PATCH.values())
    for cin, hs in ((128, {4, 8, 28}), (256, {7, 21})):
        assert {c['H'] for c in oc.PATCH.values() if c['cin'] == cin} == hs
        for res in (False, True):
            assert {c['cout'] for c in oc.PATCH.values() if c['cin'] == cin and bool(c['join']) == res} & {64, 192}
    assert {c['N'] for c in oc.PATCH.values() if c['cin'] == 512} == {1, 2, 3}
    assert {c['cout'] for c in oc.PATCH.values()} == {64, 128, 192, 256}
    forms = {(c['out_i32'] or not c['readers'], bool(c['readers'])) for c in oc.PATCH.values()}
    assert forms == {(True, False), (False, True), (True, True)}
    assert {c['x_signed'] for c in oc.PATCH.values()} == {False, True}


def test_s2wreg_tap_rotation_takes_all_nine_values():
    """trot = (4 wave + 5 (block / 8) + 2 (block % 8)) % 9 over the live (wave, block) pairs of each image count the cases run."""
    for N in (1, 3, 4, 5):
        blocks = [b for b in range((N + 3) // 4 * 8) if (b >> 3) * 4 + (b & 3) < N]
        assert len(blocks) == 2 * N
        assert {oc.s2_trot(w, b) for w in range(8) for b in blocks} == set(range(9)), N
    assert {c['kernel'] for c in oc.S2WREG.values()} == {f'f8::conv3x3s2_wreg_kernel<{a}>' for a in ('512, 7, 7, 512', '256, 14, 14, 256', '256, 7, 7, 512')}
    for c in oc.S2WREG.values():
        assert c['batches'] == [1, 3, 4, 5] and c['max_batch'] == 5


# ---- the planner's threshold

def _one_conv(cin, cout, max_batch, **opts):
    """A 1x1 conv cin -> cout on an 8 x 8 map (two 32-pixel tiles per image) with one int8 reader: its plan token."""
    net = F8Net()
    for k, v in dict(oc.OPTS, **opts).items():
        net.set_option(k, v)
    t0 = net.input(cin, 8, 8, 8)
    kw = dict(stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False)
    y = net.conv(t0, np.ones((cout, cin, 1, 1), np.int32), None, relu=True, **kw)
    net._L.f8_net_set_label(net._h, y, b'ut')
    r = net.conv(y, np.ones((32, cout, 1, 1), np.int32), None, relu=False, **dict(kw, input_fl=4, quant_input=True))
    net.output(r, as_float=False)
    net.finalize(max_batch)
    (line,) = ic.under_test(net)
    return line


@pytest.mark.parametrize('cin,cout,at,below', [(512, 256, 256, 'f8::conv1x1_wreg_kernel<512, 256>'), (1024, 512, 128, 'f8::conv1x1_wreg_kernel<1024, 512>'),
                                               (512, 512, 128, 'f8::conv_igemm_kernel<')])
def test_wstat_threshold(cin, cout, at, below):
    """tiles >= wstat_min_tiles * max(1, cus / NG) with the default wstat_min_tiles = 2 and the 256 compute units the planner assumes before upload:
    NG 1 -> 512 tiles = 256 images of 8 x 8, NG 2 -> 256 tiles = 128 images.  One image fewer: conv1x1_wreg_kernel where it has the instance."""
    assert F8Net().get_option('wstat_min_tiles') == 2
    tok, kernel = _one_conv(cin, cout, at)
    assert tok == 'conv1x1_wstat:' and kernel == f'f8::conv1x1_wstat_kernel<{cin}, 0, 8, false, false, 1, true>'
    tok, kernel = _one_conv(cin, cout, at - 1)
    assert kernel.startswith(below) and tok.startswith('conv1x1s1_wreg:' if 'wreg' in below else 'conv1x1s1_t'), (tok, kernel)
    assert _one_conv(cin, cout, 1, wstat_min_tiles=0)[0] == 'conv1x1_wstat:'
    assert _one_conv(cin, cout, at, wstat=0)[1].startswith(below)


# ---- option wstat_grid_div

def test_wstat_grid_div_is_a_scheduling_key_and_zero_by_default(monkeypatch):
    assert F8Net().get_option('wstat_grid_div') == 0
    net = F8Net()
    t = net.input(32, 4, 4, 8)
    net.output(net.conv(t, np.ones((32, 32, 1, 1), np.int32), None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False,
                        quant_input=False, relu=True), as_float=False)
    net.finalize(2)
    net.set_option('wstat_grid_div', 32)                          # not a planning key: settable behind finalize
    assert net.get_option('wstat_grid_div') == 32
    for bad in (-1, 33):
        with pytest.raises(_lib.F8Error) as e:
            F8Net().set_option('wstat_grid_div', bad)
        assert e.value.status == F8_ERR_INVALID
    monkeypatch.setenv('F8_WSTAT_GRID_DIV', '8')
    assert F8Net().get_option('wstat_grid_div') == 8


@pytest.mark.parametrize('arch', ['resnet18', 'resnet50', 'mobilenet_v1'])
def test_shipped_plans_do_not_move_with_the_key(arch):
    spec = topology.get(arch, normalize=arch == 'resnet50')
    params = synth.make_params(spec, seed=3)
    for bs in (2, 128):
        a = build_net(spec, params, max_batch=bs, hw=224)
        for v in (0, 32):
            b = build_net(spec, params, max_batch=bs, hw=224, options={'wstat_grid_div': v})
            assert a.get_option('wstat_grid_div') == 0 and a.describe() == b.describe()
            assert [a.launch_kernel(i) for i in range(a.num_launches)] == [b.launch_kernel(i) for i in range(b.num_launches)]


# ---- liveness on the oracle's values

def _forms(name):
    """[(label, int32 value the launch requantises, int8 value, shift, signed)] of the int8 forms the launch under test writes."""
    case = ALL[name]
    g, _, _, t = _planned(name)
    if not case['readers']:
        return []
    v, fl = g.v[t]
    out = []
    for (rfl, sgn), (label, xq, s2) in zip(case['readers'], [tp for tp in g.taps if tp[0].startswith('reader')]):
        assert sgn == s2
        out.append((label, v.astype(np.int64), xq, fl - rfl, sgn))
    assert len(out) == len(case['readers'])
    return out


def _joined_sum(name):
    """The aligned sum of a join before its clamp, as wrapping int32 arithmetic gives it; None without a join."""
    case = ALL[name]
    g, _, y, t = _planned(name)
    if not (case['join'] or case['dual']):
        return None
    ov, (acc_shl, res_shl) = g.v[g.other][0], g.shl
    s = ((g.v[y][0].astype(np.int64) << acc_shl) + (ov.astype(np.int64) << res_shl)) & 0xFFFFFFFF
    return np.where(s >= 2 ** 31, s - 2 ** 32, s)


def _windows(x, k, stride, pad, P, Q):
    """{(r, s): the input values tap (r, s) multiplies, [N, C, P, Q]} with zeros outside the image."""
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    return {(r, s): xp[:, :, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] for r in range(k) for s in range(k)}


def _slice_products(x, w, stride, pad, P, Q):
    """{(r, s, K32 step): that slice's contribution to the result, [cout, N * P * Q]} (exact in float64: below 2^53)."""
    out = {}
    for (r, s), xs in _windows(x, w.shape[2], stride, pad, P, Q).items():
        A = xs.transpose(1, 0, 2, 3).reshape(xs.shape[1], -1).astype(np.float64)
        for k0 in range(0, w.shape[1], 32):
            out[(r, s, k0 // 32)] = w[:, k0:k0 + 32, r, s].astype(np.float64) @ A[k0:k0 + 32]
    return out


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure.  Every int8 form the launch writes has at least 16 distinct values, reaches each end of its clamp and keeps at
    most a quarter of its values at each (behind a ReLU the lower end of a signed form is the floor's 0); a right shift meets an exact tie above
    an even and above an odd quotient.  A join's sum exceeds 2^30 somewhere and is exactly -2^31 somewhere (the value the clamp at -(2^31 - 1)
    changes); a ReLU has values on both sides of its floor; every K32 step of every product of the launch (9 taps x cin / 32 for the 3x3 kernels,
    both products of the dual pair) changes the result: zeroing that slice of the weights would."""
    case = ALL[name]
    g, outs, y, t = _planned(name)
    joined = bool(case['join'] or case['dual'])
    for o in outs:
        assert np.unique(g.v[o][0]).size > 8
    for label, v, xq, n, sgn in _forms(name):
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        floored = case['join_relu'] if joined else case['relu']
        assert (xq == (0 if floored else lo)).any() and (xq == hi).any(), (label, int(xq.min()), int(xq.max()))
        assert (xq == lo).mean() <= 0.25 and (xq == hi).mean() <= 0.25, (label, (xq == lo).mean(), (xq == hi).mean())
        if n > 0:
            tie = (v & ((1 << n) - 1)) == (1 << (n - 1))
            q = v >> n
            inside = tie & (q >= lo) & (q < hi)
            assert (inside & (q % 2 == 0)).any() and (inside & (q % 2 == 1)).any(), (label, int(tie.sum()))
    s = _joined_sum(name)
    if s is not None:
        assert case['clamp']
        assert (np.abs(s) > 2 ** 30).any(), 'no joined value above 2^30'
        assert (s == -2 ** 31).any(), 'no joined value the clamp changes'
        assert (g.v[t][0] >= -(2 ** 31 - 1)).all()
    if case['relu']:
        raw = g.raw[y]
        assert (raw < 0).mean() > 0.01 and (raw > 0).mean() > 0.25, ((raw < 0).mean(), (raw > 0).mean())
    if case['join_relu']:
        assert (s < 0).mean() > 0.01 and (s > 0).mean() > 0.25
    if case['o_set']:
        ov = g.v[g.other][0]
        for ch, val in case['o_set'].items():
            assert (ov[:, ch] == val).all()
    if case['bias_big']:
        raw = g.raw[y].astype(np.int64)
        assert (raw > 2 ** 31 - 2 ** 13).any() and (raw < -2 ** 31 + 2 ** 13).any()
    P, Q = ic.out_hw(case)
    for label, x, w, stride, pad in oc.k_slices(case, g):
        prods = _slice_products(x, w, stride, pad, P, Q)
        assert len(prods) == w.shape[2] ** 2 * w.shape[1] // 32
        for key, contrib in prods.items():
            assert contrib.any(), (label, key)


@pytest.mark.parametrize('name', sorted(oc.S2WREG))
def test_s2wreg_every_tap_is_live_in_every_border_class(name):
    """Zeroing one tap's weights changes the result at a corner, a top-row, a left-column and an interior pixel wherever that tap lies inside the
    image there (the taps of row / column 0 multiply the padding in the top row / left column: real zeros to the oracle) — and at the interior
    pixel for all nine."""
    case = oc.S2WREG[name]
    g, _, y, _ = _planned(name)
    P, Q = ic.out_hw(case)
    (label, x, w, stride, pad), = oc.k_slices(case, g)
    for (r, s), xs in _windows(x, 3, 2, 1, P, Q).items():
        contrib = np.einsum('ncpq,oc->nopq', xs.astype(np.float64), w[:, :, r, s].astype(np.float64))
        for (p, q), inside in (((0, 0), r > 0 and s > 0), ((0, Q // 2), r > 0), ((P // 2, 0), s > 0), ((P // 2, Q // 2), True)):
            assert contrib[:, :, p, q].any() == inside, (r, s, p, q)
