"""Case tables of the op-level tests of the operand-stationary conv launches: conv1x1_wstat_kernel (f8_wstat.hip), conv1x1_wreg_kernel
(f8_wreg.hip), conv3x3s2_wreg_kernel (f8_s2conv.hip) and conv3x3_patch_kernel (f8_conv3x3.hip): tests/test_ostat_plan.py (plan, symbols, schedules
and liveness on the oracle, no GPU) and tests/test_gpu_ostat.py (every case against the oracle on the device).  No test functions here.

The graphs are those of tests/igemm_cases.py (build_graph: [1x1 producer] -> the conv under test -> [join with `other` | the dual pair] -> one 1x1
reader per int8 form, `out_i32` for the int32 result), planned with wstat = wreg = s2wreg = patch3x3 = 1 and split = 1 (a run is ONE launch over
its images, so that M, the tile count and the grid below are those of the run).

The expected plan token and kernel instance of every case are WRITTEN BY HAND from conv_variant (f8_net.cpp), conv1x1_wstat_supported /
conv1x1_wstat_waves / conv1x1_wstat_inst / conv1x1_wstat_kernel_name, conv1x1_wreg_supported, conv3x3s2_wreg_supported and conv3x3_patch_config;
nothing here asks the planner for them.
  conv1x1_wstat_kernel<K0, K1, NW, RES, OUT32, NQ, FAST>: K0 the bytes per pixel of the conv that carries the join (the host), K1 those of the dual
    pair's other conv; NW 4 where K0 + K1 > 1024, else 8; RES a join with an int32 tensor; OUT32 / NQ the int32 form and the number of int8 forms
    the launch writes; FAST: option wstat_fast, every int8 form shifts right (n > 0) and the ReLU behind the conv is off unless there is neither a
    join nor an int32 output.
  Bases: <512, 0, 8, false> and <1024, 0, 8, false> (coutP % 256 == 0), <512, 0, 8, true> (the same with a join), <512, 256, 8, false>
    (coutP % 256 == 0) and <1024, 512, 4, false> (coutP % 128 == 0): the host reads 512 / 1024 channels, the other conv 256 / 512.
  conv_variant takes the kernel at any stride where tiles >= wstat_min_tiles * max(1, cus / NG); the tables run it with wstat_min_tiles = 0.
  Schedule (launch_wstat_t): T = ceil(M / 32) tiles, NG = coutP / (32 NW) channel groups, MG = max(1, cus' / NG) pixel groups clamped to T, where
    cus' = max(1, cus / wstat_grid_div) under that option; grid = ceil(MG / 8) * 8 * NG; pixel group mg walks tiles mg T / MG .. (mg + 1) T / MG.
  The ring has S = 4 slots (3 on <1024, 512, 4>: 4 x 32 x 1536 bytes exceed 128 KB).
  dense (bit 0: the host's rows, bit 1: the other conv's): the rows are the output pixels in order, i.e. that conv has stride 1.
  conv1x1_wreg_kernel<CK, COUT>: 1x1 / 1 without a join or an int32 form, (512, 256) and (1024, 512), where wstat does not take the conv.
  conv3x3s2_wreg_kernel<CIN, HO, WO, COUT>: 3x3 / 2 / pad 1, int8 forms only, on an input of 2 HO x 2 WO.
  conv3x3_patch_kernel<CIN, W, R, IMGS, BN, KB, HAS_RES>: 3x3 / 1 / pad 1 with coutP >= 64: (128, 28, 4, 1, 128, 128) where H % 4 == 0,
    (256, 14, 7, 1, 128, 128) where H % 7 == 0, (512, 7, 7, 2, 64, 256) on 7 x 7 maps; token conv3x3s1_patch_R<R>x<IMGS>_bn<BN>[_res]."""
import igemm_cases as ic

OPTS = dict(wstat=1, wreg=1, s2wreg=1, patch3x3=1, split=1)
MIN0 = dict(wstat_min_tiles=0)
SCHED = dict(wstat_min_tiles=0, wstat_grid_div=32, whole_batch_launches=1)
_U, _S, _S3 = (4, False), (4, True), (3, True)
_tf = ic._tf

# base -> (K0, K1, NW, RES)
BASES = {'p512': (512, 0, 8, False), 'p1024': (1024, 0, 8, False), 'r512': (512, 0, 8, True), 'd512': (512, 256, 8, False), 'd1024': (1024, 512, 4, False)}
FORMS = [(True, 0), (True, 1), (True, 2), (False, 1), (False, 2)]          # (OUT32, NQ)


def ring(base):
    k0, k1 = BASES[base][:2]
    return 4 if 4 * 32 * (k0 + k1) <= 128 * 1024 else 3


def wstat_kern(base, out32, nq, fast):
    k0, k1, nw, res = BASES[base]
    return f'f8::conv1x1_wstat_kernel<{k0}, {k1}, {nw}, {_tf(res)}, {_tf(out32)}, {nq}, {_tf(fast)}>'


def wstat_token(base):
    k0, k1, nw, res = BASES[base]
    return 'conv1x1_wstat_dual:' if k1 else 'conv1x1_wstat_res:' if res else 'conv1x1_wstat:'


def all_wstat_instances():
    """Every instance launch_conv1x1_wstat can dispatch: 5 bases x 5 output forms x FAST."""
    return {wstat_kern(b, o, q, f) for b in BASES for o, q in FORMS for f in (False, True)}


def schedule(M, coutP, nw, cus, div):
    """(T, MG, NG, grid, [tiles of each pixel group]) of launch_wstat_t, by hand."""
    T, NG = (M + 31) // 32, coutP // (32 * nw)
    if div > 0:
        cus = max(1, cus // div)
    MG = min(max(1, cus // NG), T)
    return T, MG, NG, (MG + 7) // 8 * 8 * NG, [(mg + 1) * T // MG - mg * T // MG for mg in range(MG)]


def _ws(base, out32, nq, fast, H, W, N=3, cout=None, readers=None, opts=None, dual_stride=1, host=None, pre=False, **kw):
    """A case on conv1x1_wstat_kernel.  `fast` is stated by the caller; the readers default to the form: none, one, or an unsigned and a signed one
    with different fraclens."""
    k0, k1, nw, res = BASES[base]
    cout = cout or (128 if base == 'd1024' else 256)
    if readers is None:
        readers = [None, [_U], [_U, _S3]][nq]
    kw.setdefault('relu', True)
    if res or k1:
        kw.setdefault('join_relu', False)
        if nq == 1 and readers == [_U] and not kw['join_relu']:
            readers = [_S]                                        # (a join without a ReLU behind it spreads around 0)
    c = dict(opts=dict(dict(OPTS, **MIN0), **(opts or {})), readers=readers, out_i32=bool(out32 and nq), H=H, W=W, N=N)
    if k1:
        d = dict(mid=k0, stride=dual_stride)
        if host == 'shortcut':                                    # the shortcut hosts: it reads K0 bytes, the conv under test K1 (and carries no ReLU)
            d = dict(mid=k1, stride=dual_stride, host='shortcut')
            c.update(c0=k0)
        else:
            c.update(c0=k1)
        c.update(dual=d)
        cin = d['mid']
    else:
        cin = k0
        if res:
            c.update(join='other')
        if pre:
            c.update(pre=dict(w_fl=5, relu=True), in_fl=4, c0=32)
    c.update(kw)
    case = ic._case(1, cin, cout, wstat_token(base), wstat_kern(base, out32, nq, fast), **c)
    case.update(family='wstat', base=base, nw=nw, S=ring(base), dense=(1 if (k1 == 0 and case['stride'] == 1) or (k1 and (host != 'shortcut' or dual_stride == 1)) else 0) |
                (2 if k1 and (host == 'shortcut' or dual_stride == 1) else 0))
    return case


# ================================================================================================================================================
# conv1x1_wstat_kernel, table A: one case per instance.  All 50 are reachable: FAST by a conv without ReLU (or, without a join and an int32 form,
# with one), the general epilogue by a ReLU behind the conv in front of a join or an int32 form, or by wstat_fast = 0; no line of
# conv1x1_wstat_inst excludes a combination.  Three images, three runs; 7 x 9 maps (189 pixels: 6 tiles, the last with 29 live rows), 5 x 7 on
# <1024, 0, 8> and 6 x 6 on <1024, 512, 4>; coutP 256 (128 on <1024, 512, 4>).
MAPS = {'p512': (7, 9), 'r512': (7, 9), 'd512': (7, 9), 'p1024': (5, 7), 'd1024': (6, 6)}
WSTAT_A = {}
for _b in BASES:
    _joined = BASES[_b][3] or BASES[_b][1] > 0
    for _o, _q in FORMS:
        for _f in (False, True):
            # FAST: no ReLU behind the conv (with one where nothing but int8 forms leave a plain conv: the floor rides in the clamp).
            # general: the ReLU in front of a join / next to an int32 form; a plain conv with int8 forms only has it under wstat_fast = 0 alone
            _plain8 = not _joined and not _o
            _relu = (_q == 2) if (_f and _plain8) else not _f
            _opts = {'wstat_fast': 0} if (not _f and _plain8) else {}
            WSTAT_A[f'wa_{_b}_{"i32" if _o else "i8"}_{_q}_{"fast" if _f else "gen"}'] = _ws(
                _b, _o, _q, _f, *MAPS[_b], relu=_relu, opts=_opts, join_relu=_joined and _q == 1 and not _o)

# ================================================================================================================================================
# Table B: geometry.  Without wstat_grid_div the device's compute units / NG exceed every T here: MG = T, one tile per pixel group, grid
# ceil(T / 8) * 8 * NG (the workgroups of the last eight with mg >= MG return), weight rotations mg & 3 = 0 .. 3 all live from T = 4 on.
WSTAT_B = {
    'wb_M33': _ws('p512', False, 1, True, 3, 11, N=1),                          # M % 32 == 1: T 2
    'wb_M63': _ws('p512', False, 1, True, 7, 9, N=1),                           # M % 32 == 31
    'wb_M96': _ws('p512', False, 1, True, 4, 8),                                # M % 32 == 0: T 3
    'wb_T13': _ws('p512', False, 1, True, 7, 19),                               # 399 pixels: T = MG = 13, grid 16: three workgroups return
    'wb_T5_res': _ws('r512', True, 1, False, 7, 7, pre=True),                   # 147 pixels: T = MG = 5
    'wb_cout768': _ws('p512', False, 1, True, 7, 9, cout=768),                  # NG 3: T = MG = 6, grid 24
    'wb_cout768_res': _ws('r512', True, 0, True, 7, 9, cout=768, relu=False),
    'wb_cout512_1024': _ws('p1024', False, 2, True, 5, 7, cout=512),            # NG 2
    'wb_cout384_dual1024': _ws('d1024', False, 1, False, 6, 6, cout=384),       # NG 3 on four waves
    'wb_cout512_dual': _ws('d512', True, 1, False, 7, 9, cout=512),             # NG 2
    'wb_s2_plain': _ws('p512', False, 1, True, 9, 13, stride=2),                # 5 x 7 outputs gathered from a 9 x 13 map: dense 0
    'wb_s2_plain_1024': _ws('p1024', True, 1, False, 11, 7, stride=2),          # 6 x 4
    'wb_s3_plain': _ws('p512', False, 1, True, 10, 13, stride=3),               # 4 x 5
    'wb_dual_s2_host_body': _ws('d512', False, 1, False, 9, 13, dual_stride=2),             # the body's rows dense, the shortcut's gathered: dense 1
    'wb_dual_s2_host_shortcut': _ws('d512', False, 1, True, 9, 13, dual_stride=2, host='shortcut', relu=False),     # x gathered, x2 dense: dense 2
    'wb_dual1024_s2_host_shortcut': _ws('d1024', True, 1, True, 11, 7, dual_stride=2, host='shortcut', relu=False),
    'wb_dual_s1_host_shortcut': _ws('d512', False, 1, True, 5, 7, host='shortcut', relu=False),                     # dense 3
    'wb_Q1_gather': _ws('p512', False, 1, True, 9, 1, stride=2, N=5),           # 5 x 1 outputs: the decode divides by Q = 1
    'wb_Q1_dense': _ws('p512', False, 1, True, 37, 1, N=1),
    'wb_1x1_gather': _ws('p512', False, 1, True, 2, 2, stride=2, N=7),          # 1 x 1 outputs: PQ = 1, one image per row
    'wb_1x1_dense': _ws('r512', False, 1, True, 1, 1, N=7, relu=False),
    'wb_1x1_dual_s2': _ws('d512', False, 1, True, 2, 1, dual_stride=2, host='shortcut', relu=False, N=7),
}
# planned for 8 images; 1, 3 and 8 run from the same handle (T 2, 6, 16)
WSTAT_MAX_BATCH = _ws('d512', True, 1, False, 7, 9, N=8, dual_stride=1, join_relu=True)

# ================================================================================================================================================
# Table C: epilogues.  7 x 9 maps, 512 -> 256; the conv's fraclen is 13 (in 8 + w 5, or in 4 + w 9 behind the producer).
_MIN, _MAX = -2 ** 31, 2 ** 31 - 1
WSTAT_C = {
    # the two align directions of each join: 13 against 15 (acc_shl 2) and against 10 (res_shl 3)
    'wc_res_acc_shl': _ws('r512', False, 1, True, 7, 9, readers=[(5, True)], o_fl=15, relu=False),
    'wc_res_res_shl': _ws('r512', True, 1, False, 7, 9, o_fl=10),
    'wc_dual_acc_shl': _ws('d512', False, 1, False, 7, 9, readers=[(5, True)], o_fl=15),
    'wc_dual_res_shl': _ws('d512', True, 1, True, 7, 9, o_fl=10, relu=False),
    'wc_dual1024_res_shl': _ws('d1024', False, 2, True, 6, 6, o_fl=11, relu=False),
    # ReLU behind the conv and behind the join, on and off
    'wc_res_relu_relu': _ws('r512', False, 1, False, 7, 9, join_relu=True, pre=True),
    'wc_res_norelu_relu': _ws('r512', False, 1, True, 7, 9, join_relu=True, relu=False, o_fl=12),
    'wc_dual_relu_norelu': _ws('d512', False, 2, False, 7, 9),
    'wc_plain_norelu_signed': _ws('p512', False, 1, True, 7, 9, readers=[_S], relu=False),
    'wc_plain_relu_signed': _ws('p512', False, 1, True, 7, 9, readers=[_S3]),                # the floor rides in the signed form's lower clamp
    'wc_plain_pre_signed_in': _ws('p512', True, 2, False, 7, 9, pre=True, in_signed=True),
    # a reader that shifts left / not at all forces the general epilogue by itself (fraclens 2 + 3 = 5, inputs in [0, 3])
    'wc_left_shift': _ws('p512', False, 2, False, 7, 9, readers=[(4, False), (6, True)], x_fl=2, w_fl=3, x_hi=3, spread=25.0, bias_set={3: 600, 4: 505, 6: 2}),
    'wc_shift0': _ws('p512', False, 1, False, 7, 9, readers=[(5, True)], x_fl=2, w_fl=3, x_hi=3, spread=50.0, relu=False),
    # the residual operand at the ends of int32 (channels 12 / 13 of `other` are exactly those)
    'wc_res_int32_ends': _ws('r512', True, 1, True, 7, 9, o_set={12: _MIN, 13: _MAX, 14: _MIN + 1}, relu=False),
    'wc_res_int32_ends_shl': _ws('r512', True, 2, False, 7, 9, o_set={12: _MIN, 13: _MAX, 14: _MIN + 1}, o_fl=12),
    'wc_dual_int32_ends': _ws('d512', True, 1, True, 7, 9, o_set={12: _MIN, 13: _MAX}, relu=False),
    'wc_bias_big': _ws('p512', True, 2, False, 7, 9, bias_big=True),                        # accumulators next to +-2^31: the rounding add wraps
}

# ================================================================================================================================================
# Schedules: wstat_grid_div = 32 (eight compute units' worth of pixel groups on 256: MG = 8 with NG 1), whole_batch_launches = 1, int32 + int8
# outputs (4 + 1 or 4 + 2 stores per thread and tile in the counted waits), three runs.  T -> tiles per pixel group on MG = 8:
#   12 -> 1, 2 (T % MG != 0)   28 -> 3, 4   36 -> 4, 5 (T % MG != 0)   72 -> 9   56 -> 7
# S = 4: nt = 1, 2, S - 1, S, S + 1, 2 S + 1 = 1, 2, 3, 4, 5, 9;  S = 3 (<1024, 512, 4>): 1, 2, 2, 3, 4, 7.
SCHED_MAPS = {12: (11, 11), 28: (17, 17), 36: (15, 25), 72: (19, 40), 56: (19, 31)}       # three images: 363, 867, 1125, 2280, 1767 pixels
WSTAT_SCHED = {}
for _b, _ts in (('p512', (12, 28, 36, 72)), ('r512', (12, 28, 36, 72)), ('d512', (12, 28, 36, 72)), ('d1024', (12, 28, 56))):
    for _i, _t in enumerate(_ts):
        _q = 1 + _i % 2
        WSTAT_SCHED[f'ws_{_b}_T{_t}'] = dict(_ws(_b, True, _q, False, *SCHED_MAPS[_t], opts=SCHED, join_relu=_b != 'p512' and _q == 1), T=_t)
# nt of the pixel groups for 256 compute units
SCHED_NT = {12: {1, 2}, 28: {3, 4}, 36: {4, 5}, 72: {9}, 56: {7}}
# bench.py's schedule: arena_copies 3, pipeline_depth 3, set_pipelined(2), three inputs over nine runs
WSTAT_PIPELINED = dict(_ws('r512', True, 1, False, 15, 25, opts=dict(SCHED, arena_copies=3, pipeline_depth=3), join_relu=True), T=36)

# ================================================================================================================================================
# conv1x1_wreg_kernel<512, 256> / <1024, 512>: a workgroup per 64 pixels (two 32-pixel tiles), grid ceil(M / 64); reached below the wstat threshold
# (the default wstat_min_tiles = 2: 512 / 256 tiles, i.e. 16 k / 8 k pixels) and, 'off', with wstat = 0.
def _wr(ck, H, W, N, readers=None, opts=None, **kw):
    cout = ck // 2
    c = ic._case(1, ck, cout, 'conv1x1s1_wreg:', f'f8::conv1x1_wreg_kernel<{ck}, {cout}>', H=H, W=W, N=N, readers=readers or [_U], opts=dict(OPTS, **(opts or {})), **kw)
    c.update(family='wreg')
    return c


WREG = {}
for _ck in (512, 1024):
    WREG.update({
        f'wr{_ck}_M65': _wr(_ck, 5, 13, 1),                                     # M % 64 == 1: the second pixel tile is wholly dead
        f'wr{_ck}_M95': _wr(_ck, 5, 19, 1, relu=False),                         # 31
        f'wr{_ck}_M96': _wr(_ck, 4, 8, 3, readers=[_U, _S3]),                   # 32: dead to the lane
        f'wr{_ck}_M97': _wr(_ck, 97, 1, 1, readers=[_S], relu=False),           # 33: one live lane in the second tile
        f'wr{_ck}_M127': _wr(_ck, 1, 127, 1, opts={'wstat': 0}),                # 63
        f'wr{_ck}_M192': _wr(_ck, 8, 8, 3, readers=[_U, _S3], relu=False),      # 0: grid 3
        f'wr{_ck}_grid17': _wr(_ck, 16, 13, 5, pre=dict(w_fl=5, relu=True), in_fl=4, c0=32),    # 1040 pixels: 17 workgroups, every rot = (2 wave + 3 block) & 15
    })
WREG['wr512_left_shift'] = _wr(512, 7, 9, 3, readers=[(4, False), (6, True)], x_fl=2, w_fl=3, x_hi=3, spread=25.0, bias_set={3: 600, 4: 505, 6: 2})
WREG['wr1024_shift0'] = _wr(1024, 7, 9, 3, readers=[(5, True)], x_fl=2, w_fl=3, x_hi=3, spread=50.0, relu=False)


# ================================================================================================================================================
# conv3x3s2_wreg_kernel: grid ceil(N / 4) * 8, workgroup -> image (block / 8) * 4 + (block & 3) and half (block & 7) >> 2 (rows on 14 x 14
# outputs, channel tiles on 7 x 7).  Handles finalized for 5 images run 1, 3, 4 and 5.
def _s2(cin, ho, cout, readers=None, **kw):
    if kw.get('x_signed'):
        kw.setdefault('x_fl', 4)                                  # (a signed 8-bit format has at most 7 fractional bits)
    c = ic._case(3, cin, cout, 'conv3x3s2_wreg:', f'f8::conv3x3s2_wreg_kernel<{cin}, {ho}, {ho}, {cout}>', H=2 * ho, W=2 * ho, N=5, stride=2, pad=1,
                 readers=readers or [_U], opts=dict(OPTS), **kw)
    c.update(family='s2wreg', batches=[1, 3, 4, 5])
    return c


S2WREG = {}
for _cin, _ho, _cout in ((512, 7, 512), (256, 14, 256), (256, 7, 512)):
    _n = f's2_{_cin}_{_ho}_{_cout}'
    S2WREG[f'{_n}_u'] = _s2(_cin, _ho, _cout)                                                  # unsigned input: border-class biases (ncc > 0)
    S2WREG[f'{_n}_s_norelu'] = _s2(_cin, _ho, _cout, x_signed=True, relu=False, readers=[_S])    # signed: the padding is a real 0
    S2WREG[f'{_n}_u_two'] = _s2(_cin, _ho, _cout, readers=[_U, _S3], relu=False)
S2WREG['s2_256_14_256_s_two'] = _s2(256, 14, 256, x_signed=True, readers=[_U, _S3])


def s2_trot(wave, block):
    """The tap rotation of conv3x3s2_wreg_kernel, by hand."""
    return (wave * 4 + (block >> 3) * 5 + (block & 7) * 2) % 9


# ================================================================================================================================================
# conv3x3_patch_kernel: tiles = N * H / R (IMGS 1) or ceil(N / 2) (the 7 x 7 instance: two images per tile), grid = tiles * ceil(coutP / BN).
_PATCH = {128: (28, 4, 1, 128, 128), 256: (14, 7, 1, 128, 128), 512: (7, 7, 2, 64, 256)}


def _p3(cin, H, cout, N, res=False, readers=None, out_i32=False, **kw):
    W, R, imgs, bn, kb = _PATCH[cin]
    if kw.get('x_signed'):
        kw.setdefault('x_fl', 4)
    if res:
        kw.update(join='other')
        kw.setdefault('join_relu', True)
    if readers is None and not out_i32:
        readers = [_S] if res and not kw['join_relu'] else [_U]
    c = ic._case(3, cin, cout, f'conv3x3s1_patch_R{R}x{imgs}_bn{bn}{"_res" if res else ""}:', f'f8::conv3x3_patch_kernel<{cin}, {W}, {R}, {imgs}, {bn}, {kb}, {_tf(res)}>',
                 H=H, W=W, N=N, pad=1, readers=readers, out_i32=out_i32 and bool(readers), opts=dict(OPTS), **kw)
    tiles = -(-N // 2) if imgs == 2 else N * H // R
    c.update(family='patch', grid=tiles * -(-((cout + 31) // 32 * 32) // bn), bn=bn)
    return c


PATCH = {
    # (128, W 28): rows of 4; H 4, 8, 28
    'p3_128_H4_c64': _p3(128, 4, 64, 3),                                        # coutP 64 on BN 128: the upper half of the weight stage is past the buffer
    'p3_128_H4_c64_res': _p3(128, 4, 64, 3, res=True),
    'p3_128_H8_c128_i32': _p3(128, 8, 128, 2, out_i32=True),                    # int32 only
    'p3_128_H8_c192_res_both': _p3(128, 8, 192, 2, res=True, readers=[_U], out_i32=True),
    'p3_128_H28_c192': _p3(128, 28, 192, 1, x_signed=True, readers=[_S], relu=False),      # 7 tiles x 2: grid 14
    'p3_128_H28_c256_res': _p3(128, 28, 256, 1, res=True, join_relu=False),
    # (256, W 14): rows of 7; H 7, 21
    'p3_256_H7_c64_res_i32': _p3(256, 7, 64, 3, res=True, out_i32=True),
    'p3_256_H7_c192': _p3(256, 7, 192, 3, readers=[_U, _S3]),
    'p3_256_H21_c128': _p3(256, 21, 128, 1, x_signed=True, readers=[_S]),
    'p3_256_H21_c256_res': _p3(256, 21, 256, 1, res=True, readers=[_U], out_i32=True),
    'p3_256_H21_c64_both': _p3(256, 21, 64, 1, readers=[_U], out_i32=True),
    # (512, 7 x 7): image pairs; N 1, 2, 3 (the last pair of 3 holds one image)
    'p3_512_N1_c64': _p3(512, 7, 64, 1),
    'p3_512_N2_c128_res': _p3(512, 7, 128, 2, res=True),
    'p3_512_N3_c192_res': _p3(512, 7, 192, 3, res=True, join_relu=False),       # 2 tiles x 3: grid 6
    'p3_512_N3_c256_both': _p3(512, 7, 256, 3, readers=[_U, _S3], out_i32=True),
    'p3_512_N3_c64_i32_signed': _p3(512, 7, 64, 3, x_signed=True, out_i32=True, relu=False),
    'p3_512_N3_c192': _p3(512, 7, 192, 3, x_signed=True, readers=[_S], relu=False),
}

WSTAT = dict(WSTAT_A, **WSTAT_B, **WSTAT_C, **WSTAT_SCHED)
CASES = dict(WSTAT, **WREG, **S2WREG, **PATCH)


def k_slices(case, g):
    """[(label, int8 input the product reads [N, K, P, Q'], weights [cout, K, k, k], stride, pad)] of the products of the launch under test."""
    c = case
    x = next(iter(g.v.values()))[0]
    body = [tp[1] for tp in g.taps if tp[0] == 'under_test']      # (the requantised form, where the conv does not read the net input itself)
    out = [('ut', body[0] if body else x, g.weights['ut'], c['stride'], c['pad'])]
    if c['dual']:
        out.append(('other', x, g.weights['other'], c['dual']['stride'], 0))
    return out
