"""The fused head launches (f8_stem.hip) at op level: every instance of stem_pool_kernel, stem_rows_kernel and its H2 form (table A), the corners of
their geometry (table B), the forms of their epilogues (table C) — tests/stem_cases.py — and their schedules (persistent workgroups on both patch
buffers, fewer images than max_batch, runs in flight, the int32 entry's range check), bit for bit against the CPU oracle's op-by-op value.
tests/test_stem_plan.py checks on the CPU that every case plans the launch the table names and is live on the oracle's values."""
import numpy as np
import pytest
import torch

import stem_cases as sc
from f8net_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _check_plan(case, net):
    assert sc.head_lines(net) == ([sc.expect(case)] if case['kernel'] else []), net.describe()
    assert (sc.RAW_WORDING in net.describe()) == case['raw_plan'], net.describe()


def _compare(got, wants, n, msg):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(wants)
    for k, (o, want) in enumerate(zip(got, wants)):
        np.testing.assert_array_equal(o.cpu().numpy().reshape((n,) + want.shape[1:]), want[:n], err_msg=f'{msg} output {k}')


def _run_case(name, case, dev, batches=None, repeats=1, one_launch=False):
    data = sc.make_data(name, case)
    g, outs, _ = sc.plan(name, case, data['x'])
    _check_plan(case, g.net)
    if one_launch:                                               # the tile counts of the schedule tests are those of ONE launch over the whole run
        assert sc.head_launches(g.net, case['N']) == 1, g.net.describe()
    wants = [g.v[o][0] for o in outs]
    for n in batches or [case['N']]:
        for rep in range(repeats):
            _compare(sc.run_entry(g.net, case, data, dev, n), wants, n, f'{name} n={n} run {rep}')
    g.net.check()
    _check_plan(case, g.net)
    return g, wants


@pytest.mark.parametrize('name', sorted(sc.TABLE_A))
def test_every_instance(name, dev):
    """Three images on a handle finalized for three, three runs each; the entry of the case selects the kernel's KIND."""
    _run_case(name, sc.TABLE_A[name], dev, repeats=3)


@pytest.mark.parametrize('name', sorted(sc.TABLE_B))
def test_geometry(name, dev):
    _run_case(name, sc.TABLE_B[name], dev)


@pytest.mark.parametrize('name', sorted(sc.TABLE_C))
def test_epilogue(name, dev):
    _run_case(name, sc.TABLE_C[name], dev)


# ---- schedules

def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize('entry', sc.ENTRIES)
@pytest.mark.parametrize('name', sorted(sc.SCHED_ROWS))
def test_rows_persistent(name, entry, dev):
    """The row kernel's persistent loop: more band tiles than workgroups (stem_grid_div = 32: eight workgroups on 256 compute units), so that a
    workgroup walks several bands through both patch buffers, the loader waves fetch band d + G, and tile_of sees ntiles % 8 != 0 (27 tiles)."""
    c = sc.SCHED_ROWS[name]
    case = sc._resnet(c['H'], c['W'], 'rows', entry=entry, N=c['N'], opts=c['opts'], shift=6)
    ntiles = c['N'] * -(-(c['H'] // 4) // sc.RB)
    grid = min(ntiles, (_cus(dev) // 32 + 7) // 8 * 8)              # launch_stem_pool, by hand
    if name == 's_rows_9x60x8':
        assert ntiles == 27 and ntiles >= 3 * grid, f'{ntiles} band tiles on {grid} workgroups: no workgroup reaches its third band on this device'
    else:
        assert ntiles >= 2 * grid, (ntiles, grid)
    _run_case(f'{name}_{entry}', case, dev, repeats=3, one_launch=True)


@pytest.mark.parametrize('entry', sc.ENTRIES)
def test_h2_persistent(entry, dev):
    """The same for the H2 form: 9 images of 60 x 8 -> 30 output rows, bands of 14 / 14 / 2: 27 band tiles."""
    c = sc.SCHED_H2
    case = sc._h2(c['H'], c['W'], entry=entry, N=c['N'], opts=c['opts'])
    ntiles = c['N'] * -(-(c['H'] // 2) // sc.H2_RB)
    grid = min(ntiles, (_cus(dev) // 32 + 7) // 8 * 8)
    assert ntiles == 27 and ntiles >= 3 * grid, f'{ntiles} band tiles on {grid} workgroups: no workgroup reaches its third band on this device'
    _run_case(f's_h2_{entry}', case, dev, repeats=3, one_launch=True)


def test_tile_kernel_persistent(dev):
    """The tile kernel's persistent loop (both patch slots, the next tile's raw loads in registers across the epilogue) runs only where a launch has
    more tiles than compute units x stem_wpc resident workgroups.  That number is a property of the device, not of the case: with stem_wpc = 1 a
    256-unit device needs more than 512 tiles for a workgroup to reach it = 2, and an image has at most 56 of them (224 x 224, the widest input
    the head takes) — 10 images, 6 MB of int32 input.  This is the one large shape of the suite; it cannot be smaller."""
    cus = _cus(dev)
    N = 2 * cus // 56 + 1
    case = sc._resnet(224, 224, 'tile', N=N, opts={'stem_rows': 0, 'stem_wpc': 1, 'split': 1}, shift=6)
    assert N * 56 > 2 * cus * 1
    _run_case('s_tile_persistent', case, dev, one_launch=True)


@pytest.mark.parametrize('form', ['rows', 'h2'])
def test_fewer_images_than_max_batch(form, dev):
    """Planned for 8 images; 1, 3 and 8 from the same handle."""
    case = sc._resnet(36, 120, 'rows', N=8, shift=6) if form == 'rows' else sc._h2(32, 60, N=8)
    _run_case(f'max_batch_{form}', case, dev, batches=[1, 3, 8])


def test_pipelined_schedule(dev):
    """bench.py's schedule on the row kernel: whole-batch launches, three arena copies, runs in flight (set_pipelined(2)), three inputs rotating
    over nine runs; every output against the oracle."""
    case = sc._resnet(36, 120, 'rows', shift=6, opts=dict(whole_batch_launches=1, arena_copies=3, pipeline_depth=3))
    datas = [sc.make_data(f'pipelined{i}', case) for i in range(3)]
    g, outs, _ = sc.plan('pipelined', case, datas[0]['x'])
    _check_plan(case, g.net)
    (out,) = outs
    wants = [g.v[out][0]] + [(lambda gg: gg[0].v[gg[1][0]][0])(sc.build_graph(case, d['x'])) for d in datas[1:]]
    xt = [torch.from_numpy(d['raw']).to(dev) for d in datas]
    bufs = [torch.empty((case['N'], wants[0][0].size), dtype=torch.int32, device=dev) for _ in range(9)]
    g.net.set_pipelined(2)
    for r in range(9):
        g.net.run(xt[r % 3], out=bufs[r])
    torch.cuda.synchronize()
    g.net.set_pipelined(0)
    for r in range(9):
        np.testing.assert_array_equal(bufs[r].cpu().numpy().reshape(wants[0].shape), wants[r % 3], err_msg=f'run {r}')
    g.net.check()
    _check_plan(case, g.net)


def _row_tile_of(d, ntiles):
    """stem_rows_kernel's tile_of, by hand: dispatch slot d -> band tile."""
    xcd, qq, rr = d & 7, ntiles >> 3, ntiles & 7
    return (xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq) + (d >> 3)


RANGE_CASES = {'rows': dict(H=60, W=24, kernel='rows', opts={}),                  # pooled 15 x 6: bands of 7 / 7 / 1
               'tile': dict(H=84, W=32, kernel='tile', opts={'stem_rows': 0})}    # pooled 21 x 8: three tiles per image


@pytest.mark.parametrize('form', sorted(RANGE_CASES))
def test_int32_range_check(form, dev):
    """The int32 entry narrows its input to the head's 8-bit format and reports values outside it through the sticky error word of f8_net_check
    (no device fault).  2 images x 3 bands: the format's own ends pass; one value chk_hi + 1 in the first band of image 0 raises, and so does one
    in the last band of the last image; a clean run on a fresh handle is exact again."""
    r = RANGE_CASES[form]
    case = sc._resnet(r['H'], r['W'], r['kernel'], N=2, opts=r['opts'], shift=6)
    data = sc.make_data(f'range_{form}', case)
    assert data['x'].min() == 0 and data['x'].max() == 255               # chk_lo and chk_hi themselves are there
    g, wants = _run_case(f'range_{form}', case, dev)                      # ... and pass net.check()
    for where in ((0, 1, 2, 3), (1, 2, r['H'] - 1, r['W'] - 2)):
        bad = data['raw'].copy()
        bad[where] = 256
        g.net.run(torch.from_numpy(bad).to(dev))
        with pytest.raises(_lib.F8Error, match='8-bit format'):
            g.net.check()
        g.net.check()                                                     # the word is cleared by the report
    low = data['raw'].copy()
    low[1, 0, r['H'] // 2, 5] = -1
    g.net.run(torch.from_numpy(low).to(dev))
    with pytest.raises(_lib.F8Error, match='8-bit format'):
        g.net.check()
    _run_case(f'range_{form}', case, dev)                                 # a fresh handle, clean input


def test_int32_range_check_in_a_band_the_loader_waves_fetch(dev):
    """With 6 band tiles every band is some workgroup's first, which all waves load.  Four images under stem_grid_div = 32 are 12 band tiles on
    eight workgroups (256 compute units): dispatch slot 8 is fetched by the loader waves of workgroup 0 while its first band is multiplied."""
    case = sc._resnet(60, 24, 'rows', N=4, opts=sc.ONE_LAUNCH, shift=6)
    ntiles = 4 * 3
    grid = min(ntiles, (_cus(dev) // 32 + 7) // 8 * 8)
    assert grid < ntiles, f'{ntiles} band tiles on {grid} workgroups: the loader waves fetch nothing on this device'
    t = _row_tile_of(grid, ntiles)
    n, band = divmod(t, 3)
    data = sc.make_data('range_loader', case)
    g, wants = _run_case('range_loader', case, dev, one_launch=True)
    bad = data['raw'].copy()
    bad[n, 1, min(28 * band + 9, 59), 7] = 256                           # a row only this band reads (bands read input rows 28 b - 5 .. 28 b + 29)
    g.net.run(torch.from_numpy(bad).to(dev))
    with pytest.raises(_lib.F8Error, match='8-bit format'):
        g.net.check()
    _compare(sc.run_entry(g.net, case, data, dev), wants, 4, 'clean input after the report')
    g.net.check()
