"""Flip test-time augmentation inside the window kernels (infer.hip: segx_window_gather_views, segx_window_merge_views; SF.ViewTable, views= of SF.window_gather /
SF.window_merge) against the composition it replaces -- torch.flip, the existing ops per view, the adds in view order, one division, harden_segmap -- bit for bit;
on the fiber emulator (CPU) and on the GPU (-m gpu).  Images hold distinct integers, so one wrong index shows."""
import itertools

import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer2d, infer3d
from test_kernels_infer import rnd
from test_sliding_fused import eager_geometry, padded_canvas

ALL2 = ((), (1,), (0,), (0, 1))
ALL3 = tuple(v for n in range(4) for v in itertools.combinations(range(3), n))           # the 8 subsets of the three axes
T = 0.5


def _same(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what + ': NaN positions differ'
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), what + ': values differ'


def _counting(*shape):
    """1, 2, 3, ... in memory order: every cell its own integer (exact in float32 at these sizes), none of them the 0 of the padding"""
    n = 1
    for s in shape:
        n *= s
    assert n < 2 ** 24
    return torch.arange(1, n + 1, dtype=torch.float32).view(*shape)


def _flip(x, view, first=2):
    dims = tuple(first + a for a in view)
    return torch.flip(x, dims) if dims else x


# image, window, stride, B, C
GATHER = [((5, 7), (8, 8), (4, 4), 2, 3),            # smaller than the window on both axes, total pads 3 and 1: left 1 / right 2 and left 0 / right 1
          ((13, 10), (8, 8), (5, 8), 2, 3),          # the last column origin clamped (8 -> 2): asymmetric overlap
          ((9, 6, 7), (8, 8, 4), (4, 4, 3), 2, 4)]   # 3-D: padded on the middle axis only, two windows along the first and the last
PATCH = {2: (6, 10), 3: (6, 6, 4)}
GIDS = lambda g: 'img%s-win%s' % ('x'.join(map(str, g[0])), 'x'.join(map(str, g[1])))


@pytest.mark.parametrize('resample', [False, True], ids=['crop', 'patch'])
@pytest.mark.parametrize('geo', GATHER, ids=GIDS)
def test_gather_views_is_flip_pad_crop_bit_for_bit(backend, geo, resample):
    image, window, stride, B, C = geo
    nd = len(image)
    views = ALL2 if nd == 2 else ALL3
    patch = PATCH[nd] if resample else None
    x = _counting(B, C, *image)
    lp, ext, origins = eager_geometry(image, window, stride)
    if image == (5, 7):
        assert lp == (1, 0) and ext == (8, 8)
    if image == (13, 10):
        assert origins == [(0, 0), (0, 2), (5, 0), (5, 2)]
    table, vt = SF.WindowTable(origins, x.device), SF.ViewTable(views, nd, x.device)
    got = SF.window_gather(x, table, window, patch, lp, ext, views=vt)
    nwin = len(origins)
    assert tuple(got.shape) == (len(views) * nwin * B, C) + tuple(patch or window)
    for v, view in enumerate(views):
        canvas = padded_canvas(_flip(x, view), lp, ext)                  # the UN-PADDED image is flipped, then padded with the un-flipped geometry's pads
        for k, o in enumerate(origins):
            crop = canvas[(slice(None), slice(None)) + tuple(slice(a, a + w) for a, w in zip(o, window))].contiguous()
            want = SF.interp_linear(crop, patch) if resample else crop
            r = (v * nwin + k) * B
            assert torch.equal(got[r:r + B], want), 'view %r window %d at %r' % (view, k, o)
    assert torch.equal(SF.window_gather(x, table, window, patch, lp, ext, views=views), got)       # a plain sequence builds the same table


def _plant(scores):
    """values at the threshold and around it, both zeros and one NaN among the random scores: sigmoid(+-0) is T exactly, the neighbours of 0 land next to T"""
    flat = scores.view(-1)
    step = max(1, flat.numel() // 11)
    for i, val in enumerate([0.0, -0.0, -1e-6, 1e-6, float('nan'), 0.0, -0.0, -1e-6]):
        flat[3 + i * step] = val
    return scores


def _composed(scores, views, origins, window, image, lp, ext, mode, B):
    """the referee: per view, window_accum per window on zeroed canvases in that view's (flipped) frame, harden_segmap's soft map cropped to the image, flipped back;
    the adds in view order; one division; harden_segmap"""
    nwin, C = len(origins), scores.shape[1]
    crop = (slice(None), slice(None)) + tuple(slice(l, l + n) for l, n in zip(lp, image))
    total = None
    for v, view in enumerate(views):
        acc = torch.zeros(B, C, *ext); cnt = torch.zeros(B, *ext)
        for k, o in enumerate(origins):
            r = (v * nwin + k) * B
            SF.window_accum(scores[r:r + B], acc, cnt, tuple(o) + tuple(window))
        soft_v = _flip(SF.harden_segmap(acc, cnt, mode=mode)[0][crop], view)
        total = soft_v if total is None else total + soft_v
    mean = total / total.new_full((), float(len(views)))                # a tensor divisor: a division, not a product with the reciprocal
    return SF.harden_segmap(mean.contiguous(), mode=mode)


def _merge_case(image, window, origins, lp, ext, views, C, mode=0, sshape=None, seed=71, B=2):
    nd = len(image)
    scores = _plant(rnd(len(views) * len(origins) * B, C, *(sshape or window), seed=seed, scale=2.0))
    table, vt = SF.WindowTable(origins, scores.device), SF.ViewTable(views, nd, scores.device)
    soft, hard = SF.window_merge(scores, table, window, image, lp, ext, mode=mode, views=vt)
    ref_soft, ref_hard = _composed(scores, views, origins, window, image, lp, ext, mode, B)
    assert tuple(soft.shape) == (B, C) + tuple(image) and soft.is_contiguous() and hard.is_contiguous()
    _same(soft, ref_soft, 'soft')
    assert torch.equal(hard, ref_hard)
    return scores, soft, hard


@pytest.mark.parametrize('C', [2, 3, 4, 5, 10])
def test_merge_views_is_the_composition_bit_for_bit(backend, C):
    """the class forms: 2, 3, 4 exact, 5 in the 8-entry form, 10 in the 16-entry form; four views, four overlapping windows"""
    image, window, stride = (13, 10), (8, 8), (5, 8)
    lp, ext, origins = eager_geometry(image, window, stride)
    _, soft, _ = _merge_case(image, window, origins, lp, ext, ALL2, C)
    assert torch.isnan(soft).any() and not torch.isnan(soft).all()       # the planted NaN reaches the map and stays where it belongs


def test_merge_views_resampled_scores(backend):
    """scores smaller than the window: the interpolating branch of window_prob at the mirrored coordinate"""
    image, window, stride = (13, 10), (8, 8), (5, 8)
    lp, ext, origins = eager_geometry(image, window, stride)
    _merge_case(image, window, origins, lp, ext, ALL2, 3, sshape=(4, 6), seed=72)


def test_merge_views_padded_image(backend):
    image, window = (5, 7), (8, 8)
    lp, ext, origins = eager_geometry(image, window, (4, 4))
    _merge_case(image, window, origins, lp, ext, ALL2, 3, seed=73)


def test_merge_views_3d_brats_rule(backend):
    image, window, stride = (9, 6, 7), (8, 8, 4), (4, 4, 3)
    lp, ext, origins = eager_geometry(image, window, stride)
    views = ((), (0,), (2,), (0, 1, 2))
    scores, soft, hard = _merge_case(image, window, origins, lp, ext, views, 4, mode=1, seed=74, B=1)
    table = SF.WindowTable(origins, scores.device)
    soft0, hard0 = SF.window_merge(scores, table, window, image, lp, ext, mode=0, views=views)
    assert not torch.equal(hard, hard0) and not torch.equal(torch.nan_to_num(soft), torch.nan_to_num(soft0))      # the consistency rule changes this result
    _merge_case(image, window, origins, lp, ext, ALL3, 4, mode=1, seed=75, B=2)                                     # all eight views


def test_merge_one_view_that_is_not_the_identity(backend):
    """V = 1: the map of the flipped image flipped back, divided by 1.  One window over a padded image: a cell's soft value is the sigmoid of one score, so the planted
    zeros sit exactly at the threshold and harden to 1, their neighbours below it to 0."""
    image, window = (5, 7), (8, 8)
    lp, ext, origins = eager_geometry(image, window, (4, 4))
    assert len(origins) == 1
    scores = rnd(2, 3, 8, 8, seed=76, scale=2.0)
    scores[0, 1, 2, 1], scores[0, 1, 2, 2], scores[0, 1, 2, 3], scores[0, 2, 3, 3] = 0.0, -0.0, -1e-6, float('nan')       # window rows 1..5, columns 0..6 are the image
    table = SF.WindowTable(origins, scores.device)
    soft, hard = SF.window_merge(scores, table, window, image, lp, ext, views=((1,),))
    ref_soft, ref_hard = _composed(scores, ((1,),), origins, window, image, lp, ext, 0, 2)
    _same(soft, ref_soft, 'soft')
    assert torch.equal(hard, ref_hard)
    row = soft[0, 1, 1]                                                  # window row 2 = image row 1; window column x = image column x, mirrored to 6 - x
    assert row[5].item() == T and row[4].item() == T and hard[0, 1, 1, 5].item() == 1.0 and hard[0, 1, 1, 4].item() == 1.0
    assert row[3].item() < T and hard[0, 1, 1, 3].item() == 0.0
    assert torch.isnan(soft[0, 2, 2, 3]) and hard[0, 2, 2, 3].item() == 0.0


def test_merge_three_views_in_an_unsorted_order(backend):
    """the adds run in the order given: (a + b) + c.  Another order of the same views gives other bits somewhere on this input, so the comparison can tell."""
    image, window, stride = (13, 10), (8, 8), (5, 8)
    lp, ext, origins = eager_geometry(image, window, stride)
    views = ((0, 1), (), (1,))
    scores, soft, _ = _merge_case(image, window, origins, lp, ext, views, 3, seed=77)
    nwin, B = len(origins), 2
    order = (1, 2, 0)
    shuffled = torch.cat([scores[v * nwin * B:(v + 1) * nwin * B] for v in order])
    other, _ = SF.window_merge(shuffled, SF.WindowTable(origins, scores.device), window, image, lp, ext, views=tuple(views[v] for v in order))
    close = (torch.nan_to_num(other) - torch.nan_to_num(soft)).abs().max().item()
    assert 0.0 < close < 1e-6                                           # the same mean up to the rounding of another order of additions


def test_merge_views_leaves_an_uncovered_cell_nan(backend):
    """a hand-built table: one 8 x 8 window over an 8 x 12 image.  Columns 8..11 have no window; in the mirrored view columns 0..3 have none.  number + NaN = NaN, as
    the composition gives."""
    image, window = (8, 12), (8, 8)
    scores, soft, hard = _merge_case(image, window, [(0, 0)], (0, 0), (8, 12), ((), (1,)), 3, seed=78)
    nan = torch.isnan(soft)
    assert nan[:, :, :, :4].all() and nan[:, :, :, 8:].all()
    assert (~nan[:, :, :, 4:8]).sum().item() >= nan[:, :, :, 4:8].numel() - 8          # all but the cells the planted NaN reaches


@pytest.mark.parametrize('geo', GATHER, ids=GIDS)
def test_the_identity_view_is_the_existing_kernels(backend, geo):
    image, window, stride, B, C = geo
    nd = len(image)
    lp, ext, origins = eager_geometry(image, window, stride)
    x = _counting(B, C, *image)
    table = SF.WindowTable(origins, x.device)
    assert torch.equal(SF.window_gather(x, table, window, None, lp, ext, views=((),)), SF.window_gather(x, table, window, None, lp, ext))
    mode = 1 if C == 4 else 0
    scores = _plant(rnd(len(origins) * B, C, *window, seed=79, scale=2.0))
    soft, hard = SF.window_merge(scores, table, window, image, lp, ext, mode=mode, views=((),))
    soft0, hard0 = SF.window_merge(scores, table, window, image, lp, ext, mode=mode)
    _same(soft, soft0, 'soft')
    assert torch.equal(hard, hard0)


@pytest.mark.parametrize('bad', [(), ((), ()), ((0, 1), (1, 0)), ((2,),), ((-1,),), ((0, 0),), tuple(((), (0,), (1,), (0, 1)) * 3)[:9], 5],
                         ids=['empty', 'twice', 'same-set', 'axis-2', 'axis-neg', 'axis-twice', 'nine', 'no-sequence'])
def test_bad_views_raise_value_error_before_anything_runs(backend, bad):
    with pytest.raises(ValueError):
        SF.ViewTable(bad, 2, torch.device('cpu'))
    x = _counting(1, 3, 8, 8)
    with pytest.raises(ValueError):
        SF.window_gather(x, SF.WindowTable([(0, 0)], x.device), (8, 8), views=bad)
    for fused in (False, True):                                          # net = None: the refusal comes before the net is touched
        with pytest.raises(ValueError):
            infer2d.test_single_batch(None, x, (8, 8), (8, 8), (4, 4), 'fundus', 3, fused=fused, tta=bad)
    with pytest.raises(ValueError):
        infer2d.test_all_cases(None, [(x, x)], 'fundus', 3, (8, 8), (8, 8), (4, 4), tta=bad)


def test_bad_views_3d(backend):
    vol = _counting(2, 8, 8, 8)
    for bad in ((), ((3,),), ((0,), (0,)), ALL3 + ((0,),)):
        for fused in (False, True):
            with pytest.raises(ValueError):
                infer3d.test_single_case(None, vol, (8, 8, 8), (8, 8, 8), 1, 4, 4, 'brats', fused=fused, tta=bad)
        with pytest.raises(ValueError):
            infer3d.test_all_cases(None, [], tta=bad)
    assert SF.ViewTable(ALL3, 3, vol.device).masks == (0, 1, 2, 4, 3, 5, 6, 7)          # axis 0 (H of [C, H, W, D]) is the kernels' depth axis: bit 0
    assert SF.ViewTable(ALL2, 2, vol.device).masks == (0, 4, 2, 6)                      # 2-D: H is bit 1, W is bit 2; bit 0 belongs to the absent depth axis


def test_library_refuses_bad_view_tables(backend):
    import ctypes
    L = backend.L
    x = _counting(1, 3, 8, 8); t = SF.WindowTable([(0, 0)], x.device)
    geom = (1, 8, 8, 0, 0, 0, 1, 8, 8, 1, 8, 8)
    mgeom = (1, 8, 8, 1, 8, 8, 1, 8, 8, 0, 0, 0, 1, 8, 8)
    soft, hard = torch.empty(1, 3, 8, 8), torch.empty(1, 3, 8, 8)

    def table(masks):
        return torch.tensor(masks, dtype=torch.int32), (ctypes.c_int32 * len(masks))(*masks)
    dev, host = table([0, 4])
    out = torch.empty(2, 3, 8, 8)
    L.window_gather_views(x, t.dev, t.host, dev, host, out, 1, 2, 1, 3, geom)
    assert torch.equal(out[0], x[0]) and torch.equal(out[1], x[0].flip(2))
    L.window_merge_views(out, t.dev, t.host, dev, host, soft, hard, 1, 2, 1, 3, mgeom, 0)
    nine = table([0, 2, 4, 6, 0, 2, 4, 6, 0])
    for V in (0, 9):
        with pytest.raises(RuntimeError, match='distinct views'):
            L.window_gather_views(x, t.dev, t.host, nine[0], nine[1], torch.empty(9, 3, 8, 8), 1, V, 1, 3, geom)
        with pytest.raises(RuntimeError, match='distinct views'):
            L.window_merge_views(torch.empty(9, 3, 8, 8), t.dev, t.host, nine[0], nine[1], soft, hard, 1, V, 1, 3, mgeom, 0)
    for masks in ([2, 2], [0, 1], [8], [-1]):                            # twice the same; the depth bit of a 2-D call; bits outside the three
        dev, host = table(masks)
        with pytest.raises(RuntimeError, match='distinct views'):
            L.window_gather_views(x, t.dev, t.host, dev, host, out, 1, len(masks), 1, 3, geom)
        with pytest.raises(RuntimeError, match='distinct views'):
            L.window_merge_views(out, t.dev, t.host, dev, host, soft, hard, 1, len(masks), 1, 3, mgeom, 0)
    dev, host = table([0, 4])
    outside = SF.WindowTable([(1, 0)], x.device)                         # 1 + 8 > 8
    with pytest.raises(RuntimeError, match='outside the padded canvas'):
        L.window_gather_views(x, outside.dev, outside.host, dev, host, out, 1, 2, 1, 3, geom)
    with pytest.raises(RuntimeError, match='outside the padded canvas'):
        L.window_merge_views(out, outside.dev, outside.host, dev, host, soft, hard, 1, 2, 1, 3, mgeom, 0)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.window_gather_views(x, t.dev, t.host, dev, None, out, 1, 2, 1, 3, geom)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.window_merge_views(out, t.dev, t.host, dev, None, soft, hard, 1, 2, 1, 3, mgeom, 0)


@pytest.mark.gpu
def test_merge_views_beyond_one_sweep_of_the_grid():
    """4100 x 4100 cells = 16.81 M, above the 65 536 x 256 = 16.78 M threads of the capped grid: the grid-stride loop takes a second trip.  One window the size of the
    image, two views, against the composition on the device."""
    dev = torch.device('cuda', 0)
    N, C = 4100, 2
    g = torch.Generator(device='cpu').manual_seed(80)
    scores = (torch.randn(2, C, 64, N, generator=g) * 2.0).repeat_interleave(65, dim=2)[:, :, :N].contiguous().to(dev)      # rows repeat: the columns carry the test
    assert tuple(scores.shape) == (2, C, N, N) and N * N > 65536 * 256
    views = ((), (0, 1))
    table = SF.WindowTable([(0, 0)], dev)
    soft, hard = SF.window_merge(scores, table, (N, N), (N, N), views=SF.ViewTable(views, 2, dev))
    total = None
    for v, view in enumerate(views):
        acc = torch.zeros(1, C, N, N, device=dev); cnt = torch.zeros(1, N, N, device=dev)
        SF.window_accum(scores[v:v + 1], acc, cnt, (0, 0, N, N))
        soft_v = _flip(SF.harden_segmap(acc, cnt)[0], view)
        total = soft_v if total is None else total + soft_v
    ref_soft, ref_hard = SF.harden_segmap((total / total.new_full((), 2.0)).contiguous())
    assert torch.equal(soft, ref_soft) and torch.equal(hard, ref_hard)
    x = torch.arange(N * N, dtype=torch.float32, device=dev).view(1, 1, N, N)                    # exact up to 2^24 = 16 777 216 < N * N: compare through the flip itself
    got = SF.window_gather(x, table, (N, N), views=views)
    assert torch.equal(got[0], x[0]) and torch.equal(got[1], x[0].flip(1, 2))
