"""The sliding-window evaluation as gather -> network on stacked windows -> merge (infer.hip: segx_window_gather, segx_window_merge; infer2d.py) against the
eager sequence it replaces (crop + interp_linear per window, window_accum per window, harden_segmap), bit for bit; on the fiber emulator (CPU) and on the
GPU (-m gpu)."""
import math

import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer2d
from test_kernels_infer import rnd, close


def eager_geometry(image, window, stride):
    """transcription of the loops of test_util2d.test_single_batch (2-D, :25-41) and test_util3d.test_single_case (3-D): left pads, padded extent and
    the window origins in the order the loops visit them (outermost axis first, the last origin of an axis clamped to extent - window)"""
    pads = [max(w - n, 0) for n, w in zip(image, window)]
    lp = [p // 2 for p in pads]
    ext = [n + p for n, p in zip(image, pads)]
    counts = [math.ceil((e - w) / s) + 1 for e, w, s in zip(ext, window, stride)]
    origins = [()]
    for ax in range(len(image)):
        origins = [o + (min(stride[ax] * i, ext[ax] - window[ax]),) for o in origins for i in range(counts[ax])]
    return tuple(lp), tuple(ext), origins


def padded_canvas(x, lp, ext):
    out = x.new_zeros(tuple(x.shape[:2]) + tuple(ext))
    out[(slice(None), slice(None)) + tuple(slice(l, l + n) for l, n in zip(lp, x.shape[2:]))] = x
    return out


# image, window, stride, patch (None = the window size)
G_2D = [((11, 13), (8, 8), (4, 5), None),            # clamped last row and column
        ((8, 8), (8, 8), (4, 4), None),              # one window
        ((6, 7), (8, 8), (4, 4), None),              # padding on both axes: zeros read outside the image
        ((11, 13), (8, 8), (4, 5), (6, 6)),          # resampled down
        ((11, 13), (8, 8), (4, 5), (12, 10)),        # resampled up
        ((9, 9), (8, 8), (8, 8), None),              # origins 0 and 1 after the clamp: the two windows coincide but for one row / column
        ((14, 19), (8, 8), (3, 4), None)]            # 3 x 4 = 12 windows: cells with four covering windows
G_3D = [((6, 9, 10), (4, 8, 8), (2, 4, 4), None),
        ((6, 9, 10), (4, 8, 8), (2, 4, 4), (4, 6, 6))]
IDS = lambda g: 'img%s-win%s-str%s-patch%s' % tuple('x'.join(map(str, v)) if v else 'same' for v in g)


@pytest.mark.parametrize('geo', G_2D + G_3D, ids=IDS)
def test_window_gather_is_the_crop_and_interp_linear_bit_for_bit(backend, geo):
    image, window, stride, patch = geo
    B, C = 2, 3
    x = rnd(B, C, *image, seed=61)
    lp, ext, origins = eager_geometry(image, window, stride)
    table = SF.WindowTable(origins, x.device)
    got = SF.window_gather(x, table, window, patch, lp, ext)
    assert tuple(got.shape) == (len(origins) * B, C) + tuple(patch or window)
    canvas = padded_canvas(x, lp, ext)
    for k, o in enumerate(origins):
        crop = canvas[(slice(None), slice(None)) + tuple(slice(a, a + w) for a, w in zip(o, window))].contiguous()
        want = SF.interp_linear(crop, patch) if patch is not None and tuple(patch) != tuple(window) else crop
        assert torch.equal(got[k * B:(k + 1) * B], want), 'window %d at %r' % (k, o)


def _merge_case(geo, C, mode, seed=62):
    image, window, stride, patch = geo
    B = 2
    lp, ext, origins = eager_geometry(image, window, stride)
    scores = rnd(len(origins) * B, C, *(patch or window), seed=seed, scale=2.0)
    table = SF.WindowTable(origins, scores.device)
    soft, hard = SF.window_merge(scores, table, window, image, lp, ext, mode=mode)
    acc = torch.zeros(B, C, *ext); cnt = torch.zeros(B, *ext)
    for k, o in enumerate(origins):
        SF.window_accum(scores[k * B:(k + 1) * B], acc, cnt, tuple(o) + tuple(window))
    ref_soft, ref_hard = SF.harden_segmap(acc, cnt, mode=mode)
    sl = (slice(None), slice(None)) + tuple(slice(l, l + n) for l, n in zip(lp, image))
    return soft, hard, ref_soft[sl], ref_hard[sl], cnt[(slice(None),) + sl[2:]]


@pytest.mark.parametrize('geo', G_2D + G_3D, ids=IDS)
def test_window_merge_is_accumulate_then_harden_bit_for_bit(backend, geo):
    soft, hard, ref_soft, ref_hard, cnt = _merge_case(geo, 3, 0)
    assert tuple(soft.shape) == tuple(ref_soft.shape) and soft.is_contiguous() and hard.is_contiguous()
    assert torch.equal(soft, ref_soft) and torch.equal(hard, ref_hard)
    if geo[0] == (14, 19):
        assert cnt.max().item() >= 4.0                 # the case is there for its cells with four and more covering windows
    if geo[0] == (9, 9):
        assert cnt.min().item() == 1.0 and cnt.max().item() == 4.0


@pytest.mark.parametrize('geo', G_3D, ids=IDS)
def test_window_merge_brats_rule(backend, geo):
    soft, hard, ref_soft, ref_hard, _ = _merge_case(geo, 4, 1, seed=63)
    assert torch.equal(soft, ref_soft) and torch.equal(hard, ref_hard)
    assert not torch.equal(ref_hard, _merge_case(geo, 4, 0, seed=63)[3])        # the rule changes labels on this input: mode 1 is not mode 0


def test_refusals(backend):
    x = rnd(2, 3, 11, 13, seed=64)
    inside = SF.WindowTable([(0, 0), (3, 5)], x.device)
    outside = SF.WindowTable([(0, 0), (4, 5)], x.device)              # 4 + 8 > 11
    SF.window_gather(x, inside, (8, 8))
    with pytest.raises(RuntimeError, match='outside the padded canvas'):
        SF.window_gather(x, outside, (8, 8))
    s = rnd(4, 3, 8, 8, seed=65)
    SF.window_merge(s, inside, (8, 8), (11, 13))
    with pytest.raises(RuntimeError, match='outside the padded canvas'):
        SF.window_merge(s, outside, (8, 8), (11, 13))
    with pytest.raises(RuntimeError, match='mode'):
        SF.window_merge(s, inside, (8, 8), (11, 13), mode=1)           # BraTS rule with C = 3
    with pytest.raises(RuntimeError, match='outside the padded canvas'):
        SF.window_gather(x, SF.WindowTable([(-1, 0)], x.device), (8, 8))
    with pytest.raises(ValueError):
        SF.WindowTable([], x.device)                                   # nwin = 0 never reaches the library
    with pytest.raises(ValueError):
        infer2d.sliding_windows(11, 13, (8, 8), (9, 4))                # stride above the window: cells no window covers
    with pytest.raises(ValueError):
        infer2d.sliding_windows(11, 13, (8, 8), (4, 9))
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.window_gather(x.clone().requires_grad_(True), inside, (8, 8))
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.window_merge(s.clone().requires_grad_(True), inside, (8, 8), (11, 13))
    with torch.no_grad():                                              # no gradient can flow: accepted
        SF.window_gather(x.clone().requires_grad_(True), inside, (8, 8))


def test_library_refuses_null_pointers_and_no_windows(backend):
    L = backend.L
    x = rnd(1, 3, 8, 8, seed=66); out = torch.empty(1, 3, 8, 8); t = SF.WindowTable([(0, 0)], x.device)
    geom = (1, 8, 8, 0, 0, 0, 1, 8, 8, 1, 8, 8)
    mgeom = (1, 8, 8, 1, 8, 8, 1, 8, 8, 0, 0, 0, 1, 8, 8)
    L.window_gather(x, t.dev, t.host, out, 1, 1, 3, geom)
    assert torch.equal(out, x)
    with pytest.raises(RuntimeError, match='nwin'):
        L.window_gather(x, t.dev, t.host, out, 0, 1, 3, geom)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.window_gather(x, t.dev, None, out, 1, 1, 3, geom)
    with pytest.raises(RuntimeError, match='nwin'):
        L.window_merge(x, t.dev, t.host, out, torch.empty_like(out), 0, 1, 3, mgeom, 0)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.window_merge(x, t.dev, None, out, torch.empty_like(out), 1, 1, 3, mgeom, 0)


@pytest.mark.parametrize('geo', G_2D, ids=IDS)
def test_sliding_windows_is_the_eager_loops_arithmetic(geo):
    image, window, stride, _ = geo
    lp, ext, origins = eager_geometry(image, window, stride)
    assert infer2d.sliding_windows(image[0], image[1], window, stride) == (lp, ext, origins)


def test_sliding_windows_product_shapes():
    pads, ext, origins = infer2d.sliding_windows(576, 576, (256, 256), (128, 128))
    assert pads == (0, 0) and ext == (576, 576) and len(origins) == 16 and origins[:5] == [(0, 0), (0, 128), (0, 256), (0, 320), (128, 0)]
    pads, ext, origins = infer2d.sliding_windows(200, 300, (256, 256), (128, 128))
    assert pads == (28, 0) and ext == (256, 300) and origins == [(0, 0), (0, 44)]


# ---- the whole path on a small model --------------------------------------------------------------------------------------------------------------
def small_net(device, seed=7):
    from segtran_amd import engine
    from test_fold_batchnorm import _randomize_bn
    net = engine.build_model(dict(engine.CONFIGS['cfg1'], size=(64, 64)), device, attractors=32)
    _randomize_bn(net.backbone, seed)
    return net.eval()


SMALL = dict(orig_input_size=(64, 64), patch_size=(64, 64), stride=(32, 32), task_name='fundus', num_classes=3)
NEAR = 1e-4                           # the bar of tests/test_fold_batchnorm.py for two summation orders of the same network


@pytest.mark.gpu
def test_fused_evaluation_of_a_small_model():
    """On the device only (the fiber emulator needs minutes for nine forwards of the whole network).  96 x 80 image, 64 x 64 windows at stride 32: 2 x 2 windows, the last column clamped (origin 16).  window_batch=1 runs the eager path's forwards, so the
    results are the eager ones bit for bit; all windows stacked changes the batch size of every GEMM, i.e. the summation order: soft within 1e-4 of scale,
    labels equal wherever the eager soft value is further than that from the threshold (a cap of 1 % of the cells may be that close)."""
    net = small_net(torch.device('cuda', 0))
    x = rnd(2, 3, 96, 80, seed=67).to('cuda:0')
    assert infer2d.sliding_windows(96, 80, (64, 64), (32, 32))[2] == [(0, 0), (0, 16), (32, 0), (32, 16)]
    hard0, soft0 = infer2d.test_single_batch(net, x, **SMALL)
    assert hard0.dtype == torch.int32 and tuple(hard0.shape) == tuple(soft0.shape) == (2, 3, 96, 80)
    hard1, soft1 = infer2d.test_single_batch(net, x, fused=True, window_batch=1, **SMALL)
    assert hard1.dtype == torch.int32 and torch.equal(hard1, hard0) and torch.equal(soft1, soft0)
    hard4, soft4 = infer2d.test_single_batch(net, x, fused=True, **SMALL)
    close(soft4, soft0, NEAR)
    decided = (soft0 - 0.5).abs() > NEAR * soft0.abs().max().item()
    decided[:, 0] = decided[:, 1:].all(1)              # the background label depends on every other class
    assert (~decided).float().mean().item() < 0.01, 'the eager soft map itself is within 1e-4 of the threshold at 1 % of the cells: pick another seed'
    assert torch.equal(hard4[decided], hard0[decided])
    hard2, soft2 = infer2d.test_single_batch(net, x, fused=True, window_batch=3, fold_bn=True, **SMALL)       # chunks of 3 + 1 windows, folded
    close(soft2, soft0, NEAR)
    assert not net.batchnorm_folded


@pytest.mark.gpu
def test_fused_test_all_cases_agrees_with_the_eager_one():
    """window_batch=1: the same forwards, so the same soft maps and the same Dice figures, with one fold for all the batches"""
    import numpy as np
    dev = torch.device('cuda', 0)
    net = small_net(dev)
    batches = [(rnd(2, 3, 96, 80, seed=68 + i).to(dev), (rnd(2, 3, 96, 80, seed=78 + i) > 0).float().to(dev)) for i in range(2)]
    args = ('fundus', 3, SMALL['orig_input_size'], SMALL['patch_size'], SMALL['stride'])
    want, n0 = infer2d.test_all_cases(net, batches, *args)
    got, n1 = infer2d.test_all_cases(net, batches, *args, fused=True, window_batch=1)
    assert n0 == n1 == 4 and np.array_equal(got, want)
    stacked, n2 = infer2d.test_all_cases(net, batches, *args, fold_bn=True, fused=True)
    assert n2 == 4 and stacked.shape == want.shape and np.isfinite(stacked).all() and not net.batchnorm_folded


def test_package_exports():
    import segtran_amd
    assert segtran_amd.GraphedSlidingWindow is infer2d.GraphedSlidingWindow
    assert segtran_amd.sliding_windows(96, 80, (64, 64), (32, 32)) == infer2d.sliding_windows(96, 80, (64, 64), (32, 32))
