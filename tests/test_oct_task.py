"""The OCT task (10 one-hot classes): index -> one-hot labels, hardening and window merge above 8 classes, the one-pass evaluation tail (metrics.hip:
segx_onehot_case_tail), onehot_inv_map, the loss weights with --focus and the trainer's flags -- on the fiber emulator (CPU) and on the GPU (-m gpu), against
tests/golden/oct2d.npz (the reference's own functions, tests/golden/make_oct_golden.py) and torch statements on the CPU.  0 / 1 maps, integers and single rounded
float operations: every comparison is for EQUALITY.

Sizes of the tail, with T = SEGX_CASE_TAIL_THREADS (a workgroup covers 4 T pixels per trip) and as tests/test_case_tail.py places them: 1 and 3 (one thread, a cut
quad), 4 T - 1 / 4 T / 4 T + 1, 8 T + 2, and 4 T MAX_BLOCKS + 4 T + 4 (and one less) where the first workgroups take a second trip (GPU only).  S % 4 != 0 puts the
planes off 16-byte alignment: those sizes take the dword path, the others the 16-byte one."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from segtran_amd import engine, functional as SF, infer2d, segx, train2d
from segtran_amd.dataloaders import datasets2d as D2
from segtran_amd.synth import synth_oct_mask
from util import golden

T, MAXB = segx.SegxLib.CASE_TAIL_THREADS, segx.SegxLib.CASE_TAIL_MAX_BLOCKS
SIZES = [1, 3, 4 * T - 1, 4 * T, 4 * T + 1, 8 * T + 2]
S_SECOND_TRIP = 4 * T * MAXB + 4 * T + 4
G = golden('oct2d')


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'segx.h')).read()
    assert int(re.search(r'#define SEGX_MAX_CLASSES (\d+)', hdr).group(1)) == segx.SegxLib.MAX_CLASSES == 16


# ---- index -> one-hot ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.uint8, torch.int32, torch.int64])
@pytest.mark.parametrize('S', [1, 255, 257])
@pytest.mark.parametrize('C', [10, 16])
def test_index_onehot_equals_the_reference(backend, C, S, dtype):
    ix, want = (G['ix4'][:, 0, 0], G['oh4'][:, :, 0]) if C == 10 else (G['ix16'][:, 0], G['oh16'][:, :, 0])
    got = SF.index_onehot(ix[:, :S].to(dtype).to(backend.dev), C)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, C, S)
    assert torch.equal(got.cpu(), want[:, :, :S].float())


def test_index_onehot_label_outside_the_classes_sets_none(backend):
    for dtype, vals in ((torch.uint8, [0, 9, 10, 255, 3]), (torch.int32, [0, 9, 10, 255, -1, 1 << 20, 3])):
        lab = torch.tensor([vals], dtype=dtype)
        got = SF.index_onehot(lab, 10).cpu()
        want = torch.stack([(lab.cpu()[0] == c) for c in range(10)]).float()[None]
        assert torch.equal(got, want)
        assert got[0, :, 2].sum() == 0 and got[0, :, 3].sum() == 0 and got[0, :, 0].sum() == 1


def test_index_to_onehot_takes_the_three_forms(backend):
    dev = backend.dev
    for mask, want in ((G['ix4'], G['oh4']), (G['ix4'][:, 0], G['oh3']), (G['ix2'], G['oh2'])):
        for m in (mask, mask.to(dev)):                                          # the torch expression (CPU tensors) and, on the GPU, the kernel
            assert torch.equal(D2.index_to_onehot(m, 10).cpu(), want.float())
    assert torch.equal(D2.index_to_onehot(G['ix4'][:, 0].to(dev), 10).cpu(), G['oh3'].float())
    assert torch.equal(SF.label_nhot(G['ix4'][:, 0].to(dev), 'oct').cpu(), G['oh4'].float())
    assert torch.equal(SF.label_nhot(G['ix16'].to(dev), 'oct', num_classes=16).cpu(), G['oh16'].float())
    assert torch.equal(engine.map_mask('oct', G['ix4'][:, 0].to(dev)).cpu(), G['oh4'].float())
    with pytest.raises(ValueError, match='index mask'):
        D2.index_to_onehot(torch.zeros(2, 3, 4, 5, dtype=torch.uint8), 10)


def test_index_onehot_refusals(backend):
    lab = torch.zeros(2, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match='classes'):
        SF.index_onehot(lab, 17)
    with pytest.raises(ValueError, match='classes'):
        SF.index_onehot(lab, 0)
    with pytest.raises(TypeError, match='integer'):
        SF.index_onehot(lab.float(), 10)
    out = torch.zeros(2, 10, 8)
    with pytest.raises(RuntimeError, match='is not in 1'):
        backend.L.index_onehot(lab, 1, out, 2, 17, 8)
    with pytest.raises(RuntimeError, match='uint8 \\(1\\) or int32 \\(4\\)'):
        backend.L.index_onehot(lab, 2, out, 2, 10, 8)


# ---- hardening and window merge above 8 classes ------------------------------------------------------------------------------------------------------------------
def torch_harden(soft, thres=0.5):
    hard = (soft >= thres).float()
    hard[:, 0] = (hard[:, 1:].sum(dim=1) == 0).float()
    return hard


@pytest.mark.parametrize('C', [9, 10, 16])
def test_harden_above_eight_classes(backend, C):
    soft = G['soft%d' % C]
    got_soft, got = SF.harden_segmap(soft.to(backend.dev), mode=0)
    assert torch.equal(got.cpu(), G['hard%d' % C].float()) and torch.equal(got.cpu(), torch_harden(soft)) and torch.equal(got_soft.cpu(), soft)
    assert torch.equal(D2.harden_segmap2d(soft[1].to(backend.dev)).cpu(), G['hard%d_3d' % C].int())
    acc, cnt = (soft * 3).to(backend.dev), torch.full((2, 5, 7), 3.0)          # the mean over a count: 3 x / 3 is x for multiples of 1/8
    assert torch.equal(SF.harden_segmap(acc, cnt, mode=0)[1].cpu(), G['hard%d' % C].float())


def test_harden_refuses_seventeen_classes(backend):
    with pytest.raises(RuntimeError, match='segx_harden_segmap'):
        SF.harden_segmap(torch.rand(1, 17, 4, 4), mode=0)
    with pytest.raises(RuntimeError, match='segx_harden_segmap'):
        SF.harden_segmap(torch.rand(1, 1, 4, 4), mode=0)


@pytest.mark.parametrize('C', [10, 16, 3])
def test_window_merge_equals_the_accumulate_loop(backend, C):
    """two overlapping 16 x 24 windows over a 16 x 36 image, from 8 x 12 scores (resampled x 2): the merge kernel is the accumulate loop followed by harden, bit for bit"""
    B, window, image, origins = 2, (16, 24), (16, 36), [(0, 0), (0, 12)]
    g = torch.Generator(device='cpu').manual_seed(70 + C)
    scores = (torch.randn(len(origins) * B, C, 8, 12, generator=g, device='cpu') * 2).to(backend.dev)
    acc, cnt = torch.zeros(B, C, *image), torch.zeros(B, *image)
    for k, (y0, x0) in enumerate(origins):
        SF.window_accum(scores[k * B:(k + 1) * B], acc, cnt, (y0, x0) + window)
    want_soft, want_hard = SF.harden_segmap(acc, cnt, mode=0)
    soft, hard = SF.window_merge(scores, SF.WindowTable(origins, backend.dev), window, image, mode=0)
    assert torch.equal(soft, want_soft) and torch.equal(hard, want_hard)
    assert torch.equal(hard.cpu(), torch_harden(soft.cpu())) and 0 < hard[:, 1:].mean() < 1
    assert (cnt == 2).any() and (cnt == 1).any()


def test_window_merge_refuses_seventeen_classes(backend):
    scores = torch.zeros(1, 17, 8, 12)
    with pytest.raises(RuntimeError, match='2 <= C <= 16'):
        SF.window_merge(scores, SF.WindowTable([(0, 0)], backend.dev), (16, 24), (16, 24), mode=0)


# ---- the one-pass tail -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case(S, C=10, B=2):
    """CPU tensors: soft [B, C, S] in multiples of 1/8 (values exactly at T = 0.5 are frequent; several classes on, or none, per pixel), gt uint8 [B, S] with labels
    up to C + 1 (two of them outside the classes), and a colour table"""
    g = torch.Generator(device='cpu').manual_seed(2000 + S + 100 * C)
    soft = torch.round(torch.rand(B, C, S, generator=g, device='cpu') ** 2 * 8) / 8
    gt = torch.randint(0, C + 2, (B, S), generator=g, device='cpu').to(torch.uint8)
    cmap = torch.randint(0, 256, (C, 3), generator=g, device='cpu').to(torch.uint8)
    return soft, gt, cmap


def composed(soft, gt, cmap, thres=0.5):
    """harden -> the operands of dice_scores -> onehot_inv_map, through the library's existing calls and torch sums; (counts, labels, rgb) on the CPU"""
    C = soft.shape[1]
    hard = SF.harden_segmap(soft, mode=0, T=thres)[1]
    nh = SF.index_onehot(gt, C)
    h, n = hard[:, 1:].cpu() != 0, nh[:, 1:].cpu() != 0
    counts = torch.stack([(h & n).sum(-1), h.sum(-1), n.sum(-1)], dim=-1).to(torch.int32)
    labels = D2.onehot_inv_map(hard.unsqueeze(-2))[:, 0, :, 0].to(torch.uint8)
    rgb = D2.onehot_inv_map(hard.unsqueeze(-2), cmap.to(soft.device))[:, 0]
    return counts, labels.cpu(), rgb.cpu()


def check(b, S, C=10, B=2):
    soft, gt, cmap = (t.to(b.dev) for t in case(S, C, B))
    counts, labels, rgb = SF.onehot_case_tail(soft, gt, cmap)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (B, C - 1, 3)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, S) and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (B, S, 3)
    want = composed(soft, gt, cmap)
    assert torch.equal(counts.cpu(), want[0]) and torch.equal(labels.cpu(), want[1]) and torch.equal(rgb.cpu(), want[2])
    return want


@pytest.mark.parametrize('S', SIZES)
def test_tail_equals_the_composed_path(backend, S):
    check(backend, S)


@pytest.mark.parametrize('C', [2, 3, 8, 9, 16])
def test_tail_at_other_class_counts(backend, C):
    """both register forms (C <= 8 and above) and their edges, on the dword and on the 16-byte path"""
    check(backend, 4 * T + 1, C)
    check(backend, 8, C, B=3)


def test_the_tail_inputs_hold_ties_empty_pixels_and_every_label():
    soft, gt, cmap = case(8 * T + 2)
    on = (soft[:, 1:] >= 0.5).sum(1)
    assert (on > 1).sum() > 50 and (on == 0).sum() > 50 and (soft == 0.5).sum() > 50
    labels = torch_harden(soft).argmax(dim=1)
    assert sorted(labels.unique().tolist()) == list(range(10)) and sorted(gt.unique().tolist()) == list(range(12))


@pytest.mark.gpu
@pytest.mark.parametrize('S', [S_SECOND_TRIP, S_SECOND_TRIP - 1])
def test_second_trip_of_the_grid_stride_loop(S):
    """S above 4 T MAX_BLOCKS: the grid is capped and the first workgroups run the loop again; on the 16-byte path and, one pixel shorter, on the dword path.  GPU only
    (2.1 M pixels x 10 classes are minutes on the fiber emulator; the stride arithmetic is the one the small sizes run)."""
    segx.use_library(None)
    counts = check(types.SimpleNamespace(dev=torch.device('cuda', 0)), S, 10, 1)[0]
    assert (counts > 0).all()


def test_image_shape_integer_masks_and_threshold(backend):
    H, W = 6, 11
    soft, gt, cmap = (t.to(backend.dev) for t in case(H * W))
    for thres in (0.5, 0.25):
        want = composed(soft, gt, cmap, thres)
        for dtype in (torch.uint8, torch.int32, torch.int64):
            counts, labels, rgb = SF.onehot_case_tail(soft.view(2, 10, H, W), gt.view(2, H, W).to(dtype), cmap, T=thres)
            assert tuple(labels.shape) == (2, H, W) and tuple(rgb.shape) == (2, H, W, 3)
            assert torch.equal(counts.cpu(), want[0]) and torch.equal(labels.cpu().view(2, -1), want[1]) and torch.equal(rgb.cpu().view(2, -1, 3), want[2])
    counts = SF.onehot_case_tail(soft, torch.full((2, H * W), -1, dtype=torch.int64), want_labels=False)[0]
    assert not counts[:, :, 0].any() and not counts[:, :, 2].any()              # a negative label is no class
    nan = soft.clone(); nan[:, 3] = float('nan')
    assert not SF.onehot_case_tail(nan, gt, want_labels=False)[0][:, 2, :2].any()   # a NaN is off


@pytest.mark.parametrize('S', [4 * T + 1, 8 * T])
def test_each_null_combination(backend, S):
    soft, gt, cmap = (t.to(backend.dev) for t in case(S))
    want = composed(soft, gt, cmap)
    table = [tuple(int(v) for v in row) for row in cmap.cpu()]
    for use_gt in (True, False):
        for want_labels in (True, False):
            for cm in (cmap, table, None):
                if not use_gt and not want_labels and cm is None:
                    with pytest.raises(ValueError, match='nothing to compute'):
                        SF.onehot_case_tail(soft, None, None, want_labels=False)
                    continue
                counts, labels, rgb = SF.onehot_case_tail(soft, gt if use_gt else None, cm, want_labels=want_labels)
                assert (counts is None) == (not use_gt) and (labels is None) == (not want_labels) and (rgb is None) == (cm is None)
                assert counts is None or torch.equal(counts.cpu(), want[0])
                assert labels is None or torch.equal(labels.cpu(), want[1])
                assert rgb is None or torch.equal(rgb.cpu(), want[2])


def test_counts_are_initialised_by_every_call(backend):
    S = 8 * T + 2
    soft, gt, cmap = (t.to(backend.dev) for t in case(S))
    want = composed(soft, gt, cmap)
    counts = torch.full((2, 9, 3), 12345, dtype=torch.int32)
    labels, rgb = torch.full((2, S), 77, dtype=torch.uint8), torch.full((2, S, 3), 77, dtype=torch.uint8)
    c, l, r = SF.onehot_case_tail(soft, gt, cmap, counts=counts, labels=labels, rgb=rgb)
    assert c is counts and l is labels and r is rgb
    assert torch.equal(counts.cpu(), want[0]) and torch.equal(labels.cpu(), want[1]) and torch.equal(rgb.cpu(), want[2])
    gt2 = (9 - gt.clamp(max=9)).to(torch.uint8)
    SF.onehot_case_tail(soft, gt2, cmap, counts=counts, labels=labels, rgb=rgb)
    assert torch.equal(counts.cpu(), composed(soft, gt2, cmap)[0]) and torch.equal(labels.cpu(), want[1])
    SF.onehot_case_tail(torch.zeros_like(soft), torch.zeros_like(gt), counts=counts, want_labels=False)
    assert not counts.any()


def test_tail_refusals(backend):
    L, S = backend.L, 8
    soft, gt, cmap = (t.to(backend.dev) for t in case(S))
    counts, labels, rgb = torch.zeros(2, 9, 3, dtype=torch.int32), torch.zeros(2, S, dtype=torch.uint8), torch.zeros(2, S, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='null soft'):
        L.onehot_case_tail(None, gt, cmap, counts, labels, rgb, 2, 10, S)
    with pytest.raises(RuntimeError, match='none of counts, labels and rgb'):
        L.onehot_case_tail(soft, gt, cmap, None, None, None, 2, 10, S)
    with pytest.raises(RuntimeError, match='counts need the ground truth'):
        L.onehot_case_tail(soft, None, cmap, counts, labels, rgb, 2, 10, S)
    with pytest.raises(RuntimeError, match='rgb needs the colormap'):
        L.onehot_case_tail(soft, gt, None, counts, labels, rgb, 2, 10, S)
    for bad in (1, 17):
        with pytest.raises(RuntimeError, match='is not in 2'):
            L.onehot_case_tail(soft, gt, cmap, counts, labels, rgb, 2, bad, S)
    for bad in (0, -4, 1 << 31):
        with pytest.raises(RuntimeError, match='is not in 1'):
            L.onehot_case_tail(soft, gt, cmap, counts, labels, rgb, 2, 10, bad)
    for bad in (0, 65536):
        with pytest.raises(RuntimeError, match='B = '):
            L.onehot_case_tail(soft, gt, cmap, counts, labels, rgb, bad, 10, S)
    # the wrapper's own
    with pytest.raises(ValueError, match='float32'):
        SF.onehot_case_tail(soft.double(), gt)
    with pytest.raises(ValueError, match='classes'):
        SF.onehot_case_tail(torch.zeros(2, 17, S), gt)
    with pytest.raises(ValueError, match='is not the index mask'):
        SF.onehot_case_tail(soft, gt[:, :4])
    with pytest.raises(TypeError, match='integer index mask'):
        SF.onehot_case_tail(soft, gt.float())
    with pytest.raises(ValueError, match='counts need gt'):
        SF.onehot_case_tail(soft, None, counts=counts)
    with pytest.raises(ValueError, match='rgb needs a colormap'):
        SF.onehot_case_tail(soft, gt, rgb=rgb)
    with pytest.raises(ValueError, match='int32 \\[2, 9, 3\\]'):
        SF.onehot_case_tail(soft, gt, counts=torch.zeros(54, dtype=torch.int32))
    with pytest.raises(ValueError, match='labels is a contiguous uint8'):
        SF.onehot_case_tail(soft, gt, labels=torch.zeros(2, S, dtype=torch.int32))
    with pytest.raises(ValueError, match='rgb is a contiguous uint8'):
        SF.onehot_case_tail(soft, gt, cmap, rgb=torch.zeros(2, S, dtype=torch.uint8))
    with pytest.raises(ValueError, match='colormap'):
        SF.onehot_case_tail(soft, gt, cmap[:5])


def test_dice_table_equals_the_reference_exactly(backend):
    for i in range(2):
        soft, mask = G['metric_soft%d' % i][None].to(backend.dev), G['metric_mask%d' % i][None].to(backend.dev)
        for m in (mask, mask[:, None], mask.long()):
            got = infer2d.calc_batch_metric_onehot(soft, m, 10)
            assert got.dtype == np.float64 and got.shape == (1, 9)
            assert np.array_equal(got[0], G['metric'][i].numpy())
    assert (G['metric'][:, 6] == 1).all() and (G['metric'][:, 7] < 1e-6).all()     # absent from both: Dice 1; absent from the mask only: ~0
    small = SF.interp_linear(soft, (6, 10))                                        # a prediction of another size is resampled to the mask's first
    want = infer2d.calc_batch_metric_onehot(SF.interp_linear(small, tuple(mask.shape[1:])), mask, 10)
    assert np.array_equal(infer2d.calc_batch_metric_onehot(small, mask, 10), want)
    with pytest.raises(ValueError, match='classes'):
        infer2d.calc_batch_metric_onehot(soft, mask, 9)


# ---- onehot_inv_map and the export -------------------------------------------------------------------------------------------------------------------------------
def test_onehot_inv_map_equals_the_reference(backend):
    nhot, cmap = G['nhot'].float().to(backend.dev), G['colormap'].to(backend.dev)
    rgb, idx = D2.onehot_inv_map(nhot, cmap), D2.onehot_inv_map(nhot)
    assert rgb.dtype == torch.uint8 and idx.dtype == torch.int64
    assert torch.equal(rgb.cpu(), G['inv_rgb']) and torch.equal(idx.cpu(), G['inv_idx'])
    assert torch.equal(D2.onehot_inv_map(nhot[1], cmap).cpu(), G['inv_rgb3']) and torch.equal(D2.onehot_inv_map(nhot[1]).cpu(), G['inv_idx3'])
    assert torch.equal(D2.onehot_inv_map(nhot, [tuple(int(v) for v in r) for r in G['colormap']]).cpu(), G['inv_rgb'])
    assert torch.equal(D2.onehot_inv_map(G['nhot'].int().to(backend.dev), cmap.long()).cpu(), G['inv_rgb'])
    soft = torch.rand(1, 10, 5, 6)                                                  # arg-max over values that are no 0 / 1
    assert torch.equal(D2.onehot_inv_map(soft)[..., 0].cpu(), soft.argmax(dim=1).cpu())
    with pytest.raises(ValueError, match='n-hot maps'):
        D2.onehot_inv_map(nhot[0, 0])
    with pytest.raises(ValueError, match='classes'):
        SF.onehot_colormap(torch.zeros(1, 17, 2, 2))
    with pytest.raises(ValueError, match='colormap'):
        SF.onehot_colormap(nhot, cmap[:4])
    with pytest.raises(RuntimeError, match='is not in 1'):
        backend.L.onehot_colormap(nhot, None, torch.zeros(2, 6, 9, 3, dtype=torch.uint8), 2, 17, 54)


def test_export_masks_through_onehot_inv_map(backend):
    cmap = G['colormap'].to(backend.dev)
    soft = case(12 * 20)[0].view(2, 10, 12, 20).to(backend.dev)
    inv = functools.partial(D2.onehot_inv_map, colormap=cmap)
    out = infer2d.export_masks(soft, [(12, 20), (18, 25)], inv)
    assert [tuple(o.shape) for o in out] == [(12, 20, 3), (18, 25, 3)] and all(o.dtype == torch.uint8 for o in out)
    assert torch.equal(out[0], SF.onehot_case_tail(soft[:1], None, cmap, want_labels=False)[2][0])
    big = SF.interp_linear(soft[1:], (18, 25))
    assert torch.equal(out[1], D2.onehot_inv_map(D2.harden_segmap2d(big[0]), cmap))
    with pytest.raises(ValueError, match='remove_frag'):
        infer2d.export_masks(soft, [(12, 20), (12, 20)], inv, remove_frag=True)


@pytest.mark.skipif(not os.path.isdir('/root/reference/code'), reason='the reference is only present in the build container')
def test_committed_oct2d_fixture_is_what_the_generator_writes(tmp_path, monkeypatch):
    """as tests/test_golden_regen.py does for the small cases of make_golden.py: script and data agree"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_oct_golden
    monkeypatch.setattr(make_oct_golden.mg, 'OUT_DIR', str(tmp_path))
    make_oct_golden.case_oct2d()
    new = np.load(tmp_path / 'oct2d.npz', allow_pickle=False)
    assert sorted(new.files) == sorted(G)
    for k in new.files:
        old = G[k].numpy() if isinstance(G[k], torch.Tensor) else G[k]
        assert new[k].dtype == old.dtype and np.array_equal(new[k], old), k


# ---- loss weights, synthetic masks, the trainer's flags (host only) ------------------------------------------------------------------------------------------------
def test_oct_loss_weights_equal_the_reference():
    assert engine.BCE_WEIGHT['oct'] == G['bce_weight'].tolist()
    pw, cw = engine.loss_weights('oct', 'cpu')
    assert torch.equal(pw, G['pos_weight']) and torch.equal(cw, G['class_w'])
    pw3, cw3 = engine.loss_weights('oct', 'cpu', focus_class=3)
    assert torch.equal(pw3, G['pos_weight']) and torch.equal(cw3, G['class_w_focus3'])
    assert torch.equal(engine.loss_weights('polyp', 'cpu', focus_class=1)[1], engine.loss_weights('polyp', 'cpu')[1])     # two classes: no focus (train2d.py:1125)
    assert torch.equal(engine.loss_weights('fundus', 'cpu', focus_class=2)[1], torch.tensor([0., 1., 2.]) / 3)
    with pytest.raises(ValueError, match='focus_class'):
        engine.loss_weights('oct', 'cpu', focus_class=10)


def test_synth_batch_makes_rectangles_and_every_oct_class():
    cfg = dict(dim=2, task='oct', num_classes=10, size=(64, 96))
    x, m = engine.synth_batch(cfg, 3, 'cpu')
    assert tuple(x.shape) == (3, 3, 64, 96) and tuple(m.shape) == (3, 1, 64, 96) and m.dtype == torch.uint8
    assert all(sorted(m[b].unique().tolist()) == list(range(10)) for b in range(3))
    assert torch.equal(m, synth_oct_mask(3, 64, 96, 10, 1338)) and not torch.equal(m[0], m[1])
    assert (m[:, 0, 1:] >= m[:, 0, :-1]).all()                                  # stacked bands: the class never decreases downwards
    assert torch.equal(engine.map_mask('oct', m).sum(1), torch.ones(3, 64, 96))
    x, m = engine.synth_batch(dict(dim=2, task='fundus', num_classes=3, size=(64, 96)), 2, 'cpu')
    assert tuple(x.shape) == (2, 3, 64, 96) and tuple(m.shape) == (2, 3, 64, 96) and m[:, 0].any() and m[:, 1].any()
    sq = engine.synth_batch(dict(engine.CONFIGS['cfg1'], size=(64, 64)), 2, 'cpu')
    assert tuple(sq[0].shape) == (2, 3, 64, 64) and tuple(sq[1].shape) == (2, 3, 64, 64)


def test_trainer_flags():
    args, cfg = train2d.parse_args(['--task', 'oct', '--patch', '64,96', '--focus', '3'])
    assert cfg['size'] == (64, 96) and cfg['num_classes'] == 10 and cfg['task'] == 'oct' and args.focus_class == 3
    pw, cw = engine.loss_weights(cfg['task'], 'cpu', args.focus_class)
    assert torch.equal(pw, G['pos_weight']) and torch.equal(cw, G['class_w_focus3'])
    assert train2d.parse_args(['--task', 'oct'])[1]['size'] == (288, 512)
    assert train2d.parse_args(['--task', 'oct', '--insize', '96,64'])[1]['size'] == (96, 64)
    assert train2d.parse_args(['--task', 'fundus', '--patch', '64,96'])[1]['size'] == (64, 96)
    a, c = train2d.parse_args(['--task', 'polyp'])
    assert c['size'] == (320, 320) and c['num_classes'] == 2 and a.focus_class == -1
    assert train2d.parse_args(['--patch', '512'])[1]['size'] == (512, 512) and train2d.parse_args([])[1]['size'] == (576, 576)
    for bad in (['--task', 'oct', '--patch', '60,96'], ['--task', 'oct', '--patch', '64,100'], ['--patch', '100'], ['--patch', '64,96,8'], ['--patch', 'big']):
        with pytest.raises(SystemExit, match='--patch'):
            train2d.parse_args(bad)
    with pytest.raises(SystemExit, match='--focus'):
        train2d.parse_args(['--task', 'oct', '--focus', '10'])
