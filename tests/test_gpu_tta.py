"""GPU (-m gpu): flip test-time augmentation of the sliding-window evaluation (tta= of infer2d / infer3d) -- the fused form and its hipGraph replay against the
composed host loop (torch.flip, the eager evaluation per view, the adds in view order, one division, harden_segmap: infer_common.composed_tta), bit for bit wherever
the forwards see the eager shapes.  2-D: Segtran2d on resnet34 at 64 x 96, a 2 x 3 x 64 x 144 batch under two windows that overlap in 48 columns
(test_gpu_resnet_model.py); 3-D: the cfg4 net of test_gpu_sliding3d.py at 112 x 112 x 16."""
import functools

import numpy as np
import pytest
import torch

from segtran_amd import engine, infer2d, infer3d, segx
from segtran_amd import functional as SF
from test_kernels_infer import rnd
from test_gpu_sliding3d import the_net, volume, same, PATCH

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SMALL = dict(dim=2, task='fundus', num_classes=3, translayers=1, compress=[1, 1], attractors=32, bs=2, size=(64, 96))
WINDOWS = dict(orig_input_size=(64, 96), patch_size=(64, 96), stride=(64, 48), task_name='fundus', num_classes=3)
GEO = (WINDOWS['orig_input_size'], WINDOWS['patch_size'], WINDOWS['stride'])
SHAPE = (2, 3, 64, 144)
VIEWS2 = ((), (1,), (0,), (0, 1))
VIEWS3 = ((), (0,), (2,), (0, 1, 2))
NEAR = 2.5e-4                      # a quarter of the project's 1e-3 logit bar: the sigmoid is 1/4-Lipschitz, and a mean of views moves no further than its terms


@functools.lru_cache(None)
def net2d():
    return engine.build_model(SMALL, DEV, dropout_prob=0.0, attractors=32, backbone_type='resnet34').eval()


@functools.lru_cache(None)
def batch(seed):
    return rnd(*SHAPE, seed=seed).to(DEV)


@functools.lru_cache(None)
def composed2d(seed):
    """the referee of every 2-D test, computed once per image: (preds_hard, preds_soft) of the composed host loop"""
    return infer2d.test_single_batch(net2d(), batch(seed), fused=False, tta=VIEWS2, **WINDOWS)


def test_composed_loop_is_what_it_says():
    """the referee itself, written out with torch.flip around today's call"""
    net, x = net2d(), batch(91)
    total = None
    for view in VIEWS2:
        dims = tuple(2 + a for a in view)
        soft = infer2d.test_single_batch(net, torch.flip(x, dims) if dims else x, **WINDOWS)[1]
        soft = torch.flip(soft, dims) if dims else soft
        total = soft if total is None else total + soft
    mean = total / torch.full((), 4.0, device=DEV)
    want_soft, want_hard = SF.harden_segmap(mean.contiguous())
    hard, soft = composed2d(91)
    assert hard.dtype == torch.int32 and torch.equal(soft, want_soft) and torch.equal(hard, want_hard.to(torch.int32))
    assert not torch.equal(soft, infer2d.test_single_batch(net, x, **WINDOWS)[1])                  # the other views do change the map
    assert 0 < hard[:, 1:].float().mean() < 1


def test_fused_tta_with_the_eager_forwards_is_the_composed_loop_bit_for_bit():
    want_hard, want_soft = composed2d(91)
    hard, soft = infer2d.test_single_batch(net2d(), batch(91), fused=True, window_batch=1, tta=VIEWS2, **WINDOWS)
    assert hard.dtype == torch.int32 and torch.equal(hard, want_hard) and torch.equal(soft, want_soft)


def test_fused_tta_with_stacked_windows_is_near_the_composed_loop():
    """default stacking: each view's two windows in one net() call, so the GEMM shapes differ from the eager path's"""
    want_hard, want_soft = composed2d(91)
    hard, soft = infer2d.test_single_batch(net2d(), batch(91), fused=True, tta=VIEWS2, **WINDOWS)
    err = (soft - want_soft).abs().max().item()
    print('stacked tta: |soft - composed| = %.3e' % err)
    assert err <= NEAR
    decided = (want_soft - 0.5).abs() > NEAR
    decided[:, 0] = decided[:, 1:].all(1)                                # the background label depends on every other class
    assert decided.float().mean().item() > 0.9
    assert torch.equal(hard[decided], want_hard[decided])


def test_graph_replays_equal_the_fused_eager_run_on_two_images():
    net = net2d()
    g = infer2d.GraphedSlidingWindow(net, SHAPE, *GEO, 3, fold_bn=False, window_batch=1, tta=VIEWS2)
    try:
        seen = []
        for seed in (91, 92):
            hard, soft = g(batch(seed))
            want_hard, want_soft = infer2d.test_single_batch(net, batch(seed), fused=True, window_batch=1, tta=VIEWS2, **WINDOWS)
            assert torch.equal(hard, want_hard) and torch.equal(soft, want_soft)
            assert torch.equal(soft, composed2d(seed)[1])
            seen.append(soft.clone())
        assert not torch.equal(seen[0], seen[1]) and g.replays == 2
    finally:
        g.close()


def test_graphed_batch_evaluation_tail_reads_the_averaged_map():
    net = net2d()
    values = (255, 128, 0)
    g = infer2d.GraphedBatchEvaluation(net, SHAPE, *GEO, 3, fold_bn=False, window_batch=1, values=values, with_extents=True, tta=VIEWS2)
    try:
        for seed in (91, 92):
            mask = (rnd(*SHAPE, seed=100 + seed) > 0).float().to(DEV)
            hard, soft, counts, ext, labels = g(batch(seed), mask)
            want_hard, want_soft = composed2d(seed)
            assert torch.equal(soft, want_soft) and torch.equal(hard, want_hard)
            c0, e0, l0, _ = SF.nhot_case_tail(want_soft, mask, values=values, want_extents=True)
            assert torch.equal(counts, c0) and torch.equal(ext, e0) and torch.equal(labels, l0)
            assert counts[..., 1].min() > 0
    finally:
        g.close()


def test_all_cases_2d_gives_the_tables_of_the_per_batch_calls():
    net = net2d()
    masks = [(rnd(*SHAPE, seed=110 + i) > 0).float().to(DEV) for i in range(2)]
    batches = [(batch(91 + i), masks[i]) for i in range(2)]
    args = ('fundus', 3) + GEO
    tables = [infer2d.calc_batch_metric(composed2d(91 + i)[1], masks[i], 3) for i in range(2)]
    want = sum(t.sum(axis=0) for t in tables) / 4
    for kw in (dict(fused=False), dict(fused=True, window_batch=1), dict(fused=True, window_batch=1, device_tail=True)):
        got, n = infer2d.test_all_cases(net, batches, *args, tta=VIEWS2, **kw)
        assert n == 4 and np.array_equal(got, want), kw
    vtables = [infer2d.calc_batch_metric(composed2d(91 + i)[1], masks[i], 3, do_calc_vcdr_error=True) for i in range(2)]
    got, n = infer2d.test_all_cases(net, batches, *args, fused=True, window_batch=1, do_calc_vcdr_error=True, tta=VIEWS2)
    assert np.array_equal(got, sum(t.sum(axis=0) for t in vtables) / 4) and np.array_equal(n, np.full(3, 4.0))
    index = [(rnd(2, 64, 144, seed=120 + i) > 0).to(torch.uint8).to(DEV) * (1 + i) for i in range(2)]                # index masks with classes {0, 1} and {0, 2}
    rows = [infer2d.calc_batch_metric_onehot(composed2d(91 + i)[1], index[i], 3) for i in range(2)]
    got, n = infer2d.test_all_cases(net, [(batch(91 + i), index[i]) for i in range(2)], *args, fused=True, window_batch=1, gt_is_index=True, tta=VIEWS2)
    assert n == 4 and np.array_equal(got, sum(r.sum(axis=0) for r in rows) / 4)


# ---- 3-D ---------------------------------------------------------------------------------------------------------------------------------------------------
ROW = (112, 280, 16)                       # one x row of four windows (y origins 0, 56, 112, 168): batch 3 runs it as 3 + 1, batch 1 as four calls
TWO = (120, 112, 16)                       # two windows (x origins 0 and 8)


def _case3d(shape, seed, batch_size, **kw):
    return infer3d.test_single_case(the_net(), volume(shape, seed)[0], PATCH, PATCH, batch_size, 56, 16, 'brats', **kw)


@functools.lru_cache(None)
def composed3d(shape, seed, batch_size):
    return _case3d(shape, seed, batch_size, fused=False, tta=VIEWS3)


def test_composed_loop_3d_is_what_it_says():
    x = volume(TWO, 11)[0]
    total = None
    for view in VIEWS3:
        dims = tuple(1 + a for a in view)
        soft = infer3d.test_single_case(the_net(), torch.flip(x, dims) if dims else x, PATCH, PATCH, 2, 56, 16, 'brats')[1]
        soft = torch.flip(soft, dims) if dims else soft
        total = soft if total is None else total + soft
    mean = total / torch.full((), 4.0, device=DEV)
    want_soft, want_hard = SF.harden_segmap(mean.unsqueeze(0).contiguous(), mode=1)
    assert same(composed3d(TWO, 11, 2), (want_hard[0], want_soft[0]))


@pytest.mark.parametrize('batch_size', [1, 3])
def test_fused_tta_3d_is_the_composed_loop_bit_for_bit(batch_size):
    assert len(infer3d.sliding_windows(*ROW, PATCH, 56, 16, batch_size)[2]) == 4
    want = composed3d(ROW, 11, batch_size)
    got = _case3d(ROW, 11, batch_size, fused=True, tta=VIEWS3)
    assert tuple(got[0].shape) == (4,) + ROW and same(got, want)
    assert got[1].min() > 0 and got[1].max() < 1 and 0 < got[0].mean() < 1
    assert not torch.equal(got[1], _case3d(ROW, 11, batch_size, fused=True)[1])


def test_graph_replays_3d_equal_the_composed_loop_and_its_tail():
    g = infer3d.GraphedSlidingWindow3d(the_net(), (4,) + TWO, PATCH, PATCH, 2, 56, 16, fold_bn=False, warmup=1, with_mask=True, tta=VIEWS3)
    try:
        seen = []
        for seed in (11, 13):
            x, lab = volume(TWO, seed)
            hard, soft, labels, counts = g(x, lab)
            want = composed3d(TWO, seed, 2)
            assert same((hard, soft), want)
            want_counts, want_labels = SF.brats_case_tail(want[1], want[0], lab)
            assert torch.equal(counts, want_counts) and torch.equal(labels, want_labels)
            seen.append(counts.clone())
        assert not torch.equal(seen[0], seen[1])
    finally:
        g.close()


def test_all_cases_3d_gives_the_table_of_the_per_case_calls():
    cases = [(TWO, 11), (TWO, 13)]
    db = [dict(image=volume(s, seed)[0].cpu(), mask=volume(s, seed)[1].cpu().long(), image_path='/data/brats/case_%d.nii.gz' % i) for i, (s, seed) in enumerate(cases)]
    total, valid = np.zeros((3, 4)), np.zeros((3, 4))
    for s, seed in cases:
        hard, soft = composed3d(s, seed, 2)
        m, ok = infer3d.case_metrics(SF.brats_case_tail(soft, hard, volume(s, seed)[1], want_labels=False)[0])
        total += m; valid += ok
    kw = dict(batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16, tta=VIEWS3)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = total / valid
    for form in (dict(fused=False), dict(fused=True), dict(graph=True)):
        assert np.array_equal(infer3d.test_all_cases(the_net(), db, **form, **kw), want, equal_nan=True), form


# ---- tta=None is today's path ------------------------------------------------------------------------------------------------------------------------------
def test_without_tta_neither_new_kernel_is_launched(monkeypatch):
    calls = []
    cls = type(segx.lib())
    for name in ('window_gather_views', 'window_merge_views'):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    net, x = net2d(), batch(91)
    mask = (rnd(*SHAPE, seed=130) > 0).float().to(DEV)
    for fused in (False, True):
        infer2d.test_single_batch(net, x, fused=fused, **WINDOWS)
        infer2d.test_all_cases(net, [(x, mask)], 'fundus', 3, *GEO, fused=fused)
    infer2d.test_all_cases(net, [(x, mask)], 'fundus', 3, *GEO, fused=True, device_tail=True)
    infer2d.test_all_cases(net, [(x, mask[:, 0].to(torch.uint8))], 'fundus', 3, *GEO, fused=True, gt_is_index=True)
    for make in (lambda: infer2d.GraphedSlidingWindow(net, SHAPE, *GEO, 3, fold_bn=False, warmup=1),
                 lambda: infer2d.GraphedBatchEvaluation(net, SHAPE, *GEO, 3, fold_bn=False, warmup=1)):
        g = make()
        try:
            g(x, mask) if isinstance(g, infer2d.GraphedBatchEvaluation) else g(x)
        finally:
            g.close()
    vol, lab = volume(TWO, 11)
    for fused in (False, True):
        _case3d(TWO, 11, 2, fused=fused)
    db = [dict(image=vol.cpu(), mask=lab.cpu().long(), image_path='case_0.nii.gz')]
    infer3d.test_all_cases(the_net(), db, batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16)
    g = infer3d.GraphedSlidingWindow3d(the_net(), (4,) + TWO, PATCH, PATCH, 2, 56, 16, fold_bn=False, warmup=1)
    try:
        g(vol)
    finally:
        g.close()
    assert calls == []
    infer2d.test_single_batch(net, x, fused=True, tta=((1,),), **WINDOWS)                           # and with tta they are the path: one launch each
    assert calls == ['window_gather_views', 'window_merge_views']
