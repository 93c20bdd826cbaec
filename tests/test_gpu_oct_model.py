"""GPU (-m gpu): the OCT task through the model -- the 10-class train step on a 64 x 96 input against the reference fixture (seg2d_oct_train.npz, tests/golden/
make_oct_golden.py), the three evaluation forms at 10 classes bit for bit, the index-mask evaluation against the composed one, and the trainer's loop."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from segtran_amd import engine, functional as SF, infer2d, segx, train2d
from segtran_amd.dataloaders.datasets2d import index_to_onehot
from segtran_amd.synth import synth_oct_mask
from test_gpu_model import _grads_vs_golden
from test_kernels_infer import rnd
from util import golden, assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
OCT = dict(dim=2, task='oct', num_classes=10, translayers=1, compress=[1, 1], attractors=32, bs=2, size=(64, 96))
WINDOWS = dict(orig_input_size=(64, 96), patch_size=(64, 96), stride=(64, 48), task_name='oct', num_classes=10)
SHAPE = (2, 3, 64, 144)                                      # two 64 x 96 windows that overlap in 48 columns


@pytest.mark.parametrize('tile_engine', ['x6', 'f32'])
def test_segtran2d_oct_train_step_vs_reference(tile_engine):
    """10 classes, 1 layer, 32 attractors, 2 x 3 x 64 x 96 -> 8 x 12 tokens, the index mask through segx_index_onehot; the tolerances of
    test_gpu_model.test_segtran2d_polyp_cfg3_vs_reference, on both tile engines"""
    L = segx.lib()
    prev = L.set_engine(tile_engine)
    try:
        g = golden('seg2d_oct_train')
        net = engine.build_model(OCT, DEV, dropout_prob=0.0, attractors=int(g['A']))
        net.backbone.drop_connect_rate = 0.0
        net.train()
        y = net(g['x'].to(DEV))
        assert tuple(y.shape) == (2, 10, 64, 96)
        assert_close(y, g['logits'], 1e-4, 'logits')
        safe = g['logits'].abs() > 1e-4
        assert torch.equal((y.cpu() > 0)[safe], g['labels'][safe]), 'hardened label map differs'
        nhot = engine.map_mask('oct', g['mask'].to(DEV))
        assert torch.equal(nhot.cpu(), g['nhot'].float())
        pw, cw = engine.loss_weights('oct', DEV)
        loss, _ = SF.seg_loss(y, nhot, pw, cw)
        assert abs(loss.item() - float(g['loss'])) < 5e-5
        loss.backward()
        _grads_vs_golden(net, g, tol=2e-3)
    finally:
        L.set_engine(prev)


@pytest.fixture(scope='module')
def oct_net():
    return engine.build_model(OCT, DEV, dropout_prob=0.0, attractors=32).eval()


def test_three_evaluation_forms_are_bit_identical_at_ten_classes(oct_net):
    x = rnd(*SHAPE, seed=81).to(DEV)
    want_hard, want_soft = infer2d.test_single_batch(oct_net, x, fused=False, **WINDOWS)
    assert tuple(want_soft.shape) == (2, 10, 64, 144) and want_hard.dtype == torch.int32 and 0 < want_hard[:, 1:].float().mean() < 1
    hard, soft = infer2d.test_single_batch(oct_net, x, fused=True, window_batch=1, **WINDOWS)
    assert torch.equal(hard, want_hard) and torch.equal(soft, want_soft)
    g = infer2d.GraphedSlidingWindow(oct_net, SHAPE, WINDOWS['orig_input_size'], WINDOWS['patch_size'], WINDOWS['stride'], 10, fold_bn=False, window_batch=1)
    try:
        for xi, (wh, ws) in ((x, (want_hard, want_soft)),):
            hard, soft = g(xi)
            assert torch.equal(hard, wh) and torch.equal(soft, ws)
        x2 = rnd(*SHAPE, seed=82).to(DEV)
        hard, soft = g(x2)
        wh, ws = infer2d.test_single_batch(oct_net, x2, fused=False, **WINDOWS)
        assert torch.equal(hard, wh) and torch.equal(soft, ws) and not torch.equal(ws, want_soft)
    finally:
        g.close()


@pytest.mark.parametrize('fused', [False, True])
def test_all_cases_on_index_masks_equals_the_composed_path(oct_net, fused):
    """two batches; the second one's masks are larger than the images, so its predictions are resampled first"""
    batches = [(rnd(*SHAPE, seed=83).to(DEV), synth_oct_mask(2, 64, 144, 10, 5).to(DEV)),
               (rnd(1, 3, 64, 144, seed=84).to(DEV), synth_oct_mask(1, 80, 160, 10, 6).to(DEV))]
    kw = dict(WINDOWS, fused=fused, window_batch=1 if fused else None)
    want, n = infer2d.test_all_cases(oct_net, batches, mask_prepred_mapping_func=functools.partial(index_to_onehot, num_classes=10), **kw)
    got, m = infer2d.test_all_cases(oct_net, batches, gt_is_index=True, **kw)
    assert n == m == 3 and got.shape == (9,) and got.dtype == np.float64
    assert np.array_equal(got, want) and (got > 0).all() and (got < 1).all()
    for (x, mask) in batches:                                                       # and per batch: the table from the counts is the composed table
        soft = infer2d.test_single_batch(oct_net, x, **kw)[1]
        assert np.array_equal(infer2d.calc_batch_metric_onehot(soft, mask, 10), infer2d.calc_batch_metric(soft, index_to_onehot(mask, 10), 10))
    with pytest.raises(ValueError, match='gt_is_index'):
        infer2d.test_all_cases(oct_net, batches, gt_is_index=True, mask_prepred_mapping_func=lambda m: m, **kw)


def test_two_trainer_iterations_run(tmp_path, monkeypatch):
    """python -m segtran_amd.train2d --task oct --patch 64,96 --synthweights, two iterations in this process: the index masks, the 10-class loss with --focus and
    the checkpoint at the last iteration (written under ../model, relative to the working directory)"""
    work = tmp_path / 'work'
    work.mkdir()
    monkeypatch.chdir(work)
    net = train2d.main(['--task', 'oct', '--patch', '64,96', '--synthweights', '--maxiter', '2', '--bs', '2', '--attractors', '32', '--focus', '3',
                        '--logiter', '1'])
    assert all(torch.isfinite(p).all() for p in net.parameters())
    saved = glob.glob(os.path.join(str(tmp_path), 'model', 'segtran-oct-*', 'iter_2.pth'))
    assert len(saved) == 1
    ck = torch.load(saved[0], map_location='cpu')
    assert ck['iter_num'] == 2 and ck['args']['task_name'] == 'oct' and ck['args']['focus_class'] == 3
    head = [v for k, v in ck['model'].items() if v.dim() >= 1 and v.shape[0] == 10]
    assert head, 'no 10-class tensor in the checkpoint'
