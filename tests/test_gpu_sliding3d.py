"""GPU (-m gpu): the 3-D case evaluation in one pass -- infer3d.test_single_case(fused=True), infer3d.GraphedSlidingWindow3d and infer3d.test_all_cases -- against the
eager loop of test_util3d.test_single_case, bit for bit: the fused sequence hands net() the eager loop's batches and the merge is the accumulate + harden
arithmetic, so nothing may differ for any batch_size.  cfg4 at (112, 112, 16), built as test_gpu_model.py::test_eval_path_3d_vs_reference builds it."""
import functools

import numpy as np
import pytest
import torch

import segtran_amd
from segtran_amd import engine, infer3d
from segtran_amd import functional as SF
from segtran_amd import test_util3d as T3
from segtran_amd.dataloaders import datasets3d as D3
from segtran_amd.synth import synth_brats
from util import golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
PATCH = (112, 112, 16)
BIG = (120, 224, 16)                       # 2 x 3 x 1 windows: at batch 2 every x row runs as a chunk of 2 and a chunk of 1


@functools.lru_cache(None)
def the_net():
    g = golden('eval3d')
    return engine.build_model(dict(engine.CONFIGS['cfg4'], size=PATCH), DEV, dropout_prob=0.0, attractors=int(g['A'])).eval()


@functools.lru_cache(None)
def volume(shape, seed):
    """(image [4, H, W, D], raw labels [H, W, D] with some 3 -> 4, as BraTS files hold them) on the device"""
    x, lab = synth_brats(1, *shape, seed)
    lab = lab[0]
    lab[lab == 3] += (torch.arange(lab.numel(), device='cpu').reshape(lab.shape)[lab == 3] % 2)       # every other 3 becomes the raw 4
    return x[0].to(DEV), lab.to(DEV)


@functools.lru_cache(None)
def eager(shape, seed, batch_size, orig=PATCH, **kw):
    net = the_net()
    assert not net.batchnorm_folded and not net.training
    return infer3d.test_single_case(net, volume(shape, seed)[0], orig, PATCH, batch_size, 56, 16, 'brats', fused=False, **dict(kw))


def fused(shape, seed, batch_size, orig=PATCH, **kw):
    return infer3d.test_single_case(the_net(), volume(shape, seed)[0], orig, PATCH, batch_size, 56, 16, 'brats', fused=True, **kw)


def same(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))


# ---- fused path -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,batch_size', [(BIG, 2), (BIG, 1), ((112, 168, 12), 2)])
def test_fused_equals_eager(shape, batch_size):
    """BIG at batch 2: chunks of 2 and 1 per row; at batch 1: six forwards of one window; 112 x 168 x 12: the depth is padded to 16 (left pad 2), the output has the
    image's shape"""
    want = eager(shape, 11, batch_size)
    got = fused(shape, 11, batch_size)
    assert tuple(got[0].shape) == (4,) + shape and same(got, want)
    assert got[1].min() > 0 and got[1].max() < 1 and 0 < got[0].mean() < 1                       # a real soft map and a non-trivial hard one


def test_fused_equals_eager_with_resampled_windows():
    """orig_patch_size (120, 120, 16) != input_patch_size: one interp_linear over all gathered windows instead of one per batch"""
    shape = (128, 180, 16)                                                                          # 2 x 3 windows (origins 0, 8 and 0, 56, 60)
    assert len(infer3d.sliding_windows(*shape, (120, 120, 16), 56, 16, 2)[2]) == 6
    assert same(fused(shape, 12, 2, orig=(120, 120, 16)), eager(shape, 12, 2, orig=(120, 120, 16)))


def test_fused_equals_eager_folded_and_in_three_terms():
    net = the_net()
    want_fold = eager(BIG, 11, 2, fold_bn=True)
    assert same(fused(BIG, 11, 2, fold_bn=True), want_fold) and not net.batchnorm_folded
    want_x3 = eager(BIG, 11, 2, precision='bf16x3')
    assert same(fused(BIG, 11, 2, precision='bf16x3'), want_x3)
    assert not torch.equal(want_x3[1], eager(BIG, 11, 2)[1])                                       # the mode is on in both
    with pytest.raises(NotImplementedError):
        infer3d.test_single_case(net, volume(BIG, 11)[0], PATCH, PATCH, 2, 56, 16, 'atria', fused=True)
    with pytest.raises(NotImplementedError):
        infer3d.test_single_case(net, volume(BIG, 11)[0], PATCH, PATCH, 2, 56, 16, 'brats', net_type='vnet', fused=True)


# ---- graph path -------------------------------------------------------------------------------------------------------------------------------------------
def _graphed(net, **kw):
    return infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, **kw)


def test_replays_equal_the_eager_evaluation_and_its_tail():
    net = the_net()
    assert segtran_amd.GraphedSlidingWindow3d is infer3d.GraphedSlidingWindow3d
    g = _graphed(net, fold_bn=False, with_mask=True)
    try:
        seen = []
        for seed in (11, 13):                                # the second replay: the static inputs are refreshed, the static outputs rewritten
            x, lab = volume(BIG, seed)
            hard, soft, labels, counts = g(x, lab)
            want = eager(BIG, seed, 2)
            assert same((hard, soft), want) and same((hard, soft), fused(BIG, seed, 2))
            want_counts, want_labels = SF.brats_case_tail(want[1], want[0], lab)
            assert torch.equal(labels, want_labels) and torch.equal(counts, want_counts)
            assert counts[:, 0].min() > 0 and len(labels.unique()) > 1
            seen.append((soft.clone(), counts.clone()))
        assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
        assert g.replays == 2
        with pytest.raises(ValueError, match='mask'):
            g(volume(BIG, 11)[0])
    finally:
        g.close()
    g = _graphed(net, fold_bn=False, with_labels=False)      # nothing of the tail asked for
    try:
        hard, soft, labels, counts = g(volume(BIG, 11)[0])
        assert labels is None and counts is None and same((hard, soft), eager(BIG, 11, 2))
    finally:
        g.close()


def test_lifecycle():
    net = the_net()
    x = volume(BIG, 11)[0]
    try:
        net.train()
        with pytest.raises(RuntimeError, match='eval'):
            _graphed(net)
        net.eval()
        assert not net.batchnorm_folded
        g = _graphed(net, fold_bn=True)
        assert net.batchnorm_folded
        hard, soft, labels, counts = g(x)
        assert counts is None and same((hard, soft), eager(BIG, 11, 2, fold_bn=True))
        assert torch.equal(labels, SF.brats_case_tail(soft, hard)[1])
        with pytest.raises(ValueError, match='captured for'):
            g(x[:, :100])
        net.train()
        with pytest.raises(RuntimeError, match='train mode'):
            g(x)
        net.eval()                                              # train() dropped the fold: the captured kernels read operands that are no longer the net's
        with pytest.raises(RuntimeError, match='fold'):
            g(x)
        g.close()
        assert not net.batchnorm_folded                        # as before construction
        with pytest.raises(RuntimeError, match='closed'):
            g(x)

        infer3d.fold_batchnorm(net)                             # a net the caller folded stays folded
        g = _graphed(net, fold_bn=True, with_labels=False)
        g(x)
        g.close()
        assert net.batchnorm_folded
        infer3d.unfold_batchnorm(net)

        with pytest.raises(ValueError, match='stride'):         # a failed construction leaves the net as it was found
            infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 113, 16, fold_bn=True)
        assert not net.batchnorm_folded
    finally:
        net.eval()
        infer3d.unfold_batchnorm(net)


# ---- case loop --------------------------------------------------------------------------------------------------------------------------------------------
CASES = [(BIG, 11), ((112, 168, 12), 11), (BIG, 13)]


def _db():
    return [dict(image=volume(s, seed)[0].cpu(), mask=volume(s, seed)[1].cpu().long(), image_path='/data/brats/case_%d.nii.gz' % i) for i, (s, seed) in enumerate(CASES)]


@functools.lru_cache(None)
def reference_loop():
    """reference test_util3d.py:15-91 from the eager pieces: per case map the ground truth, test_single_case, calculate_metric_percase, and the export through
    brats_inv_map_label + argmax + the 3 -> 4 relabel"""
    total, valid_counts, exports = np.zeros((3, 4)), np.zeros((3, 4)), []
    for s, seed in CASES:
        _, lab = volume(s, seed)
        mask = lab.long() - (lab == 4).long()
        gt = D3.brats_map_label(mask.unsqueeze(0).float(), False)[0]
        hard, soft = eager(s, seed, 2)
        metric, valid = T3.calculate_metric_percase(hard, gt, 4)
        total += metric; valid_counts += valid
        out = torch.argmax(D3.brats_inv_map_label(soft), dim=0)
        out += (out == 3).long()
        exports.append(out.to(torch.uint8))
    with np.errstate(divide='ignore', invalid='ignore'):
        return total / valid_counts, exports


@pytest.mark.parametrize('graph', [False, True])
def test_all_cases_equals_the_reference_loop(graph):
    want_avg, want_exports = reference_loop()
    got = []
    avg = infer3d.test_all_cases(the_net(), _db(), batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16,
                                 on_labels=lambda name, vol: got.append((name, vol)), graph=graph)
    assert avg.shape == (3, 4) and np.array_equal(avg, want_avg, equal_nan=True)
    assert (avg[:, :2] > 0).all() and np.isnan(avg[:, 2:]).all()                                  # Dice / Jaccard are real numbers; the surface columns are valid nowhere
    assert [n for n, _ in got] == ['case_0', 'case_1', 'case_2']
    for (_, vol), want in zip(got, want_exports):
        assert vol.dtype == torch.uint8 and torch.equal(vol, want)
    assert not the_net().batchnorm_folded


def test_all_cases_other_arguments():
    net = the_net()
    db = _db()[:1]
    kw = dict(batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16)
    assert np.array_equal(infer3d.test_all_cases(net, db, has_mask=False, **kw), np.zeros((3, 4)))
    base = infer3d.test_all_cases(net, db, fused=False, **kw)
    s, seed = CASES[0]
    _, lab = volume(s, seed)
    gt = SF.label_nhot((lab - (lab == 4).to(lab.dtype)).unsqueeze(0), 'brats')[0]
    metric, valid = infer3d.calculate_metric_percase(eager(s, seed, 2)[0], gt, 4, hd95=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.array_equal(infer3d.test_all_cases(net, db, hd95=True, **kw), metric / valid, equal_nan=True)
        assert np.array_equal(base[:, :2], (metric / valid)[:, :2])
    with pytest.raises(NotImplementedError):
        infer3d.test_all_cases(net, db, num_classes=2, **kw)
    with pytest.raises(NotImplementedError):
        infer3d.test_all_cases(net, db, task_name='atria', **kw)
    with pytest.raises(TypeError):
        infer3d.test_all_cases(net, db, test_interp=(0.5,), **kw)
