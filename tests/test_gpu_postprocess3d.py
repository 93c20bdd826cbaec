"""GPU (-m gpu): connected-component post-processing inside the 3-D case evaluation -- the `postprocess=` argument of infer3d.test_single_case,
infer3d.GraphedSlidingWindow3d and infer3d.test_all_cases -- against the same evaluation WITHOUT the argument followed by the torch referee's BraTS rule
(tests/components3d_referee.py, running on the device), bit for bit; and one full-size labelling against the referee.  The model and the volumes are those of
tests/test_gpu_sliding3d.py (cfg4 at (112, 112, 16) on a 120 x 224 x 16 volume: a little more than one window along x, two along y).

Which tests feed CONSTRUCTED predictions: test_postprocess_brats_with_satellites builds its preds_hard (a main blob, two satellites, speckled ET) and takes only
preds_soft from the network; every other test runs on what the network itself predicts.  The synthetic-weight network's own WT is ONE component (428564 of the
430080 voxels on seed 11), so on its predictions the WT options remove nothing and only the ET rule changes the result (68938 ET voxels -> 0 under P_DROP); the WT
filtering inside the evaluation is what the constructed test and tests/test_components3d.py hold to the referee."""
import functools

import numpy as np
import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer3d, segx
from segtran_amd import test_util3d as T3
from segtran_amd.dataloaders import datasets3d as D3
from components3d_referee import ref_brats, ref_labels3d
from test_gpu_sliding3d import BIG, PATCH, same, the_net, volume

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
P_SMALL = dict(wt_min_voxels=30, et_min_voxels=10)                                   # drops the small WT components; ET stays
P_DROP = dict(wt_largest_only=True, et_min_voxels=1 << 30, connectivity=6)           # one WT component; ET can never reach the threshold: dropped
ARGS = (PATCH, PATCH, 2, 56, 16, 'brats')


@functools.lru_cache(None)
def plain(seed, tta=None):
    """(preds_hard, preds_soft) of the fused evaluation without post-processing"""
    return infer3d.test_single_case(the_net(), volume(BIG, seed)[0], *ARGS, fused=True, tta=tta)


def key(p):
    return tuple(sorted(p.items()))


@functools.lru_cache(None)
def referee(seed, pkey, tta=None):
    """(hard', labels', dropped) by the referee from the plain evaluation and its tail labels"""
    hard, soft = plain(seed, tta)
    labels = SF.brats_case_tail(soft, hard)[1]
    return ref_brats(hard, labels, check_every=8, **dict(pkey))


@pytest.mark.parametrize('p', [P_SMALL, P_DROP], ids=['small', 'drop'])
def test_single_case_equals_plain_then_referee(p):
    hard0, soft0 = plain(11)
    want, _, dropped = referee(11, key(p))
    hard, soft = infer3d.test_single_case(the_net(), volume(BIG, 11)[0], *ARGS, fused=True, postprocess=p)
    assert hard.dtype == torch.float32 and torch.equal(hard, want)
    assert torch.equal(soft, soft0)                                                   # preds_soft is returned unchanged
    print('postprocess %r: WT %d -> %d voxels, ET %d -> %d' % (p, int(hard0[2].sum()), int(hard[2].sum()), int(hard0[1].sum()), int(hard[1].sum())))
    assert hard0[1].any() and (p is P_SMALL or not torch.equal(hard, hard0))          # P_DROP changes any prediction that has ET
    assert dropped == (p is P_DROP) and bool(hard[1].any()) != dropped
    if p is P_DROP:
        _, sizes = infer3d.connected_components(hard[2], connectivity=6)
        assert int((sizes > 0).sum()) == 1
    eager = infer3d.test_single_case(the_net(), volume(BIG, 11)[0], *ARGS, fused=False, postprocess=p)      # the eager loop takes the argument too
    assert same(eager, (hard, soft))


def test_single_case_with_tta_equals_plain_then_referee():
    tta = ((), (0,))
    want, _, _ = referee(11, key(P_SMALL), tta)
    hard, soft = infer3d.test_single_case(the_net(), volume(BIG, 11)[0], *ARGS, fused=True, tta=tta, postprocess=P_SMALL)
    assert torch.equal(hard, want) and torch.equal(soft, plain(11, tta)[1])
    assert not torch.equal(soft, plain(11)[1])                                        # the views were on


def test_postprocess_none_is_bit_identical():
    net, (x, lab) = the_net(), volume(BIG, 11)
    assert same(infer3d.test_single_case(net, x, *ARGS, fused=True, postprocess=None), plain(11))
    g0 = infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, with_mask=True)
    try:
        a = [t.clone() for t in g0(x, lab)]
    finally:
        g0.close()
    g1 = infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, with_mask=True, postprocess=None)
    try:
        assert g1.flag is None and same(g1(x, lab), a)
    finally:
        g1.close()
    db = [dict(image=x.cpu(), mask=lab.cpu().long(), image_path='/data/case_0.nii.gz')]
    kw = dict(batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16)
    got0, got1 = [], []
    avg0 = infer3d.test_all_cases(net, db, on_labels=lambda n, v: got0.append(v), **kw)
    avg1 = infer3d.test_all_cases(net, db, on_labels=lambda n, v: got1.append(v), postprocess=None, **kw)
    assert np.array_equal(avg0, avg1, equal_nan=True) and torch.equal(got0[0], got1[0]) and torch.equal(got0[0], a[2])


def _gt(lab):
    mask = lab.long() - (lab == 4).long()
    return D3.brats_map_label(mask.unsqueeze(0).float(), False)[0]


def test_graph_replays_equal_the_eager_call():
    net = the_net()
    g = infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, with_mask=True, postprocess=P_DROP)
    try:
        seen = []
        for seed in (11, 13):                                   # the second replay: static inputs refreshed, static outputs (flag and counter included) rewritten
            x, lab = volume(BIG, seed)
            hard, soft, labels, counts = g(x, lab)
            want_hard, want_labels, _ = referee(seed, key(P_DROP))
            assert same((hard, soft), infer3d.test_single_case(net, x, *ARGS, fused=True, postprocess=P_DROP))
            assert torch.equal(hard, want_hard) and torch.equal(soft, plain(seed)[1]) and torch.equal(labels, want_labels)
            metric, valid = T3.calculate_metric_percase(hard, _gt(lab), 4)
            got_metric, got_valid = infer3d.case_metrics(counts)
            assert np.array_equal(got_metric[:, :2], metric[:, :2]) and np.array_equal(got_valid[:, :2], valid[:, :2])
            plain_counts = SF.brats_case_tail(*plain(seed)[::-1], lab, want_labels=False)[0]
            assert not torch.equal(counts, plain_counts)       # the counts see the post-processed prediction
            seen.append(hard.clone())
        assert not torch.equal(seen[0], seen[1]) and g.replays == 2
    finally:
        g.close()


@pytest.mark.parametrize('graph', [False, True])
def test_all_cases_equals_the_per_case_composition(graph):
    cases = [(BIG, 11), (BIG, 13)]
    db = [dict(image=volume(s, seed)[0].cpu(), mask=volume(s, seed)[1].cpu().long(), image_path='/data/brats/case_%d.nii.gz' % i)
          for i, (s, seed) in enumerate(cases)]
    total, valid_counts, exports = np.zeros((3, 4)), np.zeros((3, 4)), []
    for s, seed in cases:
        hard, labels, _ = referee(seed, key(P_DROP))
        metric, valid = T3.calculate_metric_percase(hard, _gt(volume(s, seed)[1]), 4)
        total += metric; valid_counts += valid
        exports.append(labels)
    got = []
    avg = infer3d.test_all_cases(the_net(), db, batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16,
                                 on_labels=lambda name, vol: got.append(vol), graph=graph, postprocess=P_DROP)
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.array_equal(avg, total / valid_counts, equal_nan=True)
    assert avg[0, 0] == 0 and (avg[1:, 0] > 0).all()                                  # ET was dropped in every case: its Dice is 0
    assert len(got) == 2 and all(torch.equal(v, w) for v, w in zip(got, exports))
    assert not any((v == 4).any() for v in got)


def test_postprocess_brats_with_satellites():
    """CONSTRUCTED preds_hard: the network's WT is cut to one compact blob and two satellites are pasted in, one of which holds ET; each satellite's fate is then known"""
    hard0, soft = plain(11)
    H, W, D = BIG
    hard = torch.zeros_like(hard0)
    hard[2, 20:80, 30:150, 2:14] = 1                                                  # the main WT blob, over many tile seams
    hard[3, 30:60, 50:100, 4:12] = 1
    g = torch.Generator(device='cpu').manual_seed(4)
    hard[1, 35:50, 60:90, 5:10] = (torch.rand(15, 30, 5, generator=g, device='cpu') < 0.5).float().to(DEV)      # ET: speckle inside the core
    hard[2, 100:104, 200:204, 0:4] = 1                                                # satellite A: 64 voxels of WT alone
    hard[2, 2:7, 2:7, 10:15] = 1; hard[1, 3:5, 3:5, 11:13] = 1; hard[3, 3:5, 3:5, 11:13] = 1    # satellite B: 125 voxels of WT, 8 of them ET and TC
    hard[0] = (hard[1:].sum(0) == 0).float()
    labels = SF.brats_case_tail(soft, hard)[1]
    n_et = int((hard[1] * hard[2]).sum())
    assert n_et > 100
    before = hard.clone()
    for p, wt_left, et_left in ((dict(wt_min_voxels=64), 3, n_et), (dict(wt_min_voxels=65), 2, n_et), (dict(wt_min_voxels=126), 1, n_et - 8),
                                (dict(wt_largest_only=True, et_min_voxels=n_et - 8), 1, n_et - 8), (dict(wt_largest_only=True, et_min_voxels=n_et - 7), 1, 0),
                                (dict(wt_min_voxels=65, et_min_voxels=n_et + 1, connectivity=6), 2, 0)):
        want, want_labels, _ = ref_brats(hard, labels, check_every=8, **p)
        got, got_labels = infer3d.postprocess_brats(hard, labels, **p)
        assert torch.equal(got, want) and torch.equal(got_labels, want_labels), p
        assert int((infer3d.connected_components(got[2])[1] > 0).sum()) == wt_left and int(got[1].sum()) == et_left, p
        assert torch.equal(got[0], (got[1:].sum(0) == 0).float()) and not got_labels[got[2] == 0].any()
        assert torch.equal(infer3d.postprocess_brats(hard, **p), want)
    assert torch.equal(hard, before)


def test_full_size_labelling():
    """240 x 240 x 155: 30 x 30 x 5 tiles, raster indices up to 8.9 million, against the referee on the device (blobs of 7^3 blocks at a density below the
    percolation threshold plus speckle, so the referee's propagation ends after a few dozen sweeps; it looks for its fixed point every 16th)"""
    g = torch.Generator(device='cpu').manual_seed(3)
    coarse = (torch.rand(35, 35, 23, generator=g, device='cpu') < 0.06).to(DEV)
    mask = coarse.repeat_interleave(7, 0).repeat_interleave(7, 1).repeat_interleave(7, 2)[:240, :240, :155]
    mask = (mask | (torch.rand(240, 240, 155, generator=g, device='cpu') < 0.002).to(DEV)).float().contiguous()
    for conn in (26, 6):
        labels, sizes = infer3d.connected_components(mask, connectivity=conn)
        want_labels, want_sizes = ref_labels3d(mask[None] != 0, conn, check_every=16)
        assert torch.equal(labels, want_labels[0]) and torch.equal(sizes, want_sizes[0])
    assert int(sizes.sum()) == int(mask.sum()) and int((sizes > 0).sum()) > 1000 and int(sizes.max()) > 343
    big = infer3d.remove_small_components(mask, largest_only=True, connectivity=6)
    assert int(big.sum()) == int(sizes.max()) and big.dtype == mask.dtype
