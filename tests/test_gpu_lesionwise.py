"""GPU (-m gpu): the lesion-wise evaluation inside the 3-D case evaluation -- the `lesionwise=` argument of infer3d.test_all_cases and
infer3d.GraphedSlidingWindow3d -- against the torch referee (tests/lesionwise_referee.py, running on the device) applied to the preds_hard the same evaluation
produces, integer for integer and with an identical float64 lesion_dice; and one device-only case whose counters receive adds from many workgroups.  The model and
the volumes are those of tests/test_gpu_sliding3d.py (cfg4 at (112, 112, 16) on a 120 x 224 x 16 volume)."""
import functools

import numpy as np
import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer3d
from segtran_amd.dataloaders import datasets3d as D3
from lesionwise_referee import ref_lesionwise
from test_gpu_sliding3d import BIG, PATCH, the_net, volume

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ARGS = (PATCH, PATCH, 2, 56, 16, 'brats')
LW = dict(dilation_iters=2, dilation_connectivity=18, connectivity=26, min_lesion_voxels=20)
POST = dict(wt_largest_only=True, et_min_voxels=1 << 30, connectivity=6)         # ET can never reach the threshold: the rule drops it
KEYS = ('n_fp', 'fp_voxels', 'n_detected', 'n_missed', 'lesion_dice')
SEEDS = (11, 13)


def gt_regions(lab):
    """float [3, H, W, D]: the ET, WT, TC maps of brats_map_label for the raw labels with 4 -> 3"""
    mask = lab.long() - (lab == 4).long()
    return D3.brats_map_label(mask.unsqueeze(0).float(), False)[0][1:4]


@functools.lru_cache(None)
def prediction(seed, post):
    return infer3d.test_single_case(the_net(), volume(BIG, seed)[0], *ARGS, fused=True, postprocess=POST if post else None)[0]


@functools.lru_cache(None)
def referee(seed, post, mask_seed=None):
    """the referee's dicts for the evaluation's own preds_hard against the mask of mask_seed (default: the case's own)"""
    lab = volume(BIG, seed if mask_seed is None else mask_seed)[1]
    return ref_lesionwise(prediction(seed, post)[1:4], gt_regions(lab), check_every=8, **LW)


def assert_same(got, want):
    assert len(got) == len(want) == 3
    for r, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a['lesions'], b['lesions']) and np.array_equal(a['kept'], b['kept']), r
        for k in KEYS:
            assert a[k] == b[k], (r, k, a[k], b[k])


def database():
    return [dict(image=volume(BIG, seed)[0].cpu(), mask=volume(BIG, seed)[1].cpu().long(), image_path='/data/brats/case_%d.nii.gz' % i) for i, seed in enumerate(SEEDS)]


@pytest.mark.parametrize('post', [False, True], ids=['plain', 'postprocess'])
@pytest.mark.parametrize('graph', [False, True], ids=['fused', 'graph'])
def test_all_cases_equals_the_referee_on_its_own_prediction(graph, post):
    kw = dict(batch_size=2, orig_patch_size=PATCH, input_patch_size=PATCH, stride_xy=56, stride_z=16, graph=graph, postprocess=POST if post else None)
    avg, lw = infer3d.test_all_cases(the_net(), database(), lesionwise=LW, **kw)
    want = [referee(seed, post) for seed in SEEDS]
    assert len(lw['cases']) == len(SEEDS)
    for got, w in zip(lw['cases'], want):
        assert_same(got, w)
    mean = np.array([[c[r]['lesion_dice'] for r in range(3)] for c in want]).mean(0)
    assert lw['mean_lesion_dice'].dtype == np.float64 and np.array_equal(lw['mean_lesion_dice'], mean)
    print('lesion-wise (graph %r, postprocess %r): lesions %r, components %r, n_fp %r, mean lesion Dice %r'
          % (graph, post, [[len(r['lesions']) for r in c] for c in want], [[r['n_pred'] for r in c] for c in want], [[r['n_fp'] for r in c] for c in want], mean.tolist()))
    assert any(len(r['lesions']) for c in want for r in c) and any(r['n_detected'] for c in want for r in c)
    if post:                                                                        # the rows see the post-processed prediction: no ET component is left
        assert all(c[0]['n_pred'] == 0 and c[0]['n_detected'] == 0 and c[0]['lesion_dice'] == 0.0 for c in want)
        assert all(referee(seed, False)[0]['n_detected'] == 1 for seed in SEEDS)
    plain = infer3d.test_all_cases(the_net(), database(), **kw)                     # avg_metric does not change with the argument, bit for bit
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, avg, equal_nan=True)


def test_graph_replays_give_each_mask_its_own_tables():
    """one image, two masks: the static workspace, tables and labellings are rebuilt inside every replay"""
    net = the_net()
    with pytest.raises(ValueError, match='with_mask'):
        infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, lesionwise=LW)
    g = infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, with_mask=True, lesionwise=LW)
    try:
        x = volume(BIG, 11)[0]
        seen = []
        for mask_seed in (11, 13, 11):
            out = g(x, volume(BIG, mask_seed)[1])
            assert len(out) == 4 and torch.equal(out[0], prediction(11, False))
            got = infer3d.lesionwise_from_tables(g.lesion_rows, g.lesion_header, LW['min_lesion_voxels'])
            assert_same(got, referee(11, False, mask_seed))
            seen.append(g.lesion_rows.clone())
        assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])
    finally:
        g.close()
    assert g.lesion_rows is None and g.lesion_header is None
    g0 = infer3d.GraphedSlidingWindow3d(net, (4,) + BIG, PATCH, PATCH, 2, 56, 16, fold_bn=False, with_mask=True, lesionwise=None)
    try:
        assert g0.lesion_rows is None and g0.lesion_header is None and g0.lw is None          # the default allocates nothing new
    finally:
        g0.close()


def test_random_blobs_over_many_workgroups():
    """64 x 64 x 96, three regions: lesions and components of thousands of voxels each, so every counter receives adds from many workgroups"""
    g = torch.Generator(device='cpu').manual_seed(7)

    def field(density, speckle):
        coarse = (torch.rand(3, 11, 11, 16, generator=g, device='cpu') < density)
        m = coarse.repeat_interleave(6, 1).repeat_interleave(6, 2).repeat_interleave(6, 3)[:, :64, :64, :96]
        return (m | (torch.rand(3, 64, 64, 96, generator=g, device='cpu') < speckle)).to(DEV)
    gt, pred = field(0.05, 0.0005), field(0.06, 0.002)
    pred = pred | (gt & field(0.5, 0.0))
    for kw in (dict(dilation_iters=1), dict(dilation_iters=3, dilation_connectivity=26, connectivity=6, min_lesion_voxels=10)):
        want = ref_lesionwise(pred, gt, check_every=8, **kw)
        got = infer3d.lesionwise_metrics(pred.float(), gt.to(torch.uint8), **kw)
        assert_same(got, want)
        rows, header = SF.lesion_rows(pred, gt, **{k: v for k, v in kw.items() if k != 'min_lesion_voxels'})
        assert header[:, :5].cpu().tolist() == [[len(w['lesions']), w['n_pred'], w['n_fp'], w['fp_voxels'], 0] for w in want]
        assert all(len(w['lesions']) > 3 and w['n_fp'] > 3 and w['n_detected'] > 1 and int(w['lesions'][:, 2].max()) >= 216 for w in want)        # a 6^3 block: 36 rows of z
