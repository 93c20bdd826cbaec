"""The tail of one BraTS case (metrics.hip: segx_brats_case_tail; SF.brats_case_tail, infer3d.case_metrics) on the fiber emulator (CPU) and on the GPU (-m gpu), against
the oracle's brats_map_label / brats_inv_map_label and torch on the CPU.  Integers and single rounded float operations: every comparison is for EQUALITY.

Sizes, with T = SEGX_CASE_TAIL_THREADS (a workgroup covers 4 T voxels per trip): 1 and 3 (one thread, a cut quad), 4 T - 1 / 4 T / 4 T + 1 (the last thread of a
workgroup cut, full, one voxel into a second workgroup), 8 T + 2 (two workgroups and a cut quad), and 4 T MAX_BLOCKS + 4 T + 4 (and one less), where the grid is capped and the first
workgroups take a second trip (GPU only: too slow for the emulator).  S % 4 != 0 puts planes 1..3 off 16-byte alignment: those sizes take the dword path, the others the 16-byte one."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import segtran_oracle as O
from segtran_amd import functional as SF
from segtran_amd import infer3d, segx
from segtran_amd import test_util3d as T3

T, MAXB = segx.SegxLib.CASE_TAIL_THREADS, segx.SegxLib.CASE_TAIL_MAX_BLOCKS
SIZES = [1, 3, 4 * T - 1, 4 * T, 4 * T + 1, 8 * T + 2]
S_SECOND_TRIP = 4 * T * MAXB + 4 * T + 4


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'segx.h')).read()
    assert int(re.search(r'#define SEGX_CASE_TAIL_THREADS (\d+)', hdr).group(1)) == T
    assert int(re.search(r'#define SEGX_CASE_TAIL_MAX_BLOCKS (\d+)', hdr).group(1)) == MAXB
    assert T % 64 == 0


@functools.lru_cache(None)
def case(S):
    """CPU tensors (soft [4, S], gt int32 [S]) and the referee's (counts int64 [3, 3], labels uint8 [S], number of voxels whose argmax is tied).  soft: uniform
    draws, the consistency rule (WT = max(ET, WT, TC), TC = max(ET, TC)), then rounded to multiples of 1/8 -- exact in float32, so ties between the inverse
    probabilities are frequent."""
    g = torch.Generator().manual_seed(1000 + S)
    soft = O.make_brats_pred_consistent(torch.rand(4, S, generator=g, device='cpu'), False)
    soft = torch.round(soft * 8) / 8
    gt = torch.randint(0, 6, (S,), generator=g, device='cpu').to(torch.int32)
    inv = O.brats_inv_map_label(soft)
    lab = torch.argmax(inv, dim=0)
    lab += (lab == 3).long()                                                      # test_util3d.py:84-85
    top = inv.sort(dim=0, descending=True)[0]
    ties = int((top[0] == top[1]).sum())
    return soft, gt, lab.to(torch.uint8), ties


def gt_nhot(gt):
    """reference test_util3d.py:36-38: 4 -> 3, then brats_map_label; [4, S] floats"""
    m = gt.cpu().long()
    m = m - (m == 4).long()
    with torch.device('cpu'):                                                     # the oracle allocates on the default device, which the backend fixture sets
        return O.brats_map_label(m.unsqueeze(0))[0]


def ref_counts(hard, gt):
    nh, pred = gt_nhot(gt), hard.cpu() != 0
    return torch.stack([torch.stack([(pred[c] & (nh[c] != 0)).sum(), pred[c].sum(), (nh[c] != 0).sum()]) for c in (1, 2, 3)]).to(torch.int32)


def on_device(b, S):
    soft, gt, lab, ties = case(S)
    soft_d, gt_d = soft.to(b.dev), gt.to(b.dev)
    hard_d = SF.harden_segmap(soft_d.unsqueeze(0), mode=1)[1][0]
    return soft_d, hard_d, gt_d, lab, ties


def check(b, S):
    soft, hard, gt, lab, ties = on_device(b, S)
    counts, labels = SF.brats_case_tail(soft, hard, gt)
    assert counts.dtype == torch.int32 and labels.dtype == torch.uint8 and tuple(labels.shape) == (S,)
    assert torch.equal(labels.cpu(), lab)
    assert torch.equal(counts.cpu(), ref_counts(hard, gt))
    return ties


@pytest.mark.parametrize('S', SIZES)
def test_counts_and_labels_equal_the_referee(backend, S):
    check(backend, S)


def test_the_referee_sees_ties_and_every_label():
    """the inputs of the size tests: argmax ties occur (the lowest-index rule is exercised), every export label 0, 1, 2, 4 occurs, and the ground truth holds the raw 4
    and the out-of-range 5"""
    soft, gt, lab, ties = case(8 * T + 2)
    assert ties > 50
    assert sorted(lab.unique().tolist()) == [0, 1, 2, 4]
    assert sorted(gt.unique().tolist()) == [0, 1, 2, 3, 4, 5]
    nh = gt_nhot(gt)
    assert torch.equal(nh[1] != 0, (gt == 3) | (gt == 4)) and not nh[:, gt == 5].any()


@pytest.mark.gpu
@pytest.mark.parametrize('S', [S_SECOND_TRIP, S_SECOND_TRIP - 1])
def test_second_trip_of_the_grid_stride_loop(S):
    """S above 4 T MAX_BLOCKS: the grid is capped and the loop runs again in the first workgroups; on the 16-byte path and, one voxel shorter, on the dword path.
    GPU only: about 2.1 M voxels take 35 s per case on the fiber emulator (measured), and the loop's stride arithmetic is the one the small sizes run."""
    segx.use_library(None)
    assert check(types.SimpleNamespace(dev=torch.device('cuda', 0)), S) > 0


def test_volume_shape_and_integer_ground_truth_dtypes(backend):
    """[4, H, W, D] operands and an int64 / uint8 ground truth (converted to int32)"""
    H, W, D = 5, 6, 7
    soft, hard, gt, lab, _ = on_device(backend, H * W * D)
    want = ref_counts(hard, gt)
    for dtype in (torch.int64, torch.uint8, torch.int32):
        counts, labels = SF.brats_case_tail(soft.view(4, H, W, D), hard.view(4, H, W, D), gt.view(H, W, D).to(dtype))
        assert tuple(labels.shape) == (H, W, D) and torch.equal(labels.cpu().view(-1), lab) and torch.equal(counts.cpu(), want)


@pytest.mark.parametrize('S', [4 * T + 1, 8 * T])
def test_labels_only_and_counts_only(backend, S):
    soft, hard, gt, lab, _ = on_device(backend, S)
    counts, labels = SF.brats_case_tail(soft, hard)
    assert counts is None and torch.equal(labels.cpu(), lab)
    counts, labels = SF.brats_case_tail(soft, hard, gt, want_labels=False)
    assert labels is None and torch.equal(counts.cpu(), ref_counts(hard, gt))


def test_counts_are_initialised_by_every_call(backend):
    """a second call into the same buffers, with other data: nothing of the first call is left"""
    S = 8 * T + 2
    soft, hard, gt, lab, _ = on_device(backend, S)
    counts = torch.full((3, 3), 12345, dtype=torch.int32)
    labels = torch.full((S,), 9, dtype=torch.uint8)
    c, l = SF.brats_case_tail(soft, hard, gt, counts=counts, labels=labels)
    assert c is counts and l is labels
    assert torch.equal(counts.cpu(), ref_counts(hard, gt)) and torch.equal(labels.cpu(), lab)
    gt2 = (5 - gt).to(torch.int32)
    SF.brats_case_tail(soft, hard, gt2, counts=counts, labels=labels)
    assert torch.equal(counts.cpu(), ref_counts(hard, gt2)) and torch.equal(labels.cpu(), lab)
    empty = torch.zeros_like(hard)
    SF.brats_case_tail(soft, empty, torch.zeros_like(gt), counts=counts, want_labels=False)
    assert not counts.any()


def test_refusals(backend):
    L = backend.L
    S = 8
    soft, hard, gt, _, _ = on_device(backend, S)
    counts, labels = torch.zeros(3, 3, dtype=torch.int32), torch.zeros(S, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='null soft or hard'):
        L.brats_case_tail(None, hard, gt, counts, labels, S)
    with pytest.raises(RuntimeError, match='null soft or hard'):
        L.brats_case_tail(soft, None, gt, counts, labels, S)
    with pytest.raises(RuntimeError, match='neither counts nor labels'):
        L.brats_case_tail(soft, hard, gt, None, None, S)
    with pytest.raises(RuntimeError, match='counts need the ground truth'):
        L.brats_case_tail(soft, hard, None, counts, labels, S)
    for bad in (0, -4, 1 << 31):
        with pytest.raises(RuntimeError, match='is not in 1'):
            L.brats_case_tail(soft, hard, gt, counts, labels, bad)
    # the wrapper's own
    with pytest.raises(ValueError, match='one shape'):
        SF.brats_case_tail(soft[:3], hard[:3], gt)
    with pytest.raises(ValueError, match='one shape'):
        SF.brats_case_tail(soft, hard[:, :4], gt)
    with pytest.raises(ValueError, match='is not the volume'):
        SF.brats_case_tail(soft, hard, gt[:4])
    with pytest.raises(ValueError, match='counts need gt'):
        SF.brats_case_tail(soft, hard, None, counts=counts)
    with pytest.raises(ValueError, match='nothing to compute'):
        SF.brats_case_tail(soft, hard, None, want_labels=False)
    with pytest.raises(ValueError, match='int32 \\[3, 3\\]'):
        SF.brats_case_tail(soft, hard, gt, counts=torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError, match='uint8'):
        SF.brats_case_tail(soft, hard, gt, labels=torch.zeros(S, dtype=torch.int32))


@pytest.mark.parametrize('kind', ['random', 'empty-gt-class', 'empty-everything'])
def test_case_metrics_equal_calculate_metric_percase(backend, kind):
    S = 8 * T + 2
    soft, hard, gt, _, _ = on_device(backend, S)
    if kind == 'empty-gt-class':
        gt = torch.where((gt == 3) | (gt == 4), 2, gt).to(torch.int32)          # no ET voxel: Jaccard of class 1 is invalid
    elif kind == 'empty-everything':
        gt, hard = torch.zeros_like(gt), torch.zeros_like(hard)                  # p + g == 0: Dice 0
    counts, _ = SF.brats_case_tail(soft, hard, gt, want_labels=False)
    metric, valid = infer3d.case_metrics(counts)
    want_metric, want_valid = T3.calculate_metric_percase(hard, gt_nhot(gt).to(backend.dev), 4)
    assert metric.dtype == np.float64 and metric.shape == (3, 4) and valid.shape == (3, 4)
    assert np.array_equal(metric, want_metric) and np.array_equal(valid, want_valid)
    if kind == 'random':
        assert (metric[:, :2] > 0).all() and (valid[:, :2] == 1).all() and not valid[:, 2:].any()
    elif kind == 'empty-gt-class':
        assert valid[0, 1] == 0 and valid[1, 1] == 1
    else:
        assert not metric.any() and not valid[:, 1:].any() and valid[:, 0].all()
