"""3-D evaluation with a `precision` switch: test_util3d's sliding-window inference, optionally under the three-term bf16 product.

test_util3d.py mirrors the reference's file of that name and keeps the reference's signatures; the switch lives here, as infer2d.py holds the 2-D one.  The 3-D
convolutions of Inception-I3D (conv3d.hip, conv3d_halo.hip) and the GEMMs of the bf16 tile engine follow the precision selector inside the block; the loop, the
accumulation and the hardening are test_util3d's own.

It also holds the surface-distance half of calculate_metric_percase (reference test_util3d.py:203-213: medpy's asd, and the hd95 of the commented-out line), computed on
the device in integers (metrics.hip) and finished here in float64; test_util3d.calculate_metric_percase keeps reporting those columns as invalid.

And the case evaluation in one pass: sliding_windows (the eager loops' geometry and batches), test_single_case(fused=True) (one gather launch, net() on the
eager loop's batches, one merge launch), GraphedSlidingWindow3d (that sequence with the BraTS case tail, SF.brats_case_tail, as one replayable hipGraph), case_metrics
and test_all_cases (the reference's loop over the cases of a dataset, test_util3d.py:15-91, without its file I/O).

And the step a BraTS user runs on the prediction: connected_components, remove_small_components and postprocess_brats on the device, and the
`postprocess=` argument that places the rule between the merge and the case tail of test_single_case, GraphedSlidingWindow3d and test_all_cases.

And the lesion-wise evaluation: lesionwise_metrics / lesionwise_from_tables (per-lesion Dice, detections and false positives from device tables) and the
`lesionwise=` argument of GraphedSlidingWindow3d and test_all_cases."""
import math
import os

import numpy as np
import torch

from . import functional as SF
from . import test_util3d as _T3
from .segx import SegxLib
from .infer_common import PRECISIONS, GraphedEvaluation, _precision, composed_tta, folded, inference_precision, run_chunks, view_chunks      # noqa: F401  (inference_precision: re-exported)


def fold_batchnorm(net):
    """Inference: fold the BatchNorm3d layers of a Segtran3d's I3D backbone into its convolutions (InceptionI3d.fold_batchnorm; eval mode only); returns net.  The 3-D
    entry point has its own name because Segtran3d.fold_batchnorm() keeps refusing."""
    net.backbone.fold_batchnorm()
    return net


def unfold_batchnorm(net):
    net.backbone.unfold_batchnorm()
    return net


def _folded(net, fold_bn):
    """fold for the block if asked and not folded already (fold_batchnorm: the backbone's); a net the caller folded stays folded"""
    return folded(net, fold_bn, fold_batchnorm, unfold_batchnorm)


def sliding_windows(H, W, D, orig_patch_size, stride_xy, stride_z, batch_size):
    """The window geometry of test_util3d.test_single_case for an H x W x D volume: ((xl, yl, zl), (H2, W2, D2), origins, chunks) -- the left pads, the padded extent,
    the (xs, ys, zs) origin of every window in padded coordinates in the eager loops' order (x outer, then y, z innermost; the last origin of an axis clamped to
    extent - window), and the eager loop's grouping of them into net() calls as (first, end) index ranges into `origins`: within an x row its sy * sz windows in runs
    of batch_size, the row's last run shorter if need be -- the eager loop flushes at the end of every x row, so no chunk crosses one.  A stride that is not
    positive, or above its window extent (cells no window covers), raises ValueError, as infer2d.sliding_windows does."""
    dx, dy, dz = (int(v) for v in orig_patch_size)
    sxy, sz_, bs = int(stride_xy), int(stride_z), int(batch_size)
    if sxy <= 0 or sz_ <= 0 or sxy > min(dx, dy) or sz_ > dz:
        raise ValueError('sliding_windows: strides (%r, %r) must be positive and at most the window %r' % (stride_xy, stride_z, tuple(orig_patch_size)))
    if bs < 1:
        raise ValueError('sliding_windows: batch_size must be at least 1')
    pads = [max(dx - H, 0), max(dy - W, 0), max(dz - D, 0)]
    H2, W2, D2 = H + pads[0], W + pads[1], D + pads[2]
    nx = math.ceil((H2 - dx) / sxy) + 1
    ny = math.ceil((W2 - dy) / sxy) + 1
    nz = math.ceil((D2 - dz) / sz_) + 1
    origins = [(min(sxy * x, H2 - dx), min(sxy * y, W2 - dy), min(sz_ * z, D2 - dz)) for x in range(nx) for y in range(ny) for z in range(nz)]
    row = ny * nz
    chunks = [(x * row + k, x * row + min(k + bs, row)) for x in range(nx) for k in range(0, row, bs)]
    return tuple(p // 2 for p in pads), (H2, W2, D2), origins, chunks


class _Plan3d:
    """what the fused 3-D sequence needs beyond the image: the window table on the device, the geometry and the eager loop's chunks"""

    def __init__(self, image_shape, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, device, tta=None):
        self.shape = tuple(int(v) for v in image_shape)
        self.views = None if tta is None else SF.ViewTable(tta, 3, device)          # refuses a bad tta before anything is launched
        if len(self.shape) != 4:
            raise ValueError('a [C, H, W, D] image, not %r' % (self.shape,))
        self.window, self.patch = tuple(int(v) for v in orig_patch_size), tuple(int(v) for v in input_patch_size)
        self.pads, self.canvas, origins, self.chunks = sliding_windows(*self.shape[1:], self.window, stride_xy, stride_z, batch_size)
        self.table = SF.WindowTable(origins, device)
        if self.views is not None:                                                  # every view runs the eager loop's chunks, view after view
            self.chunks = view_chunks(self.chunks, self.table.nwin, self.views.V)

    def run(self, net, image):
        """gather -> net() per chunk of the eager loop -> merge; the caller holds torch.no_grad().  (preds_hard, preds_soft) [num_classes, H, W, D]"""
        patches = SF.window_gather(image.unsqueeze(0), self.table, self.window, self.patch, self.pads, self.canvas, views=self.views)
        scores = run_chunks(net, patches, self.chunks)
        preds_soft, preds_hard = SF.window_merge(scores, self.table, self.window, self.shape[1:], self.pads, self.canvas, mode=1, views=self.views)
        return preds_hard[0], preds_soft[0]


# ---- connected-component post-processing ----------------------------------------------------------------------------------------------------
POSTPROCESS_KEYS = ('wt_min_voxels', 'wt_largest_only', 'et_min_voxels', 'connectivity')


def _device_operand(what, t):
    if not isinstance(t, torch.Tensor) or t.device.type == 'cpu':
        raise ValueError('%s: a device tensor, not %s' % (what, 'a host tensor' if isinstance(t, torch.Tensor) else type(t).__name__))


def check_postprocess(postprocess, num_classes=4):
    """the `postprocess` argument of the evaluation entry points: None, or a dict of postprocess_brats' keyword arguments made complete and checked -- ValueError on an
    unknown key, a connectivity other than 6 / 26, a negative threshold or num_classes != 4, before anything is launched"""
    if postprocess is None:
        return None
    if not isinstance(postprocess, dict):
        raise ValueError('postprocess: None or a dict of %s, not %r' % (POSTPROCESS_KEYS, postprocess))
    unknown = sorted(set(postprocess) - set(POSTPROCESS_KEYS))
    if unknown:
        raise ValueError('postprocess: unknown keys %s (known: %s)' % (unknown, POSTPROCESS_KEYS))
    if num_classes != 4:
        raise ValueError('postprocess: the BraTS rule needs num_classes == 4, not %r' % (num_classes,))
    p = dict(wt_min_voxels=0, wt_largest_only=False, et_min_voxels=0, connectivity=26)
    p.update(postprocess)
    p['connectivity'] = SF.check_connectivity3d('postprocess', p['connectivity'])
    for k in ('wt_min_voxels', 'et_min_voxels'):
        p[k] = SF.check_voxel_count('postprocess', k, p[k])
    p['wt_largest_only'] = bool(p['wt_largest_only'])
    return p


def connected_components(mask, connectivity=26):
    """(labels, sizes) int32 of the 6- or 26-connected components of a device mask [X, Y, Z] or a stack [V, X, Y, Z] (bool, uint8 or float; set = not 0), on the
    device (SF.label_components3d): labels = 0 on the background, else 1 + the raster index inside its volume of the component's first voxel; sizes = the
    component's voxel count at that first voxel, 0 elsewhere.  ValueError for a connectivity other than 6 / 26 or a host tensor, before anything is launched."""
    SF.check_connectivity3d('connected_components', connectivity)
    _device_operand('connected_components', mask)
    with torch.no_grad():
        return SF.label_components3d(mask, connectivity)


def remove_small_components(mask, min_voxels=0, largest_only=False, connectivity=26):
    """A NEW tensor of mask's shape, dtype and device (as infer2d.remove_fragmentary_segs returns one) that holds only the components of at least min_voxels voxels
    and, with largest_only, of those only the largest of each volume (ties: the one that starts first in raster order).  A volume without foreground stays empty."""
    SF.check_connectivity3d('remove_small_components', connectivity)
    SF.check_voxel_count('remove_small_components', 'min_voxels', min_voxels)
    _device_operand('remove_small_components', mask)
    with torch.no_grad():
        return SF.remove_small_components3d(mask, min_voxels, largest_only, connectivity)


def postprocess_brats(preds_hard, labels=None, *, wt_min_voxels=0, wt_largest_only=False, et_min_voxels=0, connectivity=26):
    """The usual BraTS post-processing (Isensee et al., "No New-Net", 2018) of preds_hard [4, H, W, D] (background, ET, WT, TC) on the device (SF.brats_postprocess):
    WT loses its components below wt_min_voxels (with wt_largest_only: all but the largest), ET and TC are cut to what is left of WT, ET is dropped when fewer than
    et_min_voxels voxels remain, the background is recomputed.  Returns preds_hard' (a new tensor), and (preds_hard', labels') when the export label volume `labels`
    (uint8 [H, W, D], SF.brats_case_tail's) is given: 0 outside WT', a 4 turned into 1 where ET was dropped.  The inputs are not modified."""
    p = check_postprocess(dict(wt_min_voxels=wt_min_voxels, wt_largest_only=wt_largest_only, et_min_voxels=et_min_voxels, connectivity=connectivity),
                          preds_hard.shape[0] if isinstance(preds_hard, torch.Tensor) and preds_hard.dim() == 4 else None)
    _device_operand('postprocess_brats', preds_hard)
    if labels is not None:
        _device_operand('postprocess_brats', labels)
    with torch.no_grad():
        hard, flag = SF.brats_postprocess(preds_hard, **p)
        return hard if labels is None else (hard, SF.brats_relabel(labels, hard, flag))


# ---- lesion-wise evaluation -----------------------------------------------------------------------------------------------------------------
LESIONWISE_KEYS = ('dilation_iters', 'dilation_connectivity', 'connectivity', 'min_lesion_voxels')


def check_lesionwise(lesionwise, num_classes=4):
    """the `lesionwise` argument of the evaluation entry points: None, or a dict of lesionwise_metrics' keyword arguments made complete and checked -- ValueError on an
    unknown key, a negative dilation_iters, a dilation connectivity other than 6 / 18 / 26, a labelling connectivity other than 6 / 26, a negative
    min_lesion_voxels or num_classes != 4, before anything is launched"""
    if lesionwise is None:
        return None
    if not isinstance(lesionwise, dict):
        raise ValueError('lesionwise: None or a dict of %s, not %r' % (LESIONWISE_KEYS, lesionwise))
    unknown = sorted(set(lesionwise) - set(LESIONWISE_KEYS))
    if unknown:
        raise ValueError('lesionwise: unknown keys %s (known: %s)' % (unknown, LESIONWISE_KEYS))
    if num_classes != 4:
        raise ValueError('lesionwise: the BraTS regions need num_classes == 4, not %r' % (num_classes,))
    p = dict(dilation_iters=3, dilation_connectivity=18, connectivity=26, min_lesion_voxels=0)
    p.update(lesionwise)
    p['dilation_iters'], p['dilation_connectivity'] = SF.check_dilation('lesionwise', p['dilation_iters'], p['dilation_connectivity'])
    p['connectivity'] = SF.check_connectivity3d('lesionwise', p['connectivity'])
    p['min_lesion_voxels'] = SF.check_voxel_count('lesionwise', 'min_lesion_voxels', p['min_lesion_voxels'])
    return p


def _kernel_args(lw):
    return {k: v for k, v in lw.items() if k != 'min_lesion_voxels'}


def lesionwise_from_tables(rows, header, min_lesion_voxels=0):
    """The host half of lesionwise_metrics: rows [R, LESION_MAX_GT, 4] and header [R, LESION_HEADER] (SF.lesion_rows' tables, tensors or arrays, already read or
    not) -> a list of R dicts.  'lesions': int64 [n, 4] rows (root label, tp, gvol, pvol) of ALL lesions sorted by root label; 'kept': bool [n], gvol >=
    min_lesion_voxels; 'n_fp', 'fp_voxels': the predicted components that touch no lesion (an ignored lesion still counts as touched) and their voxels;
    'n_detected', 'n_missed': kept lesions with and without tp > 0; 'lesion_dice': float64, the sum over the kept lesions (in the order of their root labels) of
    2 tp / (gvol + pvol), divided by (kept lesions + n_fp), 1.0 when that is 0.  RuntimeError when a region exceeded a cap of the device tables (there is no slow
    path)."""
    nmin = SF.check_voxel_count('lesionwise_from_tables', 'min_lesion_voxels', min_lesion_voxels)
    rows = (rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)).astype(np.int64)
    header = (header.cpu().numpy() if isinstance(header, torch.Tensor) else np.asarray(header)).astype(np.int64)
    if rows.ndim != 3 or rows.shape[2] != 4 or header.ndim != 2 or header.shape[0] != rows.shape[0] or header.shape[1] < 5:
        raise ValueError('lesionwise_from_tables: rows [R, MAX_GT, 4] and header [R, >= 5], not %r and %r' % (rows.shape, header.shape))
    out = []
    for r in range(rows.shape[0]):
        n_all, n_pred, n_fp, fp_voxels, overflow = (int(v) for v in header[r, :5])
        if overflow or n_all > rows.shape[1]:
            raise RuntimeError('lesion-wise evaluation: region %d holds %d lesions and %d predicted components, more than the device tables take (%d and %d)'
                               % (r, n_all, n_pred, rows.shape[1], SegxLib.LESION_MAX_PRED))
        les = rows[r, :n_all]
        les = les[np.argsort(les[:, 0], kind='stable')]
        kept = les[:, 2] >= nmin
        total = 0.0
        for _, tp, gvol, pvol in les[kept].tolist():
            total += 2.0 * tp / (gvol + pvol)
        n = int(kept.sum())
        detected = int((les[kept][:, 1] > 0).sum())
        out.append(dict(lesions=les, kept=kept, n_fp=n_fp, fp_voxels=fp_voxels, n_detected=detected, n_missed=n - detected,
                        lesion_dice=total / (n + n_fp) if n + n_fp > 0 else 1.0))
    return out


def lesionwise_metrics(pred, gt, *, dilation_iters=3, dilation_connectivity=18, connectivity=26, min_lesion_voxels=0):
    """Lesion-wise Dice and detection counts (the per-lesion scoring BraTS uses since 2023; DESIGN.md 5zb defines it) of two stacks of binary device volumes
    [R, X, Y, Z], or one volume [X, Y, Z] (bool, uint8 or float; set = not 0).  The ground truth is dilated dilation_iters times by the 3 x 3 x 3 element of
    dilation_connectivity neighbours; a lesion is the ground truth inside one `connectivity`-connected component of the dilated map; a predicted component that
    shares a voxel with that component touches the lesion.  Everything up to the integer rows runs on the device (SF.lesion_rows); ONE device-to-host copy brings them,
    and lesionwise_from_tables forms the quotients in float64.  Returns its list of R dicts."""
    lw = check_lesionwise(dict(dilation_iters=dilation_iters, dilation_connectivity=dilation_connectivity, connectivity=connectivity,
                               min_lesion_voxels=min_lesion_voxels))
    _device_operand('lesionwise_metrics', pred)
    _device_operand('lesionwise_metrics', gt)
    with torch.no_grad():
        rows, header = SF.lesion_rows(pred, gt, **_kernel_args(lw))
        both = torch.cat([rows.view(rows.shape[0], -1), header], 1).cpu().numpy()         # the one device-to-host copy
    return lesionwise_from_tables(both[:, :rows.shape[1] * 4].reshape(rows.shape), both[:, rows.shape[1] * 4:], lw['min_lesion_voxels'])


def _check_task(net_type, task_name):
    """the refusals of test_util3d.test_single_case"""
    if net_type != 'segtran':
        raise NotImplementedError("net_type '%s': only segtran is built" % net_type)
    if task_name != 'brats':
        raise NotImplementedError('only the BraTS (n-hot, consistency rule) hardening is built; argmax tasks are not in BASELINE')


def test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type='segtran', num_classes=4,
                     precision='fp32', fold_bn=False, fused=False, tta=None, postprocess=None):
    """test_util3d.test_single_case with five more arguments.  precision: 'fp32' (default) -- exactly that function's results -- or 'bf16x3' -- the same loop under
    torch.no_grad() inside inference_precision('bf16x3'); the setting the process had comes back at the end, also after an exception.  Any other name: ValueError.
    fold_bn: with the backbone's BatchNorm3d layers folded into its convolutions for this call (fold_batchnorm; a net the caller folded stays folded).
    fused: one window_gather launch on the image (the padded canvas never exists), net() once per chunk of sliding_windows() -- exactly the samples the eager loop
    stacks, so the forwards see the eager shapes --, the scores side by side in one buffer, one window_merge launch (no acc / cnt canvas, no accumulate pass per
    window, no clone of the un-padded region).  The merge is the accumulate + harden arithmetic bit for bit, so (preds_hard, preds_soft) equal the eager ones
    bit for bit for every batch_size.  The gather and the score buffer hold ALL windows at once: for a BraTS case (240 x 240 x 155, window 112 x 112 x 96 at
    stride 56 / 48: 48 windows x 4 channels x 112 x 112 x 96 floats) about 0.93 GB each.
    tta: None (default: exactly the call without it) or a sequence of up to 8 views for flip test-time augmentation.  A view is a tuple of distinct
    image axes to flip, 0 = H, 1 = W, 2 = D -- e.g. ((), (0,)); the identity () has to be listed to be used.  With soft_v = this call's preds_soft (the consistent
    map) for the image flipped along view v's axes, flipped back, preds_soft = (((soft_0 + soft_1) + soft_2) + ...) / float(V) in fp32 made consistent again, and
    preds_hard its hardening (SF.harden_segmap(mean, mode=1)).  fused=False runs that as a host loop (infer_common.composed_tta); fused=True runs one gather launch
    for all views, the chunks of sliding_windows() for each view in turn and one merge launch, and equals the host loop bit for bit for every batch_size.  The
    gather and the score buffer hold V times the figure above.  A bad tta raises ValueError before anything is launched.
    postprocess: None (default: exactly the call without it) or a dict of postprocess_brats' keyword arguments: preds_hard is what that function makes of the
    merged prediction (on the device); preds_soft is returned unchanged.  A bad dict raises ValueError before anything is launched."""
    views = None if tta is None else SF.check_views(tta, 3)
    post = check_postprocess(postprocess, num_classes)
    with _precision(precision), _folded(net, fold_bn):
        if not fused:
            def eager(x):
                return _T3.test_single_case(net, x, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type=net_type,
                                            num_classes=num_classes)
            hard, soft = eager(image) if views is None else composed_tta(eager, image, views, 1, 1)
        else:
            _check_task(net_type, task_name)
            plan = _Plan3d(image.shape, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, image.device, views)
            with torch.no_grad():
                hard, soft = plan.run(net, image)
        if post is not None:
            with torch.no_grad():
                hard = SF.brats_postprocess(hard, **post)[0]
        return hard, soft


# reference function name; not a pytest test
test_single_case.__test__ = False


def _percentile95(counts, roots):
    """numpy.percentile(x, 95) (linear interpolation between order statistics) of the multiset holding roots[k] counts[k] times; counts is not all zero"""
    n = int(counts.sum())
    virt = (n - 1) * 0.95
    lo = int(np.floor(virt))
    hi = min(lo + 1, n - 1)
    t = virt - lo
    cum = np.cumsum(counts)
    a, b = roots[np.searchsorted(cum, lo, side='right')], roots[np.searchsorted(cum, hi, side='right')]     # order statistic i = the first k with cum[k] > i
    return b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t                                           # numpy's _lerp


def surface_metrics(pred, gt, hd95=False):
    """medpy.metric.binary.asd(pred[p], gt[p]) -- and, with hd95=True, medpy.metric.binary.hd95(pred[p], gt[p]) -- for every plane p of two stacks of binary volumes
    [P, D, H, W] (set = not 0), unit voxel spacing, connectivity 1.  With border(m) = m XOR erode(m) (face neighbours, outside = unset) and dt = the Euclidean distance of
    every voxel to border(gt): asd = mean(dt[border(pred)]) -- ONE direction, prediction surface to ground-truth surface, not the symmetric assd --, hd95 =
    numpy.percentile of the distances of both directions together.  The device builds the borders, the exact int32 squared distance fields and their histograms on
    the borders (SF.surface_border, SF.edt_sq, SF.surface_hist); one device-to-host copy brings the counts, and the mean / percentile over sqrt(k) are taken here in
    float64.  hd95=True transforms the prediction borders as well (twice the device work).
    Returns float64 numpy arrays (asd [P], hd [P], valid [P]): valid[p] = 0 and both metrics 0 where either map is empty, as the reference reports them; hd = 0
    without hd95."""
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError('surface_metrics: pred %s and gt %s must be [P, D, H, W] tensors of one shape' % (tuple(pred.shape), tuple(gt.shape)))
    with torch.no_grad():
        bp, bg = SF.surface_border(pred), SF.surface_border(gt)
        hists = [SF.surface_hist(bp, SF.edt_sq(bg))]
        if hd95:
            hists.append(SF.surface_hist(bg, SF.edt_sq(bp)))
        counts = torch.stack(hists).cpu().numpy().astype(np.int64)             # [directions, P, nbins]: the one device-to-host copy
    P = pred.shape[0]
    roots = np.sqrt(np.arange(counts.shape[2], dtype=np.float64))
    asd, hd, valid = np.zeros(P), np.zeros(P), np.zeros(P)
    for p in range(P):
        n = counts[0, p].sum()
        if n == 0:                                                              # an empty prediction has no border voxel, an empty ground truth only sentinels
            continue
        valid[p] = 1
        asd[p] = np.dot(counts[0, p], roots) / n
        if hd95:
            hd[p] = _percentile95(counts[0, p] + counts[1, p], roots)
    return asd, hd, valid


def calculate_metric_percase(allcls_pred, allcls_gt, num_classes, surface=False, hd95=False):
    """reference test_util3d.py:186-215.  (metric, valid) [num_classes - 1, 4] with columns [dice, jc, hd, asd].  The default is test_util3d.calculate_metric_percase:
    columns 2 and 3 are 0 and invalid.  surface=True is the reference's return value: column 3 = medpy's asd(pred, gt), column 2 = 0 (the reference's hd95 call is
    commented out), both valid where prediction and ground truth are non-empty.  hd95=True (implies surface) also fills column 2 with medpy's hd95(pred, gt)."""
    metric, valid = _T3.calculate_metric_percase(allcls_pred, allcls_gt, num_classes)
    if surface or hd95:
        asd, hd, ok = surface_metrics(allcls_pred[1:num_classes], allcls_gt[1:num_classes], hd95=hd95)
        metric[:, 2], metric[:, 3] = hd, asd
        valid[:, 2] = valid[:, 3] = ok
    return metric, valid


def case_metrics(counts):
    """(metric, valid) float64 [3, 4], columns [dice, jc, hd, asd], of one BraTS case from its integer counts [3, 3] = {sum pred * gt, sum pred, sum gt} per
    foreground class (SF.brats_case_tail; a tensor or an array): the expressions of test_util3d.calculate_metric_percase -- dice = 2 i / (p + g), 0 when p + g == 0;
    jc = i / (p + g - i), invalid when g == 0; the surface columns 0 / invalid.  The sums enter as float32 scalars, the type segx_dice_sums hands that function, so
    the quotients are its quotients bit for bit wherever its float32 sums are exact (counts below 2^24); beyond that the counts here are still the exact ones."""
    sums = (counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).astype(np.float32)
    if sums.shape != (3, 3):
        raise ValueError('case_metrics: counts [3, 3], not %r' % (sums.shape,))
    metric = np.zeros((3, 4)); valid = np.ones((3, 4))
    for c in range(3):
        inter, ps, gs = sums[c]
        dice = 2.0 * inter / (ps + gs) if ps + gs > 0 else 0.0
        if gs > 0:
            jc = inter / (ps + gs - inter)
        else:
            jc = 0.0; valid[c, 1] = 0
        valid[c, 2] = valid[c, 3] = 0
        metric[c] = [dice, jc, 0, 0]
    return metric, valid


class GraphedSlidingWindow3d(GraphedEvaluation):
    """infer2d.GraphedSlidingWindow for a volume: the fused sliding-window evaluation of one image shape [C, H, W, D] -- gather, the forward of every chunk, merge and,
    when asked, the case tail (SF.brats_case_tail) -- captured into one hipGraph and replayed; the BraTS task (n-hot hardening with the consistency rule).

    net must be in eval mode (RuntimeError otherwise).  fold_bn folds its backbone's BatchNorm3d layers (fold_batchnorm) if they are not folded already; close()
    unfolds what the constructor folded, and so does a failed construction.  with_labels: the export label volume (uint8 [H, W, D]) is part of the capture;
    with_mask: the object owns a static int32 [H, W, D] ground-truth buffer and the capture also forms the case's counts (int32 [3, 3], case_metrics() turns them
    into Dice / Jaccard).  __call__(image) or __call__(image, mask) copies into the static buffers, replays and returns (preds_hard, preds_soft, labels, counts):
    STATIC tensors that the next call overwrites -- clone what must outlive it; entries that were not asked for are None.  A call raises RuntimeError once the net
    was put in train mode or its fold state differs from the one captured, ValueError on another shape.
    precision ('fp32' default, 'bf16x3'): warm-up and capture run inside inference_precision(precision); a replay needs no setting and leaves none behind.
    The gather and score buffers hold all windows (test_single_case: about 0.93 GB each for a BraTS case) for the life of the object.
    tta: flip test-time augmentation as test_single_case(fused=True, tta=) runs it, inside the capture; the buffers then hold V times as much, and the case tail reads
    the averaged map.
    postprocess: None (default: exactly the capture without it) or a dict of postprocess_brats' keyword arguments: the rule runs inside the capture between the merge
    and the case tail, so preds_hard, the counts and the label volume are the post-processed ones; preds_soft is the merged map unchanged.
    lesionwise: None (default: exactly the capture without it) or a dict of lesionwise_metrics' keyword arguments; needs with_mask=True (ValueError otherwise).  The
    dilation of the ground truth, the two labellings and the lesion kernels (SF.lesion_rows with gt_map='brats' on channels 1..3 of preds_hard) run inside the
    capture after the rule and the case tail; __call__ keeps its 4-tuple, the STATIC tables are the attributes lesion_rows [3, LESION_MAX_GT, 4] and
    lesion_header [3, LESION_HEADER] (lesionwise_from_tables reads them).  The capture then holds four more int32 and two more byte volumes per region."""

    _fold, _unfold = staticmethod(fold_batchnorm), staticmethod(unfold_batchnorm)

    def __init__(self, net, image_shape, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, num_classes=4, fold_bn=True, warmup=2,
                 precision='fp32', with_labels=True, with_mask=False, tta=None, postprocess=None, lesionwise=None):
        self.with_labels, self.with_mask = bool(with_labels), bool(with_mask)
        views = None if tta is None else SF.check_views(tta, 3)                      # refused before the net is folded or anything is launched
        self.post = check_postprocess(postprocess, num_classes)
        self.lw = check_lesionwise(lesionwise, num_classes)
        if self.lw is not None and not self.with_mask:
            raise ValueError('GraphedSlidingWindow3d: lesionwise= needs the ground truth: build it with_mask=True')
        self.lesion_rows = self.lesion_header = None
        super().__init__(net, num_classes, fold_bn, warmup, precision, image_shape, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, views)

    def _build(self, device, *plan_args):
        self.plan = _Plan3d(*plan_args[:-1], device, plan_args[-1])
        spatial = self.plan.shape[1:]
        self.mask = torch.zeros(spatial, dtype=torch.int32, device=device) if self.with_mask else None
        self.counts = torch.zeros(3, 3, dtype=torch.int32, device=device) if self.with_mask else None
        self.labels = torch.zeros(spatial, dtype=torch.uint8, device=device) if self.with_labels else None
        self.flag = torch.zeros(2, dtype=torch.int32, device=device) if self.post is not None else None
        if self.lw is not None:
            self.lesion_rows = torch.zeros(3, SegxLib.LESION_MAX_GT, 4, dtype=torch.int32, device=device)
            self.lesion_header = torch.zeros(3, SegxLib.LESION_HEADER, dtype=torch.int32, device=device)

    def _sequence(self):
        hard, soft = self.plan.run(self.net, self.image)
        if self.post is not None:
            hard, _ = SF.brats_postprocess(hard, flag=self.flag, **self.post)
        if self.with_labels or self.with_mask:
            SF.brats_case_tail(soft, hard, self.mask, want_labels=self.with_labels, counts=self.counts, labels=self.labels)
        if self.post is not None and self.with_labels:
            SF.brats_relabel(self.labels, hard, self.flag, out=self.labels)
        if self.lw is not None:
            SF.lesion_rows(hard[1:4], self.mask, gt_map='brats', out=(self.lesion_rows, self.lesion_header), **_kernel_args(self.lw))
        return hard, soft

    def _check_classes(self):
        if self.preds_soft.shape[0] != self.num_classes:
            raise ValueError('the net has %d classes, not %d' % (self.preds_soft.shape[0], self.num_classes))

    def __call__(self, image, mask=None):
        self._check(image)
        if (mask is not None) != self.with_mask:
            raise ValueError('GraphedSlidingWindow3d: built with_mask=%r: call it %s a mask' % (self.with_mask, 'with' if self.with_mask else 'without'))
        if mask is not None and tuple(mask.shape) != self.plan.shape[1:]:
            raise ValueError('GraphedSlidingWindow3d: captured for masks %r, got %r' % (self.plan.shape[1:], tuple(mask.shape)))
        if mask is not None and mask is not self.mask:
            self.mask.copy_(mask, non_blocking=True)           # converts to int32
        self._replay(image)
        return self.preds_hard, self.preds_soft, self.labels, self.counts

    def close(self):
        """GraphedEvaluation.close(), and drop the case's static buffers as well"""
        super().close()
        self.labels = self.counts = self.image = self.mask = self.flag = self.lesion_rows = self.lesion_header = None


def test_all_cases(net, db_test, task_name='brats', net_type='segtran', num_classes=4, batch_size=8, orig_patch_size=(128, 112, 80),
                   input_patch_size=(128, 112, 64), stride_xy=56, stride_z=40, has_mask=True, on_labels=None, fused=True, graph=False, surface=False, hd95=False,
                   precision='fp32', fold_bn=False, tta=None, postprocess=None, lesionwise=None):
    """The reference's evaluation loop over the cases of a dataset (test_util3d.py:15-91) for the BraTS task, without its file I/O; returns avg_metric
    [num_classes - 1, 4] (columns dice, jc, hd, asd) = the sum of the cases' metrics over the number of cases in which each entry is valid, as the reference does
    (an entry valid in no case is 0 / 0 = NaN).

    db_test: anything indexable with len(), of samples holding 'image' [C, H, W, D], 'mask' [H, W, D] (raw BraTS labels) and 'image_path'.  Per case: the
    sliding-window evaluation (test_single_case with fused=; graph=True: one GraphedSlidingWindow3d per distinct image shape, closed at the end), then ONE
    tail launch (SF.brats_case_tail) that maps the ground truth in registers, forms the case's integer counts and, when on_labels is given, the export label
    volume.  The counts of all cases stay on the device ([ncases, 3, 3]) and are read once after the loop: the default path has no copy to the host per case.
    on_labels(image_name, labels) receives the uint8 [H, W, D] device volume the reference would save (image_name = the file name up to its first dot); writing
    NIfTI is the caller's.  has_mask=False: no metrics (every entry 0 over ncases, as in the reference).
    surface=True (hd95=True implies it): columns 2 and 3 through surface_metrics on the float ground truth of SF.label_nhot(., 'brats') -- that builds the
    [4, S] maps and reads its histograms from the device once per case.
    fold_bn: ONE fold for all the cases; precision: as test_single_case.  The reference's test_interp is not built.
    tta: flip test-time augmentation of every case's evaluation, as test_single_case takes it (fused, eager or graph).
    postprocess: None or a dict of postprocess_brats' keyword arguments: the rule runs on the device between every case's merge and its tail, so the Dice / Jaccard
    counts, the surface columns and the on_labels volumes all see the post-processed prediction.
    lesionwise: None (default: the return value is avg_metric alone, nothing more is launched or allocated) or a dict of lesionwise_metrics' keyword arguments: every
    case's lesion tables (SF.lesion_rows on channels 1..3 of the -- post-processed -- preds_hard against the raw mask, gt_map='brats') stay on the device and are
    read once after the loop, and the call returns (avg_metric, lw) with lw['cases'][i][r] = lesionwise_from_tables' dict of case i and region r (ET, WT, TC) and
    lw['mean_lesion_dice'] [3] = the mean of lesion_dice over the cases.  Needs has_mask (ValueError otherwise)."""
    post = check_postprocess(postprocess, num_classes)
    lw = check_lesionwise(lesionwise, num_classes)
    if lw is not None and not has_mask:
        raise ValueError('test_all_cases: lesionwise= needs the ground truth (has_mask=True)')
    _check_task(net_type, task_name)
    views = None if tta is None else SF.check_views(tta, 3)
    if num_classes != 4:
        raise NotImplementedError('num_classes %r: only the 4-class BraTS task is built' % (num_classes,))
    surface = bool(surface or hd95)
    ncases = len(db_test)
    device = next(net.parameters()).device
    counts_all = torch.zeros(ncases, 3, 3, dtype=torch.int32, device=device) if has_mask else None
    lesion_tables = None
    if lw is not None:
        lesion_tables = (torch.zeros(ncases, 3, SegxLib.LESION_MAX_GT, 4, dtype=torch.int32, device=device),
                         torch.zeros(ncases, 3, SegxLib.LESION_HEADER, dtype=torch.int32, device=device))
    surf = []
    graphs = {}
    try:
        with _precision(precision), _folded(net, fold_bn), torch.no_grad():
            for i in range(ncases):
                sample = db_test[i]
                image, mask = sample['image'].to(device), (sample['mask'].to(device) if has_mask else None)
                image_name = os.path.basename(os.path.normpath(sample['image_path'])).split('.')[0]
                want_labels = on_labels is not None
                if graph:
                    g = graphs.get(tuple(image.shape))
                    if g is None:
                        g = graphs[tuple(image.shape)] = GraphedSlidingWindow3d(net, image.shape, orig_patch_size, input_patch_size, batch_size, stride_xy,
                                                                                stride_z, num_classes, fold_bn=False, precision=precision,
                                                                                with_labels=want_labels, with_mask=has_mask, tta=views, postprocess=post,
                                                                                lesionwise=lw)
                    preds_hard, _, labels, counts = g(image, mask) if has_mask else g(image)
                    if has_mask:
                        counts_all[i].copy_(counts)
                    if lw is not None:
                        lesion_tables[0][i].copy_(g.lesion_rows)
                        lesion_tables[1][i].copy_(g.lesion_header)
                    if want_labels:
                        labels = labels.clone()                 # the graph's static volume: the next replay overwrites it
                else:
                    preds_hard, preds_soft = test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name,
                                                              net_type=net_type, num_classes=num_classes, fused=fused, tta=views)
                    labels = None
                    if post is not None:
                        preds_hard, flag = SF.brats_postprocess(preds_hard, **post)
                    if has_mask or want_labels:
                        _, labels = SF.brats_case_tail(preds_soft, preds_hard, mask, want_labels=want_labels, counts=counts_all[i] if has_mask else None)
                    if post is not None and want_labels:
                        labels = SF.brats_relabel(labels, preds_hard, flag, out=labels)
                    if lw is not None:
                        SF.lesion_rows(preds_hard[1:4], mask, gt_map='brats', out=(lesion_tables[0][i], lesion_tables[1][i]), **_kernel_args(lw))
                if surface and has_mask:
                    gt = SF.label_nhot((mask - (mask == 4).to(mask.dtype)).unsqueeze(0), 'brats')[0]
                    surf.append(surface_metrics(preds_hard[1:num_classes], gt[1:num_classes], hd95=hd95))
                if want_labels:
                    on_labels(image_name, labels)
    finally:
        for g in graphs.values():
            g.close()
    total, valid_counts = np.zeros((num_classes - 1, 4)), np.zeros((num_classes - 1, 4))
    if has_mask:
        for i, c in enumerate(counts_all.cpu().numpy()):       # the one device-to-host copy of the default path
            metric, valid = case_metrics(c)
            if surface:
                asd, hd, ok = surf[i]
                metric[:, 2], metric[:, 3] = hd, asd
                valid[:, 2] = valid[:, 3] = ok
            total += metric
            valid_counts += valid
    else:
        valid_counts += ncases
    with np.errstate(divide='ignore', invalid='ignore'):
        avg_metric = total / valid_counts
    if lw is None:
        return avg_metric
    cases = [lesionwise_from_tables(r, h, lw['min_lesion_voxels']) for r, h in zip(lesion_tables[0].cpu().numpy(), lesion_tables[1].cpu().numpy())]
    mean = np.array([[c[r]['lesion_dice'] for r in range(3)] for c in cases], dtype=np.float64).reshape(ncases, 3).mean(0) if ncases else np.full(3, np.nan)
    return avg_metric, dict(cases=cases, mean_lesion_dice=mean)


test_all_cases.__test__ = False
