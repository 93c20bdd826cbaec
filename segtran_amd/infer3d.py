"""3-D evaluation with a `precision` switch: test_util3d's sliding-window inference, optionally under the three-term bf16 product.

test_util3d.py mirrors the reference's file of that name and keeps the reference's signatures; the switch lives here, as infer2d.py holds the 2-D one.  The 3-D
convolutions of Inception-I3D (conv3d.hip, conv3d_halo.hip) and the GEMMs of the bf16 tile engine follow the precision selector inside the block; the loop, the
accumulation and the hardening are test_util3d's own.

It also holds the surface-distance half of calculate_metric_percase (reference test_util3d.py:203-213: medpy's asd, and the hd95 of the commented-out line), computed on
the device in integers (metrics.hip) and finished here in float64; test_util3d.calculate_metric_percase keeps reporting those columns as invalid."""
import contextlib

import numpy as np
import torch

from . import functional as SF
from . import test_util3d as _T3
from .infer2d import PRECISIONS, _precision, inference_precision          # noqa: F401  (inference_precision: re-exported)


def fold_batchnorm(net):
    """Inference: fold the BatchNorm3d layers of a Segtran3d's I3D backbone into its convolutions (InceptionI3d.fold_batchnorm; eval mode only); returns net.  The 3-D
    entry point has its own name because Segtran3d.fold_batchnorm() keeps refusing."""
    net.backbone.fold_batchnorm()
    return net


def unfold_batchnorm(net):
    net.backbone.unfold_batchnorm()
    return net


@contextlib.contextmanager
def _folded(net, fold_bn):
    """infer2d._folded for a Segtran3d: fold for the block if asked and not folded already; a net the caller folded stays folded"""
    here = bool(fold_bn) and not net.batchnorm_folded
    if here:
        fold_batchnorm(net)
    try:
        yield
    finally:
        if here:
            unfold_batchnorm(net)


def test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type='segtran', num_classes=4,
                     precision='fp32', fold_bn=False):
    """test_util3d.test_single_case with two more arguments.  precision: 'fp32' (default) -- exactly that function's results -- or 'bf16x3' -- the same loop under
    torch.no_grad() inside inference_precision('bf16x3'); the setting the process had comes back at the end, also after an exception.  Any other name: ValueError.
    fold_bn: with the backbone's BatchNorm3d layers folded into its convolutions for this call (fold_batchnorm; a net the caller folded stays folded)."""
    with _precision(precision), _folded(net, fold_bn):
        return _T3.test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type=net_type,
                                    num_classes=num_classes)


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
