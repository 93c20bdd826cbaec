"""2-D evaluation with BatchNorm folded into the backbone's kernels: test_util2d's sliding-window inference with a `fold_bn` switch, a `fused` form
(one gather launch, the network on stacked windows, one merge launch) and that form captured as one replayable hipGraph (GraphedSlidingWindow).

test_util2d.py mirrors the reference's file of that name and keeps the reference's signatures; the switch lives here.  So does the tail of the evaluation after
preds_soft: calc_vcdr, calc_batch_metric with the vCDR-error column, remove_fragmentary_segs, export_masks; and the one-hot tasks' form of it
(DESIGN.md 5t): calc_batch_metric_onehot and test_all_cases(gt_is_index=True), which work from index masks through one tail launch.  fold_bn=True folds the (eval-mode) net for
the call if it is not folded already (Segtran2d.fold_batchnorm) and unfolds it afterwards; a net the caller folded stays folded.  The n-hot tasks (fundus, polyp)
have the tail as one launch as well: SF.nhot_case_tail behind calc_batch_metric(fused=True), test_all_cases(device_tail=True) and
export_masks(fused=True), and captured with the forward in GraphedBatchEvaluation."""
import math

import torch

from . import functional as SF
from . import test_util2d as _T2
from .test_util2d import calc_dice          # noqa: F401  (same module surface)
from .dataloaders.datasets2d import fundus_inv_map_mask, harden_segmap2d, polyp_inv_map_mask
from .infer_common import PRECISIONS, GraphedEvaluation, _precision, composed_tta, folded, inference_precision, run_chunks, view_chunks      # noqa: F401  (same module surface)


def _folded(net, fold_bn):
    """fold for the block if asked and not folded already (Segtran2d.fold_batchnorm); a net the caller folded stays folded"""
    return folded(net, fold_bn, lambda n: n.fold_batchnorm(), lambda n: n.unfold_batchnorm())


def sliding_windows(H, W, orig_input_size, stride):
    """The window geometry of test_util2d.test_single_batch for an H x W image: ((hl_pad, wl_pad), (H2, W2), origins) -- the left pads, the padded extent and
    the (xs, ys) origin of every window in padded coordinates, visited x-outer, y-inner, the last row / column clamped to extent - window.  A stride above its
    window extent leaves cells no window covers (the eager path divides 0 by 0 there): ValueError."""
    dx, dy = (int(v) for v in orig_input_size)
    s0, s1 = (int(v) for v in stride)
    if s0 <= 0 or s1 <= 0 or s0 > dx or s1 > dy:
        raise ValueError('sliding_windows: stride %r must be positive and at most the window %r' % (tuple(stride), tuple(orig_input_size)))
    h_pad, w_pad = max(dx - H, 0), max(dy - W, 0)
    hl_pad, wl_pad = h_pad // 2, w_pad // 2
    H2, W2 = H + h_pad, W + w_pad
    sx = math.ceil((H2 - dx) / s0) + 1
    sy = math.ceil((W2 - dy) / s1) + 1
    origins = [(min(s0 * x, H2 - dx), min(s1 * y, W2 - dy)) for x in range(sx) for y in range(sy)]
    return (hl_pad, wl_pad), (H2, W2), origins


# The per-plane kernels of the backbone and the FPNs take (sample, channel) planes as a grid axis and refuse more: `SEGX_REQUIRE((int64_t)B * C <= 65535, ...)` in
# segx_dwconv2d_fwd / segx_dwconv2d_bias_act_pool / segx_plane_scale / segx_plane_bias_add (backbone.hip) and segx_groupnorm_fwd (fpn.hip).
MAX_PLANES = 65535


def max_stacked_samples(net):
    """the largest batch one net() call accepts: MAX_PLANES over the widest convolution output of the model (EfficientNet-B4: 2688 expanded channels -> 24)"""
    widest = max((m.weight.shape[0] for m in net.modules() if isinstance(getattr(m, 'weight', None), torch.Tensor) and m.weight.dim() >= 4), default=1)
    return max(1, MAX_PLANES // int(widest))


class _Plan:
    """what the fused sequence needs beyond the image: the window table on the device and the geometry"""

    def __init__(self, net, image_shape, orig_input_size, patch_size, stride, device, window_batch, tta=None):
        self.shape = tuple(int(v) for v in image_shape)
        self.views = None if tta is None else SF.ViewTable(tta, 2, device)          # refuses a bad tta before anything is launched
        self.window, self.patch = tuple(int(v) for v in orig_input_size), tuple(int(v) for v in patch_size)
        self.pads, self.canvas, origins = sliding_windows(self.shape[2], self.shape[3], self.window, stride)
        self.table = SF.WindowTable(origins, device)
        nwin = self.table.nwin
        fit = max(1, max_stacked_samples(net) // self.shape[0])          # windows per call the library's plane limit leaves room for
        self.window_batch = min(nwin, fit) if window_batch is None else min(nwin, int(window_batch))
        if self.window_batch < 1:
            raise ValueError('window_batch must be at least 1')

    def run(self, net, image_batch):
        """gather -> net() on chunks of window_batch windows (window_batch * B samples each) -> merge; the caller holds torch.no_grad()"""
        B, nwin = self.shape[0], self.table.nwin
        chunks = [(k * B, min(k + self.window_batch, nwin) * B) for k in range(0, nwin, self.window_batch)]
        if self.views is not None:                                                  # the views are more rows of the stacked batch; a chunk never mixes two
            chunks = view_chunks(chunks, nwin * B, self.views.V)
        patches = SF.window_gather(image_batch, self.table, self.window, self.patch, self.pads, self.canvas, views=self.views)
        scores = run_chunks(net, patches, chunks)
        preds_soft, preds_hard = SF.window_merge(scores, self.table, self.window, self.shape[2:], self.pads, self.canvas, mode=0, views=self.views)
        return preds_hard.to(torch.int32), preds_soft


def test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, model_type='segtran', fold_bn=False, fused=False,
                      window_batch=None, precision='fp32', tta=None):
    """test_util2d.test_single_batch; fold_bn: with the backbone's BatchNorm layers folded into its convolutions for this call.
    fused: one window_gather launch, net() on chunks of `window_batch` windows (window_batch * B samples each; default: all windows in one call, or the largest chunks
    max_stacked_samples(net) allows), one
    window_merge launch -- no canvas copy, no per-window accumulate pass.  With window_batch=1 the forwards are the eager path's, and so are the results, bit
    for bit; stacked windows change the GEMMs' shapes, hence the summation order inside the network.
    precision: 'fp32' (default) or 'bf16x3' -- the forwards run inside inference_precision(precision).
    tta: None (default: exactly the call without it) or a sequence of up to 8 views for flip test-time augmentation.  A view is a tuple of distinct
    image axes to flip, 0 = H, 1 = W -- e.g. ((), (1,), (0,), (0, 1)); the identity () has to be listed to be used.  With soft_v = this call's preds_soft for the
    image flipped along view v's axes (the un-padded image is flipped: pads, origins and clamping are those of the un-flipped shape), flipped back,
    preds_soft = (((soft_0 + soft_1) + soft_2) + ...) / float(V) in fp32 and preds_hard is its hardening.  fused=False runs that as a host loop
    (infer_common.composed_tta); fused=True runs one gather launch for all views, net() on the chunks of each view in turn (a chunk never mixes views: with
    window_batch=1 the forwards are the host loop's and the results equal it bit for bit) and one merge launch -- no flipped image, no per-view soft map, no ATen
    add or divide.  The gather and the score buffer hold V times what they hold without tta.  A bad tta (empty, more than 8 views, an axis outside 0..1 or twice in
    a view, the same set of axes twice) raises ValueError before anything is launched."""
    if fused and model_type not in ('segtran',):
        raise NotImplementedError("model_type '%s': only segtran is built" % model_type)
    views = None if tta is None else SF.check_views(tta, 2)
    with _precision(precision), _folded(net, fold_bn):
        if not fused:
            if views is None:
                return _T2.test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, model_type)
            hard, soft = composed_tta(lambda x: _T2.test_single_batch(net, x, orig_input_size, patch_size, stride, task_name, num_classes, model_type),
                                      image_batch, views, 2, 0)
            return hard.to(torch.int32), soft
        plan = _Plan(net, image_batch.shape, orig_input_size, patch_size, stride, image_batch.device, window_batch, views)
        with torch.no_grad():
            return plan.run(net, image_batch)


def calc_vcdr(mask_nhot_soft, thres=0.5, delta=1):
    """reference utils/losses.py:76-127, the vertical cup/disc ratio of n-hot maps (0 background, 1 disc, 2 cup), soft or hard: the vertical extent of the
    thresholded cup over that of the disc.  The extents come from SF.row_extent; the few scalar operations keep the reference's dtypes (int64 lengths, float32
    quotient), so the values are the reference's bit for bit.  No branch on device data, no copy to the host: the call can be captured into a graph.

    [C, H, W] (one image): (max_idx - min_idx - delta) of the cup over that of the disc + 0.0001; -1. without a disc, 0. without a cup; a 0-dim float32 tensor.
    [B, C, H, W]: the reference's batch form as it is -- no delta, and the minimum runs over occupied * index, so it is 0 whenever any row is unoccupied
    (the length is then the highest occupied row + 1); a float32 [B] tensor."""
    m = mask_nhot_soft.detach().float()
    if m.dim() == 4:
        B, _, H, W = m.shape
        vert_indices = torch.arange(1, H + 1, device=m.device).repeat(B, 1)

        def vert_len(c):                                     # a row is a plane of height 1: its extent is (0, 0) when occupied, (1, -1) when not
            occupied = SF.row_extent(m[:, c].reshape(B * H, 1, W), thres)[:, 1].view(B, H) == 0
            indexed = occupied * vert_indices
            return indexed.max(dim=1)[0] - indexed.min(dim=1)[0]
        return vert_len(2) / (vert_len(1) + 0.0001)
    if m.dim() != 3:
        raise ValueError('calc_vcdr: [C, H, W] or [B, C, H, W] n-hot maps, not rank %d' % m.dim())
    ext = SF.row_extent(m[1:3], thres).long()               # [2, 2]: (lowest, highest) row of disc and cup; (H, -1) where empty
    length = ext[:, 1] - ext[:, 0] - delta
    vcdr = length[1] / (length[0] + 0.0001)
    vcdr = torch.where(ext[1, 1] < 0, 0., vcdr)              # no cup
    return torch.where(ext[0, 1] < 0, -1., vcdr)            # no disc (tested first in the reference)


def vcdr_from_extents(ext, delta=1):
    """calc_vcdr's [C, H, W] branch from row extents, for a batch: ext int32 [B, 2, 2, 2] as SF.nhot_case_tail returns it ({prediction, ground truth} x {disc, cup} x
    (lowest, highest) row; (H, -1) when empty) -> (vcdr of the predictions, vcdr of the ground truths), float32 [B] tensors on the device; ext [B, 2, 2] (one of the
    halves) -> one such tensor.  The operations and dtypes are calc_vcdr's (int64 lengths, float32 quotient with + 0.0001, 0. without a cup, then -1. without a
    disc), elementwise: entry i is calc_vcdr(map_i) bit for bit.  No copy to the host."""
    if ext.dim() not in (3, 4) or tuple(ext.shape[-2:]) != (2, 2) or (ext.dim() == 4 and ext.shape[1] != 2):
        raise ValueError('vcdr_from_extents: row extents [B, 2, 2, 2] or [B, 2, 2], not %s' % (tuple(ext.shape),))
    e = ext.long()
    length = e[..., 1] - e[..., 0] - delta                    # [..., class]
    vcdr = length[..., 1] / (length[..., 0] + 0.0001)
    vcdr = torch.where(e[..., 1, 1] < 0, 0., vcdr)            # no cup
    vcdr = torch.where(e[..., 0, 1] < 0, -1., vcdr)           # no disc
    return (vcdr[:, 0], vcdr[:, 1]) if ext.dim() == 4 else vcdr


def _equal_runs(keys):
    """[(i0, i1)]: the maximal runs of consecutive equal entries of keys"""
    runs, i0 = [], 0
    for i in range(1, len(keys) + 1):
        if i == len(keys) or keys[i] != keys[i0]:
            runs.append((i0, i))
            i0 = i
    return runs


def _batched(items, i0, i1):
    """items[i0:i1] as one [n, ...] tensor: a slice of a tensor, a stack of a list's entries"""
    return items[i0:i1] if isinstance(items, torch.Tensor) else torch.stack(list(items[i0:i1]))


def _nhot_metric_rows(preds_soft, gt, num_classes, do_calc_vcdr_error, gt_map='nhot'):
    """float32 [B, num_classes - 1 (+ 1)] on the device: the rows of calc_batch_metric for one batch of equally sized masks from ONE tail launch -- Dice as calc_dice's
    expression on the integer counts, then |vCDR(gt) - vCDR(pred)| from the row extents"""
    if preds_soft.shape[1] != num_classes:
        raise ValueError('preds_soft has %d classes, not %d' % (preds_soft.shape[1], num_classes))
    counts, ext, _, _ = SF.nhot_case_tail(preds_soft.float(), gt, gt_map=gt_map, want_extents=do_calc_vcdr_error)
    c, smooth = counts.float(), 1e-5
    rows = (2 * c[..., 0] + smooth) / (c[..., 1] + c[..., 2] + smooth)                          # SF.dice_scores' expression on the same sums
    if do_calc_vcdr_error:
        vcdr_pred, vcdr_gt = vcdr_from_extents(ext)
        rows = torch.cat([rows, (vcdr_gt - vcdr_pred).abs().unsqueeze(1)], dim=1)
    return rows


def calc_batch_metric(BC_pred_soft, BC_gt, num_classes, do_calc_vcdr_error=False, fused=False):
    """reference test_util2d.py:241-265.  The default is test_util2d.calc_batch_metric, unchanged (that function still refuses the flag); with do_calc_vcdr_error
    the table has one more column, |calc_vcdr(gt) - calc_vcdr(pred)| (:259-263, the fundus task's own metric): that function's loop -- resample, harden, Dice,
    the same calls, so the Dice columns are the default's bit for bit -- with the column computed from the same hardened maps.
    fused: the table from ONE tail launch (SF.nhot_case_tail; one per run of equally sized masks when BC_gt is a list of differently sized maps) and ONE read: the
    resampled and the hardened maps never exist.  Integer counts and extents, the same float32 expressions: the table equals the default's exactly while a plane has
    fewer than 2^24 pixels (float32 holds the default's sums exactly up to there)."""
    if fused:
        with torch.no_grad():
            keys = [(tuple(p.shape), tuple(g.shape)) for p, g in zip(BC_pred_soft, BC_gt)]
            if len(keys) != len(BC_pred_soft) or len(keys) != len(BC_gt) or not keys:
                raise ValueError('calc_batch_metric: %d predictions for %d masks' % (len(BC_pred_soft), len(BC_gt)))
            rows = [_nhot_metric_rows(_batched(BC_pred_soft, i0, i1), _batched(BC_gt, i0, i1), num_classes, do_calc_vcdr_error) for i0, i1 in _equal_runs(keys)]
            return torch.cat(rows).cpu().numpy().astype(_T2.np.float64)                         # the one read
    if not do_calc_vcdr_error:
        return _T2.calc_batch_metric(BC_pred_soft, BC_gt, num_classes)
    out = _T2.np.zeros((len(BC_pred_soft), num_classes))
    for ins, (C_pred_soft, C_gt) in enumerate(zip(BC_pred_soft, BC_gt)):
        if tuple(C_pred_soft.shape[1:]) != tuple(C_gt.shape[1:]):
            C_pred_soft = SF.interp_linear(C_pred_soft.unsqueeze(0).contiguous(), tuple(C_gt.shape[1:]))[0]
        C_pred = harden_segmap2d(C_pred_soft)
        d = SF.dice_scores(C_pred[1:].float().reshape(num_classes - 1, -1), C_gt[1:].float().reshape(num_classes - 1, -1))
        out[ins, :num_classes - 1] = d.cpu().numpy()
        out[ins, num_classes - 1] = _T2.np.abs((calc_vcdr(C_gt) - calc_vcdr(C_pred)).cpu().numpy())
    return out


def remove_fragmentary_segs(segmap, bg_value):
    """reference test_util2d.py:267-289 on the device: segmap is a uint8 label image [H, W] or a stack [P, H, W] (each plane on its own) on the device.  The
    8-connected components of segmap != bg_value are labelled, the two most frequent of {background, components} stay, every other component is painted bg_value.
    Returns a NEW tensor of the same shape, dtype and device; the input is not modified (the reference writes into its host copy).

    It gives the reference's result wherever the reference is defined: at least one background pixel, at least one foreground component, and no tie at the
    cut (the second and third largest counts differ).  Outside that domain the reference drops into pdb (fewer than two labels) or depends on argpartition's
    unspecified order among equals; here ties go to the background first, then to the component whose first pixel comes first in raster order, and a plane that
    is all background or all foreground comes back unchanged."""
    if not isinstance(segmap, torch.Tensor) or segmap.dtype != torch.uint8:
        raise TypeError('remove_fragmentary_segs: a uint8 device tensor, not %s' % (segmap.dtype if isinstance(segmap, torch.Tensor) else type(segmap).__name__))
    return SF.remove_fragments(segmap, bg_value)


def _index_mask(what, preds_soft, gt_index):
    """the index mask as [B, H, W] next to preds_soft [B, C, H, W]"""
    if not isinstance(preds_soft, torch.Tensor) or preds_soft.dim() != 4:
        raise ValueError('%s: preds_soft is a [B, C, H, W] tensor' % what)
    gt = gt_index[:, 0] if gt_index.dim() == 4 and gt_index.shape[1] == 1 else gt_index
    if gt.dim() != 3 or gt.shape[0] != preds_soft.shape[0]:
        raise ValueError('%s: an index mask [B, H, W] or [B, 1, H, W] for %d images, not %s' % (what, preds_soft.shape[0], tuple(gt_index.shape)))
    return gt


def _onehot_counts(preds_soft, gt, num_classes):
    """int32 [B, C - 1, 3] on the device: {sum pred * gt, sum pred, sum gt} per image and foreground class (SF.onehot_case_tail); preds_soft is resampled to the
    mask's size first when it differs, as calc_batch_metric does"""
    if preds_soft.shape[1] != num_classes:
        raise ValueError('preds_soft has %d classes, not %d' % (preds_soft.shape[1], num_classes))
    if tuple(preds_soft.shape[2:]) != tuple(gt.shape[1:]):
        preds_soft = SF.interp_linear(preds_soft.contiguous(), tuple(gt.shape[1:]))
    return SF.onehot_case_tail(preds_soft.float(), gt, want_labels=False)[0]


def calc_batch_metric_onehot(preds_soft, gt_index, num_classes):
    """calc_batch_metric (reference test_util2d.py:241-265) for a one-hot task, from the index mask: preds_soft [B, C, H, W], gt_index [B, H, W] or [B, 1, H, W]
    integer labels.  One launch forms the integer counts {I, Z, Y} = {sum pred * gt, sum pred, sum gt} of every image and class (the hardened maps and the
    one-hot mask never exist), ONE read brings them to the host, and Dice is calc_dice's expression (2 I + 1e-5) / (Z + Y + 1e-5) in float32.  0 / 1 maps square to
    themselves and float32 holds every integer below 2^24, so the table equals the reference's exactly while a plane has fewer than 2^24 pixels.
    Returns the float64 [B, C - 1] table."""
    np = _T2.np
    with torch.no_grad():
        counts = _onehot_counts(preds_soft, _index_mask('calc_batch_metric_onehot', preds_soft, gt_index), num_classes)
    c = counts.cpu().numpy().astype(np.float32)
    smooth = np.float32(1e-5)
    return ((np.float32(2) * c[..., 0] + smooth) / (c[..., 1] + c[..., 2] + smooth)).astype(np.float64)


def test_all_cases(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func=None, fold_bn=False, fused=False,
                   window_batch=None, precision='fp32', do_calc_vcdr_error=False, gt_is_index=False, device_tail=False, gt_map='nhot', tta=None):
    """test_util2d.test_all_cases; fold_bn: ONE fold for all the batches; fused / window_batch / precision: as test_single_batch; do_calc_vcdr_error: the vCDR
    error as one more entry (both returned vectors then have num_classes entries, as in the reference).
    gt_is_index (one-hot tasks: oct): the masks are index masks [B, H, W] / [B, 1, H, W] and stay so -- no mapping function, no one-hot mask, no hardened map; each
    batch's Dice rows are formed on the device from the integer counts of SF.onehot_case_tail (calc_dice's expression in float32) and stay there; they are read
    ONCE after the last batch and summed as the default path sums its tables.
    device_tail (n-hot tasks: fundus, polyp): the same for n-hot masks -- ONE tail launch per batch (SF.nhot_case_tail) forms the Dice rows and, with
    do_calc_vcdr_error, the vCDR-error column on the device; they are read ONCE after the last batch and summed in the default path's order, so (mean, count)
    equals the default's.  gt_map ('fundus', 'fundus_exclusive', 'polyp'; needs device_tail): the batches hold the RAW uint8 masks, mapped inside the tail launch
    -- the n-hot mask never exists; it excludes mask_prepred_mapping_func.
    tta: flip test-time augmentation of every batch's evaluation, as test_single_batch takes it, in every form above."""
    views = None if tta is None else SF.check_views(tta, 2)
    if gt_is_index and (do_calc_vcdr_error or mask_prepred_mapping_func is not None or device_tail):
        raise ValueError('test_all_cases: gt_is_index takes the index masks as they are (no mask_prepred_mapping_func, no device_tail) and has no vCDR column')
    if gt_map != 'nhot' and (not device_tail or mask_prepred_mapping_func is not None):
        raise ValueError('test_all_cases: gt_map=%r reads the raw masks in the tail launch: it needs device_tail=True and excludes mask_prepred_mapping_func' % (gt_map,))
    with _precision(precision), _folded(net, fold_bn):
        if gt_is_index:
            return _test_all_cases_index(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, fused, window_batch, views)
        if device_tail:
            return _test_all_cases_tail(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func, fused, window_batch,
                                        do_calc_vcdr_error, gt_map, views)
        if not fused and not do_calc_vcdr_error and views is None:
            return _T2.test_all_cases(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func)
        np = _T2.np
        total, count = (np.zeros(num_classes), np.zeros(num_classes)) if do_calc_vcdr_error else (np.zeros(num_classes - 1), 0)
        for image_batch, mask_batch in batches:
            gt = mask_prepred_mapping_func(mask_batch) if mask_prepred_mapping_func else mask_batch
            _, preds_soft = test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, fused=fused, window_batch=window_batch,
                                              tta=views)
            m = calc_batch_metric(preds_soft, gt, num_classes, do_calc_vcdr_error=do_calc_vcdr_error)
            total += m.sum(axis=0); count += len(m)
        return total / np.maximum(count, 1), count


def _sum_tables(rows, ncols, count):
    """the ONE read of the per-batch device tables `rows` and their sum in the order the default path adds its per-batch tables; count: the default's 0 (or zeros)"""
    np = _T2.np
    total = np.zeros(ncols)
    if rows:
        sizes = [len(r) for r in rows]
        table = torch.cat(rows).cpu().numpy().astype(np.float64)                                # the one read
        for m in np.split(table, np.cumsum(sizes)[:-1]):
            total += m.sum(axis=0); count += len(m)
    return total / np.maximum(count, 1), count


def _test_all_cases_tail(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func, fused, window_batch,
                         do_calc_vcdr_error, gt_map, tta=None):
    rows = []
    for image_batch, mask_batch in batches:
        gt = mask_prepred_mapping_func(mask_batch) if mask_prepred_mapping_func else mask_batch
        _, preds_soft = test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, fused=fused, window_batch=window_batch,
                                          tta=tta)
        with torch.no_grad():
            rows.append(_nhot_metric_rows(preds_soft, gt, num_classes, do_calc_vcdr_error, gt_map))
    np = _T2.np
    return _sum_tables(rows, num_classes, np.zeros(num_classes)) if do_calc_vcdr_error else _sum_tables(rows, num_classes - 1, 0)


def _test_all_cases_index(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, fused, window_batch, tta=None):
    np = _T2.np
    rows, smooth = [], 1e-5
    for image_batch, mask_batch in batches:
        _, preds_soft = test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, fused=fused, window_batch=window_batch,
                                          tta=tta)
        with torch.no_grad():
            c = _onehot_counts(preds_soft, _index_mask('test_all_cases', preds_soft, mask_batch), num_classes).float()
            rows.append((2 * c[..., 0] + smooth) / (c[..., 1] + c[..., 2] + smooth))          # SF.dice_scores' expression on the same sums
    total, count = np.zeros(num_classes - 1), 0
    if rows:
        sizes = [len(r) for r in rows]
        table = torch.cat(rows).cpu().numpy().astype(np.float64)                                # the one read
        for m in np.split(table, np.cumsum(sizes)[:-1]):
            total += m.sum(axis=0); count += len(m)
    return total / max(count, 1), count


_INV_MAP_VALUES = {fundus_inv_map_mask: (255, 128, 0), polyp_inv_map_mask: (0, 255)}      # the value tables of the inverse maps the tail launch can stand in for


def export_masks(preds_soft, unscaled_sizes, inv_map, remove_frag=False, bg_value=255, fused=False, values=None):
    """The arithmetic of the reference's save loop (test_util2d.py:93-106, and test2d.py's --removefrag) without the files: per image i, preds_soft[i] [C, H, W] is
    resampled to unscaled_sizes[i] = (H0, W0) (interp_linear), hardened (harden_segmap2d), mapped to pixel values by inv_map (fundus_inv_map_mask /
    polyp_inv_map_mask of dataloaders.datasets2d, or functools.partial(onehot_inv_map, colormap=...) for a one-hot task: test2d.py:640-649) and, with remove_frag,
    cleaned by remove_fragmentary_segs(., bg_value).  Returns the list of uint8 [H0, W0] device tensors ([H0, W0, 3] from onehot_inv_map; fragment removal is
    defined on single-channel label images and refuses those); writing them in an image format is the caller's.
    fused: the label images come from the tail launch (SF.nhot_case_tail with size = unscaled_sizes[i]), one launch per run of equal sizes -- no resampled and no
    hardened map; the value table is `values` (C ints 0..255; inv_map may then be None) or that of inv_map when it IS fundus_inv_map_mask or polyp_inv_map_mask.
    Any other inv_map (a partial of onehot_inv_map) keeps the default path."""
    if len(unscaled_sizes) != len(preds_soft):
        raise ValueError('export_masks: %d sizes for %d predictions' % (len(unscaled_sizes), len(preds_soft)))
    if values is not None and not fused:
        raise ValueError('export_masks: values= is the table of the fused form (fused=True)')
    table = values if values is not None else (_INV_MAP_VALUES.get(inv_map) if fused else None)
    out = []
    with torch.no_grad():
        if fused and table is not None:
            keys = [(tuple(soft.shape), tuple(int(v) for v in size)) for soft, size in zip(preds_soft, unscaled_sizes)]
            for i0, i1 in _equal_runs(keys):
                soft = _batched(preds_soft, i0, i1).float()
                labels = SF.nhot_case_tail(soft, size=keys[i0][1], values=table)[2]
                out.extend((remove_fragmentary_segs(labels, bg_value) if remove_frag else labels).unbind(0))
            return out
        for soft, size in zip(preds_soft, unscaled_sizes):
            H0, W0 = (int(v) for v in size)
            soft = soft.unsqueeze(0).contiguous()
            if (H0, W0) != tuple(soft.shape[2:]):
                soft = SF.interp_linear(soft, (H0, W0))
            mask = inv_map(harden_segmap2d(soft[0]))
            if remove_frag and mask.dim() != 2:
                raise ValueError('export_masks: remove_frag works on single-channel label images, not on the %s result of this inv_map' % (tuple(mask.shape),))
            out.append(remove_fragmentary_segs(mask, bg_value) if remove_frag else mask)
    return out


class GraphedSlidingWindow(GraphedEvaluation):
    """The fused sliding-window evaluation of one image-batch shape captured into a hipGraph and replayed: gather, the forward(s) and merge -- a few hundred
    launches per forward -- become one graph launch, which takes the host out of a launch-bound evaluation (as engine.GraphedTrainStep does for the train step).

    net must be in eval mode (RuntimeError otherwise).  fold_bn folds its BatchNorm layers if they are not folded already; close() unfolds what the constructor
    folded.  __call__(image_batch) copies the batch into a static buffer, replays and returns (preds_hard int32, preds_soft) [B, num_classes, H, W]: STATIC
    tensors that the next call overwrites -- clone what must outlive it.  The captured kernels read the weights (and the folded operands) at fixed addresses, so
    a call raises RuntimeError once the net was put in train mode or its fold state differs from the one captured (train(), load_state_dict() and in-place edits
    of a folded tensor all drop the fold).
    precision ('fp32' default, 'bf16x3'): warm-up and capture run inside inference_precision(precision); a GEMM's route is fixed when it is captured, so a
    replay needs no setting and leaves none behind.  The object reports it as .precision.
    tta: flip test-time augmentation as test_single_batch(fused=True, tta=) runs it -- the view table is built before the capture, and the graph holds the one
    gather, the forwards of every view and the one merge; a replay equals that call bit for bit.  The static gather and score buffers hold V times as much."""

    def __init__(self, net, image_shape, orig_input_size, patch_size, stride, num_classes, fold_bn=True, window_batch=None, warmup=2, precision='fp32', tta=None):
        views = None if tta is None else SF.check_views(tta, 2)                      # refused before the net is folded or anything is launched
        super().__init__(net, num_classes, fold_bn, warmup, precision, image_shape, orig_input_size, patch_size, stride, window_batch, views)

    def _build(self, device, image_shape, orig_input_size, patch_size, stride, window_batch, tta=None):
        self.plan = _Plan(self.net, image_shape, orig_input_size, patch_size, stride, device, window_batch, tta)

    def _sequence(self):
        return self.plan.run(self.net, self.image)

    def _check_classes(self):
        assert self.preds_soft.shape[1] == self.num_classes, 'the net has %d classes, not %d' % (self.preds_soft.shape[1], self.num_classes)

    def __call__(self, image_batch):
        self._check(image_batch)
        self._replay(image_batch)
        return self.preds_hard, self.preds_soft



class GraphedBatchEvaluation(GraphedSlidingWindow):
    """GraphedSlidingWindow with the n-hot tasks' evaluation tail in the capture: gather, the forward(s), merge and ONE SF.nhot_case_tail launch are one graph.

    mask_size (H, W): the ground truth's size (default: the image's); gt_map: the form of the mask the object takes -- 'nhot' (float32 [B, num_classes, H, W], what
    fundus_map_mask / polyp_map_mask return) or the raw uint8 [B, 3, H, W] mask of 'fundus' / 'fundus_exclusive' / 'polyp', mapped inside the launch; values: the
    pixel values of the classes for the label images (e.g. (255, 128, 0) for fundus), None for none; with_extents: the row extents vcdr_from_extents reads.
    __call__(image_batch, mask) copies both into static buffers, replays and returns (preds_hard, preds_soft, counts, ext, labels): counts int32
    [B, num_classes - 1, 3], ext int32 [B, 2, 2, 2] or None, labels uint8 [B, H, W] or None -- STATIC tensors that the next call overwrites, nothing is read from the
    device.  A mask of another shape or dtype raises ValueError; the other guards are GraphedSlidingWindow's.  tta: as GraphedSlidingWindow; the tail reads the
    averaged soft map."""

    def __init__(self, net, image_shape, orig_input_size, patch_size, stride, num_classes, fold_bn=True, window_batch=None, warmup=2, precision='fp32',
                 mask_size=None, gt_map='nhot', values=None, with_extents=False, tta=None):
        from .segx import SegxLib
        if gt_map not in SegxLib.NHOT_GT_MAPS:
            raise ValueError('GraphedBatchEvaluation: gt_map %r is not one of %s' % (gt_map, sorted(SegxLib.NHOT_GT_MAPS)))
        self.mask_size = None if mask_size is None else tuple(int(v) for v in mask_size)
        self.gt_map, self.values, self.with_extents = gt_map, (None if values is None else tuple(values)), bool(with_extents)
        super().__init__(net, image_shape, orig_input_size, patch_size, stride, num_classes, fold_bn, window_batch, warmup, precision, tta)

    def _build(self, device, *plan_args):
        super()._build(device, *plan_args)
        B, C = self.plan.shape[0], self.num_classes
        H, W = self.mask_size = self.mask_size or self.plan.shape[2:]
        self.mask = torch.zeros((B, C, H, W), dtype=torch.float32, device=device) if self.gt_map == 'nhot' else torch.zeros((B, 3, H, W), dtype=torch.uint8, device=device)
        self.counts = torch.zeros(B, C - 1, 3, dtype=torch.int32, device=device)
        self.ext = torch.zeros(B, 2, 2, 2, dtype=torch.int32, device=device) if self.with_extents else None
        self.labels = None
        if self.values is not None:
            SF._value_table('GraphedBatchEvaluation', self.values, C, device)                   # the table's one host copy happens here, not inside the capture
            self.labels = torch.zeros(B, H, W, dtype=torch.uint8, device=device)

    def _sequence(self):
        hard, soft = self.plan.run(self.net, self.image)
        SF.nhot_case_tail(soft, self.mask, gt_map=self.gt_map, values=self.values, counts=self.counts, ext=self.ext, labels=self.labels)
        return hard, soft

    def __call__(self, image_batch, mask):
        self._check(image_batch)
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(self.mask.shape) or mask.dtype != self.mask.dtype:
            raise ValueError('GraphedBatchEvaluation: captured for %s masks %r (gt_map=%r), got %s %r' %
                             (self.mask.dtype, tuple(self.mask.shape), self.gt_map, getattr(mask, 'dtype', None), tuple(getattr(mask, 'shape', ()))))
        if mask is not self.mask:
            self.mask.copy_(mask, non_blocking=True)
        self._replay(image_batch)
        return self.preds_hard, self.preds_soft, self.counts, self.ext, self.labels

    def close(self):
        """GraphedEvaluation.close(), and drop the tail's static buffers as well"""
        super().close()
        self.mask = self.counts = self.ext = self.labels = None


# reference function names; not pytest tests
test_single_batch.__test__ = False
test_all_cases.__test__ = False
