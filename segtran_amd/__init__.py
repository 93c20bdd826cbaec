def fold_batchnorm(net):
    """Inference: fold the BatchNorm layers of net's backbone into its convolutions (Segtran2d.fold_batchnorm); returns net."""
    return net.fold_batchnorm()


def sliding_windows(H, W, orig_input_size, stride):
    """The window geometry of the 2-D sliding-window evaluation (infer2d.sliding_windows): left pads, padded extent, window origins."""
    from .infer2d import sliding_windows as f
    return f(H, W, orig_input_size, stride)


def inference_precision(name):
    """Context manager: the precision of the bf16 tile engine's GEMMs and forward 3-D convolutions inside the block (infer2d.inference_precision).  'fp32' (the default behaviour): six bf16
    products per block, fp32-equivalent; 'bf16x3': three, ~2^-15 relative per product sum -- inference only: entering with gradients enabled raises RuntimeError."""
    from .infer2d import inference_precision as f
    return f(name)


def connected_components(mask, connectivity=26):
    """6- / 26-connected components of a device mask [X, Y, Z] or [V, X, Y, Z] on the device (infer3d.connected_components): (labels, sizes)."""
    from .infer3d import connected_components as f
    return f(mask, connectivity)


def remove_small_components(mask, min_voxels=0, largest_only=False, connectivity=26):
    """A new mask without the components below min_voxels / other than the largest (infer3d.remove_small_components)."""
    from .infer3d import remove_small_components as f
    return f(mask, min_voxels, largest_only, connectivity)


def postprocess_brats(preds_hard, labels=None, **kw):
    """The usual BraTS post-processing of a hard prediction [4, H, W, D] on the device (infer3d.postprocess_brats)."""
    from .infer3d import postprocess_brats as f
    return f(preds_hard, labels, **kw)


def lesionwise_metrics(pred, gt, **kw):
    """Lesion-wise Dice, detections and false positives of binary device volumes [R, X, Y, Z] or [X, Y, Z] (infer3d.lesionwise_metrics): a list of R dicts."""
    from .infer3d import lesionwise_metrics as f
    return f(pred, gt, **kw)


def __getattr__(name):
    # all three take tta= (flip test-time augmentation inside the captured gather and merge launches: DESIGN.md 5z)
    if name == 'GraphedSlidingWindow':          # infer2d.GraphedSlidingWindow: the whole sliding-window evaluation of one image shape as one replayable hipGraph
        from .infer2d import GraphedSlidingWindow
        return GraphedSlidingWindow
    if name == 'GraphedSlidingWindow3d':        # infer3d.GraphedSlidingWindow3d: the same for one volume shape, with the BraTS case tail (label volume, metric counts)
        from .infer3d import GraphedSlidingWindow3d
        return GraphedSlidingWindow3d
    if name == 'GraphedBatchEvaluation':        # infer2d.GraphedBatchEvaluation: GraphedSlidingWindow with the n-hot tasks' tail (metric counts, row extents, label images)
        from .infer2d import GraphedBatchEvaluation
        return GraphedBatchEvaluation
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
