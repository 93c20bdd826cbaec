def fold_batchnorm(net):
    """Inference: fold the BatchNorm layers of net's backbone into its convolutions (Segtran2d.fold_batchnorm); returns net."""
    return net.fold_batchnorm()


def sliding_windows(H, W, orig_input_size, stride):
    """The window geometry of the 2-D sliding-window evaluation (infer2d.sliding_windows): left pads, padded extent, window origins."""
    from .infer2d import sliding_windows as f
    return f(H, W, orig_input_size, stride)


def __getattr__(name):
    if name == 'GraphedSlidingWindow':          # infer2d.GraphedSlidingWindow: the whole sliding-window evaluation of one image shape as one replayable hipGraph
        from .infer2d import GraphedSlidingWindow
        return GraphedSlidingWindow
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
