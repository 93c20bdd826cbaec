def fold_batchnorm(net):
    """Inference: fold the BatchNorm layers of net's backbone into its convolutions (Segtran2d.fold_batchnorm); returns net."""
    return net.fold_batchnorm()
