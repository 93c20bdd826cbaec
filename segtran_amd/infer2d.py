"""2-D evaluation with BatchNorm folded into the backbone's kernels: test_util2d's sliding-window inference with a `fold_bn` switch.

test_util2d.py mirrors the reference's file of that name and keeps the reference's signatures; the switch lives here.  fold_bn=True folds the (eval-mode) net for
the call if it is not folded already (Segtran2d.fold_batchnorm) and unfolds it afterwards; a net the caller folded stays folded."""
import contextlib

from . import test_util2d as _T2
from .test_util2d import calc_dice, calc_batch_metric          # noqa: F401  (same module surface)


@contextlib.contextmanager
def _folded(net, fold_bn):
    here = bool(fold_bn) and not net.batchnorm_folded
    if here:
        net.fold_batchnorm()
    try:
        yield
    finally:
        if here:
            net.unfold_batchnorm()


def test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, model_type='segtran', fold_bn=False):
    """test_util2d.test_single_batch; fold_bn: with the backbone's BatchNorm layers folded into its convolutions for this call."""
    with _folded(net, fold_bn):
        return _T2.test_single_batch(net, image_batch, orig_input_size, patch_size, stride, task_name, num_classes, model_type)


def test_all_cases(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func=None, fold_bn=False):
    """test_util2d.test_all_cases; fold_bn: ONE fold for all the batches."""
    with _folded(net, fold_bn):
        return _T2.test_all_cases(net, batches, task_name, num_classes, orig_input_size, patch_size, stride, mask_prepred_mapping_func)


# reference function names; not pytest tests
test_single_batch.__test__ = False
test_all_cases.__test__ = False
