"""3-D evaluation with a `precision` switch: test_util3d's sliding-window inference, optionally under the three-term bf16 product.

test_util3d.py mirrors the reference's file of that name and keeps the reference's signatures; the switch lives here, as infer2d.py holds the 2-D one.  The 3-D
convolutions of Inception-I3D (conv3d.hip, conv3d_halo.hip) and the GEMMs of the bf16 tile engine follow the precision selector inside the block; the loop, the
accumulation and the hardening are test_util3d's own."""
from . import test_util3d as _T3
from .infer2d import PRECISIONS, _precision, inference_precision          # noqa: F401  (inference_precision: re-exported)
from .test_util3d import calculate_metric_percase                         # noqa: F401  (same module surface)


def test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type='segtran', num_classes=4,
                     precision='fp32'):
    """test_util3d.test_single_case with one more argument.  precision: 'fp32' (default) -- exactly that function's results -- or 'bf16x3' -- the same loop under
    torch.no_grad() inside inference_precision('bf16x3'); the setting the process had comes back at the end, also after an exception.  Any other name: ValueError."""
    with _precision(precision):
        return _T3.test_single_case(net, image, orig_patch_size, input_patch_size, batch_size, stride_xy, stride_z, task_name, net_type=net_type,
                                    num_classes=num_classes)


# reference function name; not a pytest test
test_single_case.__test__ = False
