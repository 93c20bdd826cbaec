"""GPU (-m gpu): the fused sliding-window evaluation captured as one hipGraph (infer2d.GraphedSlidingWindow) against the eager evaluation, bit for bit; the
lifecycle checks of the captured object; one captured run at the cfg1 product shape."""
import pytest
import torch

from segtran_amd import engine, infer2d
from test_kernels_infer import rnd
from test_sliding_fused import small_net, SMALL

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SHAPE = (2, 3, 96, 80)


def _graphed(net, **kw):
    return infer2d.GraphedSlidingWindow(net, SHAPE, SMALL['orig_input_size'], SMALL['patch_size'], SMALL['stride'], SMALL['num_classes'], **kw)


@pytest.mark.parametrize('fold_bn', [False, True])
def test_replays_equal_the_eager_evaluation_on_three_images(fold_bn):
    """window_batch=1: the captured forwards have the eager path's batch size, so every replay gives the eager bits; the second and third image show that the
    static input is refreshed and the static outputs rewritten"""
    net = small_net(DEV)
    g = _graphed(net, window_batch=1, fold_bn=fold_bn)
    assert net.batchnorm_folded == fold_bn
    seen = []
    for i in range(3):
        x = rnd(*SHAPE, seed=70 + i).to(DEV)
        hard, soft = g(x)
        want_hard, want_soft = infer2d.test_single_batch(net, x, fold_bn=fold_bn, fused=False, **SMALL)
        assert hard.dtype == torch.int32 and torch.equal(hard, want_hard) and torch.equal(soft, want_soft), 'image %d' % i
        seen.append(soft.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert g.replays == 3
    g.close()
    assert not net.batchnorm_folded


def test_lifecycle():
    net = small_net(DEV)
    x = rnd(*SHAPE, seed=73).to(DEV)
    net.train()
    with pytest.raises(RuntimeError, match='eval'):
        _graphed(net)
    net.eval()
    assert not net.batchnorm_folded
    g = _graphed(net, fold_bn=True)
    assert net.batchnorm_folded
    g(x)
    net.train()
    with pytest.raises(RuntimeError, match='train mode'):
        g(x)
    net.eval()                                              # train() dropped the fold: the captured kernels read operands that are no longer the net's
    with pytest.raises(RuntimeError, match='fold'):
        g(x)
    g.close()
    assert not net.batchnorm_folded                        # as before construction
    with pytest.raises(RuntimeError, match='closed'):
        g(x)

    g = _graphed(net, fold_bn=True)
    g(x)
    bn = next(m for m in net.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d))
    with torch.no_grad():
        bn.running_var.mul_(1.5)                            # an in-place edit of a folded tensor: the fold's version check sees it
    with pytest.raises(RuntimeError, match='fold'):
        g(x)
    g.close()
    assert not net.batchnorm_folded

    net.fold_batchnorm()                                    # a net the caller folded stays folded
    g = _graphed(net, fold_bn=True)
    g(x)
    with pytest.raises(ValueError, match='captured for'):
        g(x[:1])
    g.close()
    assert net.batchnorm_folded


def test_captured_product_shape_equals_the_fused_eager_run():
    """cfg1 at batch 2: 256 x 256 model, 576 x 576 image, stride 128 -- ceil(320 / 128) + 1 = 4 origins per axis (0, 128, 256 and the clamped 320), 16 windows.
    The windows are stacked as far as the library allows: its per-plane kernels take at most 65535 (sample, channel) planes and EfficientNet-B4 widens to 2688
    channels, so one forward holds 24 samples = 12 windows and the 16 windows run as 12 + 4.  The same kernels on the same batches: the same bits."""
    cfg = dict(engine.CONFIGS['cfg1'], size=(256, 256))
    net = engine.build_model(cfg, DEV, dropout_prob=0.0).eval()
    kw = dict(orig_input_size=(256, 256), patch_size=(256, 256), stride=(128, 128))
    x = rnd(2, 3, 576, 576, seed=74).to(DEV)
    assert infer2d.max_stacked_samples(net) == 24
    g = infer2d.GraphedSlidingWindow(net, x.shape, num_classes=cfg['num_classes'], **kw)
    assert g.plan.table.nwin == 16 and g.plan.window_batch == 12
    hard, soft = g(x)
    want_hard, want_soft = infer2d.test_single_batch(net, x, task_name='fundus', num_classes=cfg['num_classes'], fold_bn=True, fused=True, **kw)
    assert torch.equal(hard, want_hard) and torch.equal(soft, want_soft)
    g.close()
