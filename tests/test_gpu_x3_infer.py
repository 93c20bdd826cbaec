"""GPU (-m gpu): the folded 2-D eval forward and the sliding-window evaluation under precision='bf16x3' (three-term bf16 GEMMs) at the small
fixture sizes: the reference fixture's logits within the project's parity bar of 1e-3, its hardened maps wherever it is decided by more than that, the captured
graph against the eager path bit for bit, and no setting left behind."""
import pytest
import torch

from segtran_amd import engine, infer2d, segx
from test_kernels_infer import rnd
from test_sliding_fused import small_net, SMALL
from util import golden

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BAR = 1e-3                             # README: logits within 1e-3 of the reference


@pytest.mark.parametrize('tag,cfg', [('seg2d_cfg1_eval', 'cfg1'), ('seg2d_cfg2_eval', 'cfg2')])
def test_folded_eval_forward_meets_the_parity_bar_in_three_terms(tag, cfg):
    g = golden(tag)
    L = segx.lib()
    net = engine.build_model(dict(engine.CONFIGS[cfg], size=(64, 64)), DEV, dropout_prob=0.0, attractors=int(g['A'])).eval()
    net.fold_batchnorm()
    x = g['x'].to(DEV)
    with torch.no_grad():
        y6 = net(x)
        L.x6_launches(); L.x3_launches()
        with infer2d.inference_precision('bf16x3'):
            y3 = net(x)
        n6, n3 = L.x6_launches(), L.x3_launches()
        y6b = net(x)
    want, labels = g['logits'], g['labels']
    err = (y3.cpu() - want).abs().max().item()
    print('%s: %d of %d bf16 tile-engine launches ran three-term; max |y3 - fixture| %.3e, max |y6 - fixture| %.3e, max |y3 - y6| %.3e'
          % (tag, n3, n6, err, (y6.cpu() - want).abs().max().item(), (y3 - y6).abs().max().item()))
    assert n3 > 0 and n3 <= n6
    assert not torch.equal(y3, y6), 'the three-term forward gave the six-term bits: the mode was not on'
    assert torch.equal(y6b, y6), 'the six-term forward after the block differs from the one before it'
    assert err < BAR
    decided = want.abs() >= BAR
    assert torch.equal((y3.cpu() > 0)[decided], labels[decided]), 'a hardened label differs where the fixture is decided by more than the bar'
    excused = ((y3.cpu() > 0) != labels) & ~decided
    assert excused.float().mean().item() <= (~decided).float().mean().item()


def test_sliding_window_in_three_terms_eager_and_captured():
    """96 x 96 image, 64 x 64 windows at stride 32 (2 x 2 windows); window_batch=1: the captured forwards are the eager ones"""
    net = small_net(DEV)
    L = segx.lib()
    shape = (2, 3, 96, 96)
    x = rnd(*shape, seed=81).to(DEV)
    before = infer2d.test_single_batch(net, x, fold_bn=True, fused=True, window_batch=1, **SMALL)
    L.x3_launches()
    hard, soft = infer2d.test_single_batch(net, x, fold_bn=True, fused=True, window_batch=1, precision='bf16x3', **SMALL)
    assert L.x3_launches() > 0 and not torch.equal(soft, before[1])
    assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    g = infer2d.GraphedSlidingWindow(net, shape, SMALL['orig_input_size'], SMALL['patch_size'], SMALL['stride'], SMALL['num_classes'], window_batch=1,
                                     precision='bf16x3')
    assert g.precision == 'bf16x3' and g.plan.table.nwin == 4 and L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    h1, s1 = (t.clone() for t in g(x))
    L.x3_launches()
    h2, s2 = g(x)
    assert L.x3_launches() == 0                            # a replay launches through the graph: the route was fixed at capture
    assert torch.equal(h1, hard) and torch.equal(s1, soft) and torch.equal(h2, h1) and torch.equal(s2, s1)
    g.close()
    assert not net.batchnorm_folded and L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    after = infer2d.test_single_batch(net, x, fold_bn=True, fused=True, window_batch=1, **SMALL)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]), 'the three-term mode leaked into a later six-term evaluation'
    with pytest.raises(ValueError):
        infer2d.GraphedSlidingWindow(net, shape, SMALL['orig_input_size'], SMALL['patch_size'], SMALL['stride'], SMALL['num_classes'], precision='tf32')
