"""GPU (-m gpu): the eval forward with BatchNorm folded into the backbone's kernels (Segtran2d.fold_batchnorm) at the BASELINE shapes, held to the assertions the
unfolded forward is held to (tests/test_gpu_fullshape.py::test_fullshape_eval_every_label, tests/test_gpu_model.py::test_eval_path_2d_vs_reference) against the same
reference-generated fixtures; its replay from a captured graph; and the fold's lifecycle on the whole model."""
import numpy as np
import pytest
import torch

from segtran_amd import engine, functional as SF, segx
from segtran_amd.synth import sample
from util import golden, assert_close
from test_gpu_fullshape import _inputs, _case, engine_sel, LABEL_MARGIN      # noqa: F401  (engine_sel: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.mark.parametrize('engine_sel', ['x6', 'f32'], indirect=True)
@pytest.mark.parametrize('case', ['cfg2', 'cfg3', 'cfg2_b2'])
def test_fullshape_eval_every_label_folded(case, engine_sel, monkeypatch):
    cfg, B, tag = _case(case)
    g = golden(tag)
    net = engine.build_model(cfg, DEV, dropout_prob=0.0)
    net.eval()
    net.fold_batchnorm()
    assert net.batchnorm_folded
    calls = []
    real = type(segx.lib()).bn_act_fwd2
    monkeypatch.setattr(type(segx.lib()), 'bn_act_fwd2', lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    x, _ = _inputs(cfg, B)
    y = net(x.to(DEV))                                      # grad mode on: the folded forward builds no graph by itself
    assert not calls, 'the folded forward launched BatchNorm %d times' % len(calls)
    assert not y.requires_grad
    y = y.cpu()
    assert list(y.shape) == g['shape'].tolist()
    absmax = float(g['absmax'])
    err = (sample(y, 65536)[::4] - g['logits']).abs().max().item()
    print('%s %s folded: |logits - reference| = %.3e (absmax %.3e)' % (case, engine_sel, err, absmax))
    assert err < 1e-3 and err <= 2e-4 * absmax, 'logits differ from the reference by %.3e' % err
    ref_bits = np.unpackbits(g['labels'].numpy())[:y.numel()].astype(bool)
    got_bits = (y > 0).numpy().reshape(-1)
    bad = np.nonzero(ref_bits != got_bits)[0]
    uncertain = set(g['near_idx'].numpy()[np.abs(g['near_val'].numpy()) < LABEL_MARGIN].tolist())
    outside = [int(i) for i in bad if int(i) not in uncertain]
    assert not outside, '%d hardened labels differ where the reference |logit| >= %g (first: %s)' % (len(outside), LABEL_MARGIN, outside[:5])
    near = g['near_idx'].long()
    assert (y.reshape(-1)[near] - g['near_val']).abs().max().item() < 2e-5


def test_eval_path_2d_folded_vs_reference():
    from segtran_amd import infer2d as T2                    # test_util2d's functions with the fold_bn switch
    g = golden('eval2d')
    net = engine.build_model(dict(engine.CONFIGS['cfg1'], size=(64, 64)), DEV, dropout_prob=0.0, attractors=int(g['A']))
    net.eval()
    for tag in 'ab':
        cfg = [int(v) for v in g['cfg_' + tag]]
        hard, soft = T2.test_single_batch(net, g['x_' + tag].to(DEV), tuple(cfg[0:2]), tuple(cfg[2:4]), tuple(cfg[4:6]), 'fundus', 3, fold_bn=True)
        assert not net.batchnorm_folded                      # folded for the call only
        assert hard.dtype == torch.int32 and hard.shape == g['hard_' + tag].shape
        assert_close(soft.cpu(), g['soft_' + tag], 1e-5, 'soft ' + tag)
        safe = (g['soft_' + tag] - 0.5).abs() > 1e-5
        assert torch.equal(hard.cpu()[safe], g['hard_' + tag].int()[safe]), 'hardened label map differs'
    net.fold_batchnorm()
    cfg = [int(v) for v in g['cfg_a']]
    T2.test_single_batch(net, g['x_a'].to(DEV), tuple(cfg[0:2]), tuple(cfg[2:4]), tuple(cfg[4:6]), 'fundus', 3, fold_bn=True)
    assert net.batchnorm_folded                              # a net the caller folded stays folded


def test_folded_eval_forward_replays_from_a_captured_graph():
    """one stream, no parallel branch, default queue settings: the replay gives the eager folded result bit for bit"""
    c = dict(engine.CONFIGS['cfg2'], size=(128, 128))
    net = engine.build_model(c, DEV, dropout_prob=0.0, attractors=64)
    net.eval().fold_batchnorm()
    x, _ = engine.synth_batch(c, 2, DEV)
    with torch.no_grad():
        eager = net(x).clone()
        xs = x.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(xs)                                          # warm-up on the capture stream: every workspace size is planned before the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(xs)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_train_step_after_a_dropped_fold_equals_the_never_folded_twin():
    c = dict(engine.CONFIGS['cfg2'], size=(64, 64))
    x, raw = engine.synth_batch(c, 2, DEV)
    res = []
    for fold_first in (True, False):
        torch.manual_seed(0)
        net = engine.build_model(c, DEV, dropout_prob=0.0, attractors=32)
        if fold_first:
            net.eval().fold_batchnorm()
            with torch.no_grad():
                net(x)
        net.train()
        assert not net.batchnorm_folded
        SF.manual_seed(3)
        y = net(x)
        pw, cw = engine.loss_weights('fundus', DEV)
        loss, _ = SF.seg_loss(y, engine.map_mask('fundus', raw), pw, cw)
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, {n: b.clone() for n, b in net.named_buffers()}))
    (la, ga, ba), (lb, gb, bb) = res
    assert torch.equal(la, lb) and sorted(ga) == sorted(gb) and len(ga) > 100
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for n in ba:
        assert torch.equal(ba[n], bb[n]), n
