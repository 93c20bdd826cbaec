"""GPU (-m gpu): Segtran2d on the ResNet backbones -- the train step of resnet34 and resnet101 against the reference fixtures (tests/golden/make_resnet_golden.py) on
both tile engines, the folded eval forward against the unfolded one, the three evaluation forms bit for bit, the trainer's loop with --bb, and the --nofeatup form
(do_pool1: the stem's max-pool) against a plain-torch restatement of the backbone."""
import glob
import os

import pytest
import torch
import torch.nn.functional as F

from segtran_amd import engine, functional as SF, infer2d, segx, train2d, train_common as tc
from test_gpu_model import _grads_vs_golden, REFEREE
from test_kernels_infer import rnd
from util import golden, assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SMALL = dict(dim=2, task='fundus', num_classes=3, translayers=1, compress=[1, 1], attractors=32, bs=2, size=(64, 96))
WINDOWS = dict(orig_input_size=(64, 96), patch_size=(64, 96), stride=(64, 48), task_name='fundus', num_classes=3)
SHAPE = (2, 3, 64, 144)                                      # two 64 x 96 windows that overlap in 48 columns


def _build(bb, **kw):
    return engine.build_model(SMALL, DEV, dropout_prob=0.0, attractors=32, backbone_type=bb, **kw)


@pytest.mark.parametrize('tile_engine', ['x6', 'f32'])
@pytest.mark.parametrize('bb', ['resnet34', 'resnet101'])
def test_segtran2d_resnet_train_step_vs_reference(bb, tile_engine):
    """3 classes, 1 layer, 32 attractors, 2 x 3 x 64 x 96 -> 8 x 12 tokens; the bars of test_gpu_oct_model.py, the gradients with the fp64 referee of test_gpu_model.py.
    The fixture stores how far the fp32 reference itself is from its fp64 twin: it must stay inside a quarter of every bar for the bars to mean anything."""
    L = segx.lib()
    prev = L.set_engine(tile_engine)
    try:
        g = golden('seg2d_%s_train' % bb)
        assert tuple(g['x'].shape) == (2, 3, 64, 96)
        assert float(g['ref32_vs_64_logit_err']) <= 0.25 * 1e-4 and float(g['ref32_vs_64_loss_err']) <= 0.25 * 5e-5 and float(g['ref32_vs_64_grad_err']) <= 0.25 * 2e-3
        net = _build(bb)
        net.train()
        y = net(g['x'].to(DEV))
        assert tuple(y.shape) == (2, 3, 64, 96)
        print('%s %s: |logits - reference| = %.3e of their scale' % (bb, tile_engine, (y.cpu() - g['logits']).abs().max().item() / g['logits'].abs().max().item()))
        assert_close(y, g['logits'], 1e-4, 'logits')
        safe = g['logits'].abs() > 1e-4
        assert torch.equal((y.cpu() > 0)[safe], g['labels'][safe]), 'hardened label map differs'
        nhot = engine.map_mask('fundus', g['mask'].to(DEV))
        assert torch.equal(nhot.cpu(), g['nhot'].float())
        pw, cw = engine.loss_weights('fundus', DEV)
        loss, _ = SF.seg_loss(y, nhot, pw, cw)
        print('%s %s: loss %.6f vs %.6f' % (bb, tile_engine, loss.item(), float(g['loss'])))
        assert abs(loss.item() - float(g['loss'])) < 5e-5
        loss.backward()
        _grads_vs_golden(net, g, tol=2e-3, referee=True)
        for k, v in net.state_dict().items():
            if k.endswith('num_batches_tracked'):
                assert int(v) == 1, k                                   # the deferred ticks reached every BatchNorm of the backbone
        L.team_check()
    finally:
        L.set_engine(prev)


@pytest.mark.parametrize('bb', ['resnet34', 'resnet101'])
def test_eval_forward_folded_vs_unfolded(bb, monkeypatch):
    """the bar of test_gpu_fold_fullshape.py (1e-3 absolute and 2e-4 of the largest logit), and no BatchNorm launch in the folded forward"""
    net = _build(bb).eval()
    x = rnd(2, 3, 64, 96, seed=71).to(DEV)
    with torch.no_grad():
        want = net(x)
    net.fold_batchnorm()
    assert net.batchnorm_folded
    calls = []
    real = type(segx.lib()).bn_act_fwd2
    monkeypatch.setattr(type(segx.lib()), 'bn_act_fwd2', lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    y = net(x)                                              # grad mode on: the folded forward builds no graph by itself
    assert not calls, 'the folded forward launched BatchNorm %d times' % len(calls)
    assert not y.requires_grad and torch.isfinite(y).all()
    err, absmax = (y - want).abs().max().item(), want.abs().max().item()
    print('%s folded: |folded - unfolded| = %.3e (absmax %.3e)' % (bb, err, absmax))
    assert err < 1e-3 and err <= 2e-4 * absmax
    net.unfold_batchnorm()
    with torch.no_grad():
        assert torch.equal(net(x), want) and calls


def test_three_evaluation_forms_are_bit_identical_with_resnet34():
    net = _build('resnet34').eval()
    x = rnd(*SHAPE, seed=81).to(DEV)
    want_hard, want_soft = infer2d.test_single_batch(net, x, fused=False, **WINDOWS)
    assert tuple(want_soft.shape) == (2, 3, 64, 144) and want_hard.dtype == torch.int32
    hard, soft = infer2d.test_single_batch(net, x, fused=True, window_batch=1, **WINDOWS)
    assert torch.equal(hard, want_hard) and torch.equal(soft, want_soft)
    g = infer2d.GraphedSlidingWindow(net, SHAPE, WINDOWS['orig_input_size'], WINDOWS['patch_size'], WINDOWS['stride'], 3, fold_bn=False, window_batch=1)
    try:
        hard, soft = g(x)
        assert torch.equal(hard, want_hard) and torch.equal(soft, want_soft)
    finally:
        g.close()
    # folded: the graph equals the folded loop
    fold_hard, fold_soft = infer2d.test_single_batch(net, x, fused=True, window_batch=1, fold_bn=True, **WINDOWS)
    assert not net.batchnorm_folded
    assert not torch.equal(fold_soft, want_soft)                 # another operation order: the folded forward really ran
    g = infer2d.GraphedSlidingWindow(net, SHAPE, WINDOWS['orig_input_size'], WINDOWS['patch_size'], WINDOWS['stride'], 3, fold_bn=True, window_batch=1)
    try:
        hard, soft = g(x)
        assert torch.equal(hard, fold_hard) and torch.equal(soft, fold_soft)
    finally:
        g.close()
    assert not net.batchnorm_folded


def test_two_trainer_iterations_with_bb_resnet34(tmp_path, monkeypatch):
    """python -m segtran_amd.train2d --bb resnet34 ..., two iterations in this process; the checkpoint reloads strictly into a fresh --bb resnet34 net and is refused by
    --bb eff-b4"""
    work = tmp_path / 'work'
    work.mkdir()
    monkeypatch.chdir(work)
    argv = ['--bb', 'resnet34', '--task', 'fundus', '--patch', '64,96', '--synthweights', '--maxiter', '2', '--bs', '2', '--attractors', '32', '--logiter', '1']
    net = train2d.main(argv)
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert int(net.backbone.layer4[2].bn2.num_batches_tracked) == 2
    saved = glob.glob(os.path.join(str(tmp_path), 'model', 'segtran-fundus-*', 'iter_2.pth'))
    assert len(saved) == 1
    ck = torch.load(saved[0], map_location='cpu')
    assert ck['iter_num'] == 2 and ck['args']['backbone_type'] == 'resnet34'
    args, cfg = train2d.parse_args(argv)
    fresh = engine.build_model(cfg, 'cpu', attractors=32, synth=False, **tc.arch_overrides(args))
    assert tc.load_model(fresh, args, saved[0]) == 2
    assert fresh.load_state_dict(ck['model'], strict=True).missing_keys == []
    assert torch.equal(fresh.backbone.layer2[0].downsample[0].weight, net.backbone.layer2[0].downsample[0].weight.cpu())
    eff_args, eff_cfg = train2d.parse_args([a if a != 'resnet34' else 'eff-b4' for a in argv])
    eff = engine.build_model(eff_cfg, 'cpu', attractors=32, synth=False, **tc.arch_overrides(eff_args))
    with pytest.raises(SystemExit, match=r'args\[backbone_type\]=eff-b4, checkpoint args\[backbone_type\]=resnet34'):
        tc.load_model(eff, eff_args, saved[0])


def _backbone_restated(bb, x):
    """ext_features of the reference (resnet.py:186-200, blocks :42-69) in plain torch on the parameters of `bb` (BasicBlock only), with do_pool1"""
    def conv(c, u):
        return F.conv2d(u, c.weight, None, c.stride, c.padding)

    def bn(m, u):
        return F.batch_norm(u, m.running_mean, m.running_var, m.weight, m.bias, m.training, m.momentum, m.eps)
    x0 = F.relu(bn(bb.bn1, conv(bb.conv1, x)))
    feats = [F.max_pool2d(x0, 3, 2, 1) if bb.do_pool1 else x0]
    for layer in (bb.layer1, bb.layer2, bb.layer3, bb.layer4):
        cur = feats[-1]
        for blk in layer:
            sc = cur if blk.downsample is None else bn(blk.downsample[1], conv(blk.downsample[0], cur))
            out = F.relu(bn(blk.bn1, conv(blk.conv1, cur)))
            cur = F.relu(bn(blk.bn2, conv(blk.conv2, out)) + sc)
        feats.append(cur)
    return feats


def _vs_restatement(got, w32, w64, tol, scale, what):
    """the project's referee rule (test_gpu_model._grads_vs_golden): within tol of the fp32 restatement, or at most REFEREE x as far from the fp64 restatement as
    the fp32 one is (a BatchNorm over the 12 values of a 2 x 3 plane pair amplifies rounding on either side)"""
    got, w32, w64 = got.detach().cpu().double(), w32.detach().double(), w64.detach()
    e32, e64, r64 = [(a - b).abs().max().item() / scale for a, b in ((got, w32), (got, w64), (w32, w64))]
    assert e32 <= tol or e64 <= REFEREE * r64, '%s: |hip - fp32| %.2e, |hip - fp64| %.2e, |fp32 - fp64| %.2e of the scale' % (what, e32, e64, r64)


def test_nofeatup_backbone_forward_and_backward_vs_plain_torch():
    """--nofeatup: do_pool1, the stem's max-pool on zero padding.  The backbone of a --nofeatup resnet34 net at 64 x 96, train mode, against its restatement on ATen's
    CPU kernels in fp32 (tolerances of tests/test_kernels_backbone.py: 3e-5 of the scale forward, 1e-4 backward) with the same restatement in fp64 as referee, and
    the whole model runs forward and backward."""
    import copy
    net = _build('resnet34', bb_feat_upsize=False)
    assert net.backbone.do_pool1
    net.train()
    ref = copy.deepcopy(net.backbone).cpu()
    ref64 = copy.deepcopy(ref).double()
    x0 = rnd(2, 3, 64, 96, seed=91).cpu()
    feats = net.backbone.ext_features(x0.to(DEV))
    want, want64 = _backbone_restated(ref, x0), _backbone_restated(ref64, x0.double())
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 16, 24), (64, 16, 24), (128, 8, 12), (256, 4, 6), (512, 2, 3)]
    for i, (f, w, w64) in enumerate(zip(feats, want, want64)):
        _vs_restatement(f, w, w64, 3e-5, w64.abs().max().item(), 'feature %d' % i)
    gs = [rnd(*w.shape, seed=92 + i).cpu() for i, w in enumerate(want)]
    sum((f * g.to(DEV)).sum() for f, g in zip(feats, gs)).backward()
    sum((w * g).sum() for w, g in zip(want, gs)).backward()
    sum((w * g.double()).sum() for w, g in zip(want64, gs)).backward()
    got, exp, exp64 = dict(net.backbone.named_parameters()), dict(ref.named_parameters()), dict(ref64.named_parameters())
    scale = max(p.grad.abs().max().item() for k, p in exp64.items() if p.grad is not None)
    n = 0
    for k, p in exp.items():
        if p.grad is None:
            assert got[k].grad is None, k                               # fc
            continue
        _vs_restatement(got[k].grad, p.grad, exp64[k].grad, 1e-4, scale, k)
        n += 1
    assert n == 108
    # the whole --nofeatup model: H / 16 tokens
    net.zero_grad()
    y = net(x0.to(DEV))
    assert tuple(y.shape) == (2, 3, 64, 96) and tuple(net.orig_feat_shape) == (4, 6)
    y.square().mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None) and net.backbone.conv1.weight.grad.abs().max() > 0
