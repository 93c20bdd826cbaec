"""CPU: the ResNet backbones of Segtran2d on the host side (no kernels run) -- state_dict parity with the reference, the refusals, the `--bb` flag on its way to the
model builder and into checkpoints, and the lifecycle of the BatchNorm fold."""
import argparse
import os

import pytest
import torch

from segtran_amd import engine, resnet, train2d, train_common as tc
from segtran_amd.networks import segtran2d
from test_fold_batchnorm import _randomize_bn
from util import golden_json

SMALL = dict(dim=2, task='fundus', num_classes=3, translayers=1, compress=[1, 1], attractors=32, bs=2, size=(64, 96))


def _build(bb, **kw):
    return engine.build_model(SMALL, 'cpu', attractors=32, synth=False, backbone_type=bb, **kw)


@pytest.mark.parametrize('bb', ['resnet34', 'resnet50', 'resnet101'])
def test_state_dict_keys_and_shapes_equal_the_reference(bb):
    want = golden_json('state_dict_keys_resnet')[bb]
    sd = _build(bb).state_dict()
    own = {k: list(v.shape) for k, v in sd.items()}
    derived = {k for k in want if '.pos_coder.all_' in k}             # the reference's index buffers (not built here, dropped by load_model)
    assert set(own) == set(want) - derived, (sorted(set(want) - derived - set(own))[:5], sorted(set(own) - set(want))[:5])
    assert all(own[k] == want[k] for k in own), [k for k in own if own[k] != want[k]][:5]
    assert sum(k.startswith('backbone.') for k in own) == {'resnet34': 218, 'resnet50': 320, 'resnet101': 626}[bb]
    assert 'backbone.fc.weight' in own and 'backbone.layer4.2.bn2.num_batches_tracked' in own and sd['backbone.bn1.num_batches_tracked'].dtype == torch.int64


def test_initialisation_follows_the_reference():
    """resnet.py:149-155: normal(0, sqrt(2 / (k * k * out_channels))) for every convolution, BatchNorm weight 1 and bias 0"""
    torch.manual_seed(0)
    net = resnet.resnet34(do_pool1=False)
    w = net.layer3[1].conv2.weight
    assert abs(w.std().item() / (2.0 / (9 * 256)) ** 0.5 - 1) < 0.02 and abs(w.mean().item()) < 1e-3
    assert all(torch.equal(m.weight, torch.ones_like(m.weight)) and not m.bias.any() for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert not net.do_pool1 and resnet.resnet50().do_pool1
    assert [len(l) for l in (net.layer1, net.layer2, net.layer3, net.layer4)] == [3, 4, 6, 3]
    assert [len(l) for l in (resnet.resnet101().layer3,)] == [23]


@pytest.mark.parametrize('bb', ['resnet18', 'effv2m', 'resibn101', 'resnet152'])
def test_unbuilt_backbones_raise(bb):
    with pytest.raises(NotImplementedError, match=bb):
        _build(bb)


def test_unbuilt_parts_of_the_reference_file_raise():
    for ctor in (resnet.resnet18, resnet.resnet152, resnet.resibn101):
        with pytest.raises(NotImplementedError, match='not built'):
            ctor()
    with pytest.raises(NotImplementedError, match='lens'):
        resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1], lens_stage='res4')
    with pytest.raises(NotImplementedError, match='ext_features'):
        resnet.resnet34()(torch.zeros(1, 3, 32, 32))


def test_pretrained_weights_come_from_a_local_file_or_fail_loudly(tmp_path, monkeypatch):
    monkeypatch.delenv('SEGX_PRETRAINED_DIR', raising=False)
    with pytest.raises(RuntimeError, match=r'pretrained.*resnet34-333f7ec4\.pth.*--nopretrain.*--synthweights'):
        _build('resnet34', use_pretrained=True)
    monkeypatch.setenv('SEGX_PRETRAINED_DIR', str(tmp_path))
    with pytest.raises(RuntimeError, match=r'pretrained weights not found.*resnet101-5d3b4d8f\.pth.*--nopretrain.*--synthweights'):
        _build('resnet101', use_pretrained=True)
    assert resnet.PRETRAINED_FILES['resnet50'] == 'resnet50-19c8e357.pth'
    torch.manual_seed(1)
    src = resnet.resnet34()
    sd = {k: v for k, v in src.state_dict().items() if not k.startswith('fc.')}      # strict=False, as the reference loads it
    torch.save(sd, os.path.join(str(tmp_path), resnet.PRETRAINED_FILES['resnet34']))
    net = _build('resnet34', use_pretrained=True)
    assert torch.equal(net.backbone.conv1.weight, src.conv1.weight) and torch.equal(net.backbone.layer4[2].bn2.running_var, src.layer4[2].bn2.running_var)
    assert net.backbone.do_pool1 is False and _build('resnet34', bb_feat_upsize=False).backbone.do_pool1 is True


def _parse(argv, dim=2):
    p = tc.common_flags(argparse.ArgumentParser(), dim)
    return tc.finalize_args(p.parse_args(argv), dim)


def test_bb_flag_reaches_the_model_builder_and_the_checkpoint(tmp_path):
    a = _parse(['--bb', 'resnet50', '--translayers', '1', '--attractors', '32'])
    assert a.backbone_type == 'resnet50' and tc.arch_overrides(a)['backbone_type'] == 'resnet50'
    assert _parse([]).backbone_type == 'eff-b4' and tc.arch_overrides(_parse([]))['backbone_type'] == 'eff-b4'     # train2d.py:171
    assert not hasattr(_parse([], 3), 'backbone_type')                                                             # 3-D stays on 'i3d'
    with pytest.raises(SystemExit):
        _parse(['--bb', 'resnet50'], 3)
    args, cfg = train2d.parse_args(['--bb', 'resnet50', '--patch', '64,96', '--translayers', '1', '--attractors', '32'])
    net = engine.build_model(cfg, 'cpu', attractors=32, synth=False, **tc.arch_overrides(args))
    assert isinstance(net.backbone, resnet.ResNet) and isinstance(net.backbone.layer1[0], resnet.Bottleneck) and net.bb_feat_dims == [64, 256, 512, 1024, 2048]
    path = tc.save_model(net, args, str(tmp_path), 3)
    ck = torch.load(path, map_location='cpu')
    assert ck['args']['backbone_type'] == 'resnet50'
    assert tc.load_model(net, args, path) == 3
    other, _ = train2d.parse_args(['--bb', 'resnet101', '--patch', '64,96', '--translayers', '1', '--attractors', '32'])
    with pytest.raises(SystemExit, match=r'args\[backbone_type\]=resnet101, checkpoint args\[backbone_type\]=resnet50, inconsistent'):
        tc.load_model(net, other, path)
    for bad in ('resnet18', 'effv2m', 'resibn101'):
        with pytest.raises(SystemExit, match='--bb ' + bad):
            train2d.parse_args(['--bb', bad])


def test_tunebn_refuses_a_resnet_as_the_reference_does():
    """train2d.py:1089-1100: --tunebn walks the EfficientNet blocks; any other backbone prints 'not supported' and exits"""
    with pytest.raises(SystemExit, match="Backbone 'resnet34' not supported"):
        train2d.parse_args(['--tunebn', '--bb', 'resnet34', '--cp', 'x.pth'])
    with pytest.raises(SystemExit, match="Backbone 'resnet34' not supported"):
        tc.set_tune_bn_mode(_build('resnet34'))
    assert train2d.parse_args(['--tunebn', '--cp', 'x.pth'])[0].tune_bn_only


@pytest.mark.parametrize('bb', ['resnet34', 'resnet50'])
def test_fold_lifecycle(bb):
    """host side only (no kernel runs): state_dict untouched, train mode refused, train() / load_state_dict() / an in-place change of a source tensor drop the fold"""
    import segtran_amd
    net = _build(bb)
    _randomize_bn(net.backbone, 9)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(RuntimeError, match='eval'):
        net.fold_batchnorm()
    assert not net.batchnorm_folded
    net.eval()
    assert segtran_amd.fold_batchnorm(net) is net and net.batchnorm_folded
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any('fold' in n for n, _ in list(net.named_parameters()) + list(net.named_buffers()))
    # the fold algebra against fp64 on the host, and the closing bias b_last + b_down summed once
    bb_ = net.backbone
    (ws, bs, _), blocks = bb_._folded[:2]
    assert len(blocks) == sum(len(l) for l in (bb_.layer1, bb_.layer2, bb_.layer3, bb_.layer4))

    def fold64(conv, bn):
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return (conv.weight.detach().double() * s.view(-1, 1, 1, 1)).float(), (bn.bias.detach().double() - bn.running_mean.double() * s).float()
    w, b = fold64(bb_.conv1, bb_.bn1)
    assert torch.equal(ws, w) and torch.equal(bs, b) and not ws.requires_grad and not isinstance(ws, torch.nn.Parameter)
    first2 = len(bb_.layer1)                                           # layer2[0]: a down-sample path at stride 2
    blk = bb_.layer2[0]
    main, down, b_close = blocks[first2]
    pairs = blk._pairs()
    for (wf, bf, _), (conv, bn) in zip(main, pairs):
        w, b = fold64(conv, bn)
        assert torch.equal(wf, w) and torch.equal(bf, b)
    wd, bd = fold64(blk.downsample[0], blk.downsample[1])
    assert torch.equal(down[0], wd) and torch.equal(b_close, main[-1][1] + bd)
    plain = blocks[first2 + 1]                                         # no down-sample path: b_down = 0
    assert plain[1] is None and torch.equal(plain[2], plain[0][-1][1])
    net.train()
    assert not net.batchnorm_folded
    net.eval().fold_batchnorm()
    net.load_state_dict(before)
    assert not net.batchnorm_folded
    net.fold_batchnorm()
    with torch.no_grad():
        bb_.layer3[1].bn2.running_var.mul_(2.0)                        # a source tensor changed in place: the folded operands are stale
    assert not net.batchnorm_folded
    net.fold_batchnorm()
    net.float()                                                        # _apply
    assert not net.batchnorm_folded
    net.fold_batchnorm().unfold_batchnorm()
    assert not net.batchnorm_folded
