"""Golden fixtures of Segtran2d on the ResNet backbones (`--bb resnet34|resnet50|resnet101`) from the REAL reference:
  state_dict_keys_resnet.json                        names and shapes of the reference Segtran2d for the three backbone types
  seg2d_resnet34_train.npz, seg2d_resnet101_train.npz  one dropout-free train-mode step (resnet50 shares the Bottleneck with resnet101: no fixture of its own)

Runs only where the reference checkout exists (as make_golden.py, whose helpers it uses); only inputs and outputs of the reference's own modules are stored.
Name-hashed synthetic weights (load_synth), 3 classes, 1 transformer layer, 32 attractors, a 2 x 3 x 64 x 96 batch (8 x 12 tokens).  Stored: logits, hardened labels,
loss, gscale, sub-sampled gradients (segtran_amd.synth.sample) and the same run of the same reference modules in fp64 as referee (logits64, loss64, grad64:*), with the
fp32-reference-vs-fp64 distances (ref32_vs_64_*).  oracle/ has no ResNet forward: make_golden's "the oracle reproduces the reference" step is skipped here.

The GPU tests hold the product to logits 1e-4 of their scale, loss 5e-5 and gradients 2e-3 of gscale.  Those bars mean something only while the fp32 reference itself
stays well inside them against fp64 (at 64 x 96, layer4 normalises 48 samples per channel in train mode): where a distance exceeds a QUARTER of its bar the input is
enlarged (96 x 128, then 128 x 192) until it does not; the distances are printed and stored.
Usage:  python tests/golden/make_resnet_golden.py [keys] [resnet34] [resnet101]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402
from make_golden import R, O                               # noqa: E402
from segtran_amd.synth import load_synth, sample, synth_fundus_mask   # noqa: E402

TYPES = ('resnet34', 'resnet50', 'resnet101')
SIZES = ((64, 96), (96, 128), (128, 192))
BARS = dict(logits=1e-4, loss=5e-5, grads=2e-3)            # tests/test_gpu_resnet_model.py (the bars of test_gpu_oct_model.py)
HEAD_KEYS = ['out_conv.weight', 'out_conv.bias', 'out_fpn_bridgeconv.weight', 'out_fpn12_conv.weight', 'out_fpn23_conv.weight', 'out_gn2b.weight', 'out_gn3b.bias',
             'in_fpn34_conv.weight', 'in_gn4b.weight', 'voxel_fusion.pos_code_layer.pos_coder.pos_fc.weight', 'voxel_fusion.translayers.0.attractors',
             'voxel_fusion.translayers.0.in_ator_trans.query.weight', 'voxel_fusion.translayers.0.ator_out_trans.out_trans.first_linear.weight',
             'voxel_fusion.translayers.0.ator_out_trans.out_trans.output.group_linear.weight']
BACKBONE_KEYS = ['backbone.conv1.weight', 'backbone.bn1.weight', 'backbone.bn1.bias', 'backbone.layer1.0.conv1.weight', 'backbone.layer1.0.bn2.bias',
                 'backbone.layer1.0.downsample.0.weight', 'backbone.layer1.2.conv2.weight', 'backbone.layer2.0.conv2.weight', 'backbone.layer2.0.downsample.0.weight',
                 'backbone.layer2.0.downsample.1.weight', 'backbone.layer2.3.bn1.weight', 'backbone.layer3.0.conv1.weight', 'backbone.layer3.5.conv2.weight',
                 'backbone.layer3.5.conv3.weight', 'backbone.layer3.22.bn3.weight', 'backbone.layer4.0.downsample.0.weight', 'backbone.layer4.0.bn1.bias',
                 'backbone.layer4.2.conv1.weight', 'backbone.layer4.2.bn2.weight', 'backbone.layer4.2.bn3.bias']


def build(bb):
    return R.ref_segtran2d(num_classes=3, num_attractors=32, num_translayers=1, compress=(1, 1), backbone_type=bb, dropout_prob=0)


def case_keys():
    out = {}
    for bb in TYPES:
        net = build(bb)
        out[bb] = {k: list(v.shape) for k, v in net.state_dict().items()}
        print('  %s: %d entries, %d of the backbone' % (bb, len(out[bb]), sum(k.startswith('backbone.') for k in out[bb])))
    path = os.path.join(mg.OUT_DIR, 'state_dict_keys_resnet.json')
    json.dump(out, open(path, 'w'), indent=0, sort_keys=True)
    print('  wrote state_dict_keys_resnet.json (%.0f KB)' % (os.path.getsize(path) / 1024))


def _step(net, x, nhot, pw):
    y = R.quiet(net, x)
    loss = O.seg_loss(y, nhot, pw)[0]                      # composition restated; pinned by make_golden.case_loss
    loss.backward()
    return y.detach(), loss.detach(), dict(net.named_parameters())


def run_train(bb, H, W):
    """-> (arrays, the three distances as fractions of their bars)"""
    B, A = 2, 32
    net = build(bb)
    sd = load_synth(net)
    net.train()
    g = torch.Generator().manual_seed(16)
    x = torch.randn(B, 3, H, W, generator=g)
    mask = synth_fundus_mask(B, H, 1338, S2=W)
    nhot = O.fundus_map_mask(mask)
    pw = O.bce_pos_weight([0., 1., 2.])
    y, loss, rg = _step(net, x, nhot, pw)
    net64 = build(bb)
    net64.load_state_dict(sd)
    net64 = net64.double()
    mg._force_double_inputs(net64)
    net64.train()
    y64, loss64, rg64 = _step(net64, x.double(), nhot.double(), pw.double())
    gscale = max(p.grad.abs().max().item() for p in rg.values() if p.grad is not None)
    arrs = dict(x=x, mask=mask, logits=y, labels=(y > 0), loss=loss, margin=y.abs().min(), A=np.array(A), train=np.array(1), nhot=nhot.to(torch.uint8),
                logits64=sample(y64, 8192), loss64=loss64, gscale=np.array(gscale))
    keys = [k for k in HEAD_KEYS + BACKBONE_KEYS if k in rg and rg[k].grad is not None]
    assert sum(k.startswith('backbone.') for k in keys) >= 12 and len(keys) >= 26, keys
    worst, worst_key = 0.0, None
    for k in keys:
        arrs['grad:' + k] = sample(rg[k].grad)
        arrs['grad64:' + k] = sample(rg64[k].grad)
        d = (rg64[k].grad - rg[k].grad.double()).abs().max().item() / gscale
        if d > worst:
            worst, worst_key = d, k
    arrs['unused'] = np.array(sorted(k for k, p in rg.items() if p.grad is None))
    arrs['zero_grad'] = np.array(sorted(k for k, p in rg.items() if p.grad is not None and p.grad.abs().max() == 0))
    dist = dict(logits=(y.double() - y64).abs().max().item() / y.abs().max().item(), loss=abs(loss.item() - loss64.item()), grads=worst)
    arrs.update(ref32_vs_64_logit_err=np.array(dist['logits']), ref32_vs_64_loss_err=np.array(dist['loss']), ref32_vs_64_grad_err=np.array(dist['grads']))
    print('    %s at %d x %d: loss %.6f, gscale %.3e, min |logit| %.2e; fp32 reference vs fp64: logits %.2e of their scale, loss %.2e, gradients %.2e of gscale (%s)'
          % (bb, H, W, loss.item(), gscale, y.abs().min().item(), dist['logits'], dist['loss'], dist['grads'], worst_key))
    return arrs, {k: dist[k] / BARS[k] for k in BARS}


def case_train(bb):
    for H, W in SIZES:
        arrs, frac = run_train(bb, H, W)
        if max(frac.values()) <= 0.25:
            break
        print('    %s: reference-vs-referee reaches %s of the bars (more than a quarter): enlarging the input' % (bb, {k: '%.2f' % v for k, v in frac.items()}))
    else:
        raise SystemExit('%s: the fp32 reference stays further than a quarter of a bar from its fp64 referee at every size' % bb)
    mg.save('seg2d_%s_train' % bb, **arrs)


CASES = {'keys': case_keys, 'resnet34': lambda: case_train('resnet34'), 'resnet101': lambda: case_train('resnet101')}

if __name__ == '__main__':
    for name in (sys.argv[1:] or list(CASES)):
        print(name)
        CASES[name]()
