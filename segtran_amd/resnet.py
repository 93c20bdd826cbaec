"""ResNet-34/50/101 feature extractor: host-side mirror of the reference's code/resnet.py as far as Segtran2d uses it (segtran2d.py:89-92, :341-342).

Same module and parameter names (conv1, bn1, layer1..4.<i>.{conv1,bn1,conv2,bn2[,conv3,bn3],downsample.0,downsample.1}, fc), so torchvision-format and reference
checkpoints load; same initialisation (resnet.py:149-155); `ext_features(x) -> (x0_pool, x1, x2, x3, x4)`.  `fc` is kept for checkpoints and never used.  The
`lens` / `xlayer` / `lenskit` machinery of the reference's file, resnet18 / resnet152 (no bb2feat_dims rows) and resibn101 (no constructor in the reference) are not
built and refuse loudly.

Kernel status -- the forward runs entirely on libsegx, no ATen arithmetic:
  conv1 (7 x 7, stride 2), the 3 x 3 convolutions and the stride-2 1 x 1 down-sample convolutions   SF.conv2d_dense: the implicit-GEMM engine on a depth-1 volume
                                                                                                    (all three gradients; the 3-channel stem has no input gradient to form)
  stride-1 1 x 1 convolutions                                                                       SF.conv1x1 (MFMA GEMM)
  bn -> relu                                                                                        SF.bn_act(x, bn, ACT_RELU)
  block end relu(bn(x) + shortcut)                                                                  SF.add_relu(SF.bn_act(x, bn_last, ACT_NONE, resid=shortcut)): the skip add rides
                                                                                                    on the BatchNorm apply pass, the ReLU behind it is one streaming pass (resnet.hip)
  maxpool (only with do_pool1, i.e. --nofeatup)                                                     the 3-D max-pool kernels on a depth-1 volume, see ResNet._maxpool
With BatchNorm folded (fold_batchnorm(), eval mode only) no BatchNorm launch remains: conv -> bn -> relu pairs run as SF.conv3d_bias_relu / SF.conv1x1_relu, a block's
last and down-sample convolutions run plain on the folded filters and SF.add_relu(z, shortcut, bias=b_last + b_down, out=z) closes the block in place.
"""
import math
import os
import torch
from torch import nn

from . import functional as SF
from .fold import FoldableBackbone, fold_conv_bn, pair_sources

__all__ = ['ResNet', 'BasicBlock', 'Bottleneck', 'resnet34', 'resnet50', 'resnet101']

# published checkpoint file names (the reference's model_urls table, resnet.py:13-19)
PRETRAINED_FILES = {'resnet34': 'resnet34-333f7ec4.pth', 'resnet50': 'resnet50-19c8e357.pth', 'resnet101': 'resnet101-5d3b4d8f.pth'}


class _Conv(nn.Conv2d):
    """nn.Conv2d(bias=False) parameter container whose forward runs on libsegx: k x k at any stride with symmetric padding."""

    def forward(self, x):
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        if k == 1 and s == 1:
            return SF.conv1x1(x, self.weight, None)
        return SF.conv2d_dense(x, self.weight, s, (p, p, p, p))

    # ---- BatchNorm folded (forward only, under torch.no_grad()): w, b = fold_conv_bn(self.weight, bn); ops = this layer's cache of derived filter banks ----
    def _vol(self):
        s, p = self.stride[0], self.padding[0]
        return (1, s, s), ((0, 0), (p, p), (p, p))

    def folded_relu(self, x, w, b, ops):
        """relu(conv(x, w) + b)"""
        if self.kernel_size[0] == 1 and self.stride[0] == 1:
            return SF.conv1x1_relu(x, w, b)
        stride, pads = self._vol()
        return SF.conv3d_bias_relu(x.unsqueeze(2), w.unsqueeze(2), b, stride=stride, pads=pads, ops=ops).squeeze(2)

    def folded_plain(self, x, w, ops):
        """conv(x, w): the bias is added by the block's closing pass"""
        if self.kernel_size[0] == 1 and self.stride[0] == 1:
            return SF.conv1x1(x, w, None)
        stride, pads = self._vol()
        return SF.conv3d_bias_relu(x.unsqueeze(2), w.unsqueeze(2), None, stride=stride, pads=pads, ops=ops).squeeze(2)


def conv3x3(in_planes, out_planes, stride=1):
    """3x3 convolution with padding"""
    return _Conv(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class _Block(nn.Module):
    """what BasicBlock and Bottleneck share: the (conv, bn) chain `_pairs()`, the shortcut and the closing add + ReLU"""

    def _pairs(self):
        raise NotImplementedError

    def _fold_pairs(self):
        """every (conv, bn) pair of the block, the down-sample pair last"""
        return self._pairs() + ([(self.downsample[0], self.downsample[1])] if self.downsample is not None else [])

    def forward(self, x):
        """resnet.py:42-69 / :89-120"""
        shortcut = x
        if self.downsample is not None:
            shortcut = SF.bn_act(self.downsample[0](x), self.downsample[1])
        pairs = self._pairs()
        out = x
        for conv, bn in pairs[:-1]:
            out = SF.bn_act(conv(out), bn, SF.ACT_RELU)
        conv, bn = pairs[-1]
        return SF.add_relu(SF.bn_act(conv(out), bn, SF.ACT_NONE, resid=shortcut))

    def folded_operands(self):
        """([(w, b, ops) per pair of _pairs()], (w_down, ops) | None, b_close): b_close = b_last + b_down, summed once here (b_down = 0 without a down-sample path)"""
        main = [fold_conv_bn(conv.weight, bn) + ({},) for conv, bn in self._pairs()]
        b_close, down = main[-1][1], None
        if self.downsample is not None:
            wd, bd = fold_conv_bn(self.downsample[0].weight, self.downsample[1])
            down, b_close = (wd, {}), (b_close + bd).contiguous()
        return main, down, b_close

    def forward_folded(self, x, folded):
        main, down, b_close = folded
        shortcut = x if down is None else self.downsample[0].folded_plain(x, down[0], down[1])
        pairs = self._pairs()
        out = x
        for (conv, _), (w, b, ops) in zip(pairs[:-1], main[:-1]):
            out = conv.folded_relu(out, w, b, ops)
        z = pairs[-1][0].folded_plain(out, main[-1][0], main[-1][2])
        return SF.add_relu(z, shortcut, bias=b_close, out=z)


class BasicBlock(_Block):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def _pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]


class Bottleneck(_Block):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _Conv(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _Conv(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = _Conv(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=False)
        self.downsample = downsample
        self.stride = stride

    def _pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]


class ResNet(FoldableBackbone, nn.Module):
    """set do_pool1=False when taking small images as input (resnet.py:122): Segtran2d passes do_pool1 = not bb_feat_upsize"""

    def __init__(self, block, layers, num_classes=1000, lens_stage=None, no_fc=False, no_avgpool=False, do_pool1=True):
        super().__init__()
        if lens_stage is not None:
            raise NotImplementedError("ResNet(lens_stage=%r): the reference's lens / xlayer / lenskit machinery is not built" % (lens_stage,))
        self.inplanes = 64
        self.conv1 = _Conv(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)          # kept for checkpoint compatibility; never used
        self.no_fc, self.no_avgpool, self.do_pool1 = no_fc, no_avgpool, do_pool1
        for m in self.modules():                                           # resnet.py:149-155
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(_Conv(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def _blocks_in_order(self):
        return [blk for layer in (self.layer1, self.layer2, self.layer3, self.layer4) for blk in layer]

    @staticmethod
    def _maxpool(x):
        """nn.MaxPool2d(3, 2, padding=1) on the 3-D max-pool kernels (depth-1 volume, pads ((0,0),(1,1),(1,1))).  Those kernels pad with ZEROS where torch pads with
        -inf.  Behind a ReLU the two agree: every value is >= 0 and every window holds at least one real element, so a padded zero never exceeds the real maximum.
        Where a window's real elements are all 0, a padded zero scanned first may win the tie and drop the window's gradient, where torch routes it to a real zero --
        and the backward of the ReLU in front annuls whatever reaches an element that is 0.  So outputs and the gradients in front of the ReLU are identical
        (tests/test_resnet_kernels.py, with an all-zero window)."""
        return SF._MaxPool3d.apply(x.unsqueeze(2), (1, 3, 3), (1, 2, 2), ((0, 0), (1, 1), (1, 1))).squeeze(2)

    def ext_features(self, x):
        """resnet.py:186-200"""
        if self.batchnorm_folded:
            return self._ext_features_folded(x)
        x0 = SF.bn_act(self.conv1(x), self.bn1, SF.ACT_RELU)
        feats = [self._maxpool(x0) if self.do_pool1 else x0]
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            cur = feats[-1]
            for blk in layer:
                cur = blk(cur)
            feats.append(cur)
        return tuple(feats)

    def forward(self, x):
        raise NotImplementedError('ResNet.forward (the ImageNet classifier head) is not built: Segtran2d calls ext_features()')

    # ---- inference with BatchNorm folded into the convolutions (the lifecycle is fold.FoldableBackbone's) ------------------------------------
    def _fold_build(self):
        """_folded = (stem, [per block], sources, versions)"""
        blocks = self._blocks_in_order()
        pairs = [(self.conv1, self.bn1)] + [pair for blk in blocks for pair in blk._fold_pairs()]
        return (fold_conv_bn(self.conv1.weight, self.bn1) + ({},), [blk.folded_operands() for blk in blocks]), pair_sources(pairs)

    def _ext_features_folded(self, x):
        (ws, bs, ops), blocks = self._folded[:2]
        with torch.no_grad():
            x0 = self.conv1.folded_relu(x, ws, bs, ops)
            feats = [self._maxpool(x0) if self.do_pool1 else x0]
            it = iter(blocks)
            for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
                cur = feats[-1]
                for blk in layer:
                    cur = blk.forward_folded(cur, next(it))
                feats.append(cur)
        return tuple(feats)


def pretrained_path(model_name):
    """There is no network here: the published torchvision checkpoint must already be on disk, as <$SEGX_PRETRAINED_DIR>/<file name of the reference's model_urls>."""
    d = os.environ.get('SEGX_PRETRAINED_DIR')
    if not d:
        raise RuntimeError('pretrained %s weights: no network access here -- download %s and put it under $SEGX_PRETRAINED_DIR '
                           '(or build with use_pretrained=False: --nopretrain, or --synthweights)' % (model_name, PRETRAINED_FILES[model_name]))
    path = os.path.join(d, PRETRAINED_FILES[model_name])
    if not os.path.exists(path):
        raise RuntimeError('pretrained weights not found: %s (or build with use_pretrained=False: --nopretrain, or --synthweights)' % path)
    return path


def _build(name, block, layers, pretrained, kwargs):
    model = ResNet(block, layers, **kwargs)
    if pretrained:                                                         # resnet.py:283 & co.: load_state_dict(model_zoo.load_url(...), strict=False), from a local file
        model.load_state_dict(torch.load(pretrained_path(name), map_location='cpu'), strict=False)
    return model


def resnet34(pretrained=False, **kwargs):
    return _build('resnet34', BasicBlock, [3, 4, 6, 3], pretrained, kwargs)


def resnet50(pretrained=False, **kwargs):
    return _build('resnet50', Bottleneck, [3, 4, 6, 3], pretrained, kwargs)


def resnet101(pretrained=False, **kwargs):
    return _build('resnet101', Bottleneck, [3, 4, 23, 3], pretrained, kwargs)


def _not_built(name, why):
    def refuse(*args, **kwargs):
        raise NotImplementedError('%s is not built: %s' % (name, why))
    refuse.__name__ = name
    return refuse


resnet18 = _not_built('resnet18', 'Segtran has no bb2feat_dims row for it (resnet34, resnet50 and resnet101 are built)')
resnet152 = _not_built('resnet152', 'Segtran has no bb2feat_dims row for it (resnet34, resnet50 and resnet101 are built)')
resibn101 = _not_built('resibn101', 'the reference has no constructor for it (resnet34, resnet50 and resnet101 are built)')

BACKBONES = {'resnet34': resnet34, 'resnet50': resnet50, 'resnet101': resnet101}
