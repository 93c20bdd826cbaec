"""EfficientNet-B* feature extractor with the reference's customisations (stem_stride, endpoints).

Host-side mirror of /root/reference/code/efficientnet/{model,utils}.py for the segtran path: same module /
parameter names (so lukemelas-format and reference checkpoints load), same static-'same'-padding quirk N6
(padding derived from the NOMINAL image size, the stem bookkept as stride 2 even when stem_stride=1:
model.py:169-178, utils.py:248-275), same endpoint rule (endpoints are the INPUTS of blocks
`endpoint_blk_indices`, model.py:184,211-212,275-277).

Kernel status: every 1x1 convolution (127 of the 160 convs of B4) runs on libsegx's MFMA GEMM; the 32 depthwise
k3/k5 convolutions, BatchNorm+swish (fused), the squeeze-excite pooling/gating planes and the drop_connect+skip add
run on libsegx's HBM-bound kernels (backbone.hip); the dense 3x3 stem is an implicit GEMM on the MFMA engine
(conv3d.hip with depth 1); the squeeze-excite excitation MLP has its own wave-per-dot-product kernels.  No ATen
arithmetic is left in this file: the drop_connect draw and the skip add happen inside the last BatchNorm pass of a block.
"""
import math
import torch
from torch import nn
from torch.nn import functional as F

from .. import functional as SF
from ..fold import FoldableBackbone, fold_conv_bn, pair_sources

BN_MOM, BN_EPS = 1 - 0.99, 1e-3

# (num_repeat, kernel, stride, expand, in, out, se_ratio)  -- EfficientNet-B0 base table (utils.py:514-522)
_BASE = [(1, 3, 1, 1, 32, 16, 0.25), (2, 3, 2, 6, 16, 24, 0.25), (2, 5, 2, 6, 24, 40, 0.25), (3, 3, 2, 6, 40, 80, 0.25),
         (3, 5, 1, 6, 80, 112, 0.25), (4, 5, 2, 6, 112, 192, 0.25), (1, 3, 1, 6, 192, 320, 0.25)]
# name -> (width, depth, nominal resolution, dropout)   (utils.py:476-488)
_PARAMS = {'efficientnet-b0': (1.0, 1.0, 224, 0.2), 'efficientnet-b1': (1.0, 1.1, 240, 0.2),
           'efficientnet-b2': (1.1, 1.2, 260, 0.3), 'efficientnet-b3': (1.2, 1.4, 300, 0.3),
           'efficientnet-b4': (1.4, 1.8, 380, 0.4), 'efficientnet-b5': (1.6, 2.2, 456, 0.4),
           'efficientnet-b6': (1.8, 2.6, 528, 0.5), 'efficientnet-b7': (2.0, 3.1, 600, 0.5)}


def round_filters(filters, width, divisor=8):
    filters *= width
    new = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new < 0.9 * filters:
        new += divisor
    return int(new)


def round_repeats(repeats, depth):
    return int(math.ceil(depth * repeats))


class Conv2dStaticSamePadding(nn.Conv2d):
    """TF-'SAME' conv whose padding is fixed at construction from a given image size (N6)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, image_size=None, **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride, **kwargs)
        ih = iw = image_size
        kh, kw = self.weight.shape[-2:]
        sh, sw = self.stride
        oh, ow = math.ceil(ih / sh), math.ceil(iw / sw)
        ph = max((oh - 1) * sh + (kh - 1) * self.dilation[0] + 1 - ih, 0)
        pw = max((ow - 1) * sw + (kw - 1) * self.dilation[1] + 1 - iw, 0)
        self.static_pad = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
        self.pointwise = (kh == 1 and kw == 1 and sh == 1 and sw == 1 and self.groups == 1)

    def forward(self, x, pass_input=False):
        if self.pointwise:
            return SF.conv1x1(x, self.weight, self.bias, pass_input=pass_input)       # libsegx MFMA GEMM
        if self.groups == self.in_channels and self.groups == self.out_channels and self.bias is None:
            return SF.dwconv2d(x, self.weight, self.stride[0], self.static_pad)   # libsegx depthwise stencil
        assert self.groups == 1 and self.bias is None and self.dilation == (1, 1)
        return SF.conv2d_dense(x, self.weight, self.stride[0], self.static_pad)   # the 3x3 stem: libsegx implicit GEMM


def swish(x):
    return x * torch.sigmoid(x)


def drop_connect(x, p, training):
    """utils.py:129-154 -- per-sample stochastic depth."""
    if not training:
        return x
    keep = 1 - p
    r = keep + torch.rand([x.shape[0], 1, 1, 1], dtype=x.dtype, device=x.device)
    return x / keep * torch.floor(r)


class MBConvBlock(nn.Module):
    def __init__(self, k, s, e, cin, cout, se_ratio, image_size):
        super().__init__()
        self.stride, self.expand_ratio, self.input_filters, self.output_filters = s, e, cin, cout
        oup = cin * e
        if e != 1:
            self._expand_conv = Conv2dStaticSamePadding(cin, oup, 1, image_size=image_size, bias=False)
            self._bn0 = nn.BatchNorm2d(oup, momentum=BN_MOM, eps=BN_EPS)
        self._depthwise_conv = Conv2dStaticSamePadding(oup, oup, k, stride=s, image_size=image_size, groups=oup, bias=False)
        self._bn1 = nn.BatchNorm2d(oup, momentum=BN_MOM, eps=BN_EPS)
        nsq = max(1, int(cin * se_ratio))
        self._se_reduce = Conv2dStaticSamePadding(oup, nsq, 1, image_size=1)
        self._se_expand = Conv2dStaticSamePadding(nsq, oup, 1, image_size=1)
        self._project_conv = Conv2dStaticSamePadding(oup, cout, 1, image_size=math.ceil(image_size / s), bias=False)
        self._bn2 = nn.BatchNorm2d(cout, momentum=BN_MOM, eps=BN_EPS)

    gate_in_weights = True     # False: the reference's op order (gate applied to the activation, model.py:110), as a separate pass
    fused_middle = True        # _bn0 + swish, the depthwise convolution and _bn1 + swish + pooling as ONE channel-resident launch per direction where the library serves the
                               # shape (stride-1 blocks with planes of 1024 / 4096 floats, batch <= 6: SF.mbconv_mid); False: the three ops everywhere (tools/ab_switch.py)

    fused_entry = True         # _bn0 + swish and a stride-2 depthwise convolution as ONE team launch per direction where the library serves the shape (SF.bn_act_dwconv_s2);
                               # False: the two ops (tools/ab_switch.py)
    fused_entry_s1 = True      # the same for the stride-1 blocks the channel-resident middle does not take (SF.bn_act_dwconv_s1); a switch of its own

    def _takes_fused_entry(self, x):
        """training, one process, an expansion, a stride-2 or a 'same' stride-1 depthwise convolution, a served shape (x: the block's input -- the expansion keeps its height
        and width).  Asked after _takes_fused_middle: the channel-resident middle keeps the planes it serves."""
        dw = self._depthwise_conv
        if not (self.training and SF._bn_stats_sync is None and self.expand_ratio != 1 and dw.stride in ((1, 1), (2, 2))):
            return False
        if not (MBConvBlock.fused_entry if dw.stride == (2, 2) else MBConvBlock.fused_entry_s1):
            return False
        if not (self._bn0.training and dw.kernel_size[0] == dw.kernel_size[1] and x.dim() == 4 and x.dtype == torch.float32):
            return False
        ok = SF.bn_dw_s2_ok if dw.stride == (2, 2) else SF.bn_dw_s1_ok
        return ok((x.shape[0], dw.in_channels, x.shape[2], x.shape[3]), dw.kernel_size[0], dw.stride[0], dw.static_pad)

    def _takes_fused_middle(self, x):
        """training, one process (synchronised BatchNorm exchanges statistics between statistics and apply), an expansion, stride 1 with symmetric padding, a served shape"""
        if not (MBConvBlock.fused_middle and MBConvBlock.gate_in_weights and self.training and SF._bn_stats_sync is None and self.expand_ratio != 1):
            return False
        dw = self._depthwise_conv
        k = dw.kernel_size[0]
        if not (self._bn0.training and self._bn1.training and dw.stride == (1, 1) and dw.kernel_size == (k, k) and tuple(dw.static_pad) == (k // 2,) * 4):
            return False
        return x.dim() == 4 and x.dtype == torch.float32 and SF.mbconv_mid_ok((x.shape[0], dw.in_channels, x.shape[2], x.shape[3]), k)

    def folded_operands(self):
        """(w0, b0) | None, (w1, b1), (w2, b2): expansion / depthwise / projection convolution with _bn0 / _bn1 / _bn2 folded in (EfficientNet.fold_batchnorm)"""
        f0 = fold_conv_bn(self._expand_conv.weight, self._bn0) if self.expand_ratio != 1 else None
        return f0, fold_conv_bn(self._depthwise_conv.weight, self._bn1), fold_conv_bn(self._project_conv.weight, self._bn2)

    def forward_folded(self, inputs, folded):
        """forward() in eval mode on folded operands: no BatchNorm launch.  swish(_bn0(.)) is the expansion GEMM's epilogue; the depthwise kernel adds b1, applies swish
        and leaves the squeeze-excite pooling partials; the _bn2 scale sits in the projection weights BEFORE the gate forms the per-sample weights, its shift and the skip
        input are the bias / resid operands of the per-sample GEMM."""
        f0, (w1, b1), (w2, b2) = folded
        x = inputs
        skip = self.stride == 1 and self.input_filters == self.output_filters
        if f0 is not None:
            x = SF.conv1x1(x, f0[0], f0[1], act=SF.ACT_SWISH)
        dw = self._depthwise_conv
        y, psum, nch = SF.dwconv2d_bias_act_pool(x, w1, b1, dw.stride[0], dw.static_pad, SF.ACT_SWISH)
        Wb = SF.se_gate_weights(y, psum, nch, self._se_reduce.weight, self._se_reduce.bias, self._se_expand.weight, self._se_expand.bias, w2)
        return SF.conv1x1_per_sample_bias(y, Wb, b2, resid=inputs if skip else None)

    def forward(self, inputs, drop_connect_rate=None, entry_bn=None):
        """efficientnet/model.py:82-126.  entry_bn: the BatchNorm (+ swish) the caller left to this block's depthwise convolution (EfficientNet._stem_into_block0: the
        stem's, `inputs` is then the stem convolution's raw output; only for a block without expansion and skip)"""
        x = skip_in = inputs
        skip = self.stride == 1 and self.input_filters == self.output_filters
        fused = entry_bn is None and self._takes_fused_middle(x)
        entry = entry_bn is not None or (not fused and self._takes_fused_entry(x))
        dw = self._depthwise_conv
        if entry_bn is not None:
            assert self.expand_ratio == 1 and not skip
            d = SF.bn_act_dwconv_s1(x, entry_bn, dw.weight, dw.stride[0], dw.static_pad)
        elif entry:
            d = (SF.bn_act_dwconv_s2 if dw.stride == (2, 2) else SF.bn_act_dwconv_s1)(self._expand_conv(x), self._bn0, dw.weight, dw.stride[0], dw.static_pad)
        elif self.expand_ratio != 1 and not fused:
            # (`inputs` has two consumers when there is a skip connection.  Routing the second through the GEMM op's input alias -- its gradient added
            # inside the expansion's dX GEMM, SF.conv1x1(pass_input=True), what the Inception modules do -- was measured here, r04_d: the residual keeps
            # those dX GEMMs off the wave-specialised tiles, +0.40 ms/step of GEMM time against 0.24 ms of accumulation adds saved.  Not used.)
            x = SF.bn_act(self._expand_conv(x), self._bn0, SF.ACT_SWISH)
        se = (self._se_reduce.weight, self._se_reduce.bias, self._se_expand.weight, self._se_expand.bias)
        # drop_connect (utils.py:129-154, per-sample stochastic depth) and the skip add ride on the last BatchNorm pass: the sample's keep scale is
        # drawn inside the kernels from the library's Philox stream (H3: the reference's torch.rand stream cannot be matched anyway)
        rate = float(drop_connect_rate) if (skip and drop_connect_rate and self.training) else 0.0
        if fused:
            y, Wb = SF.mbconv_mid(self._expand_conv(x), self._bn0, self._depthwise_conv.weight, self._bn1, *se, self._project_conv.weight)
            x = SF.conv1x1_per_sample(y, Wb)
        elif MBConvBlock.gate_in_weights:
            # squeeze-excite gate folded into the projection weights (per-sample weights; the gated tensor is never written)
            y, Wb = SF.bn_act_gate_weights(d if entry else self._depthwise_conv(x), self._bn1, SF.ACT_SWISH, *se, self._project_conv.weight)
            x = SF.conv1x1_per_sample(y, Wb)
        else:
            x = self._project_conv(SF.bn_act_se(d if entry else self._depthwise_conv(x), self._bn1, SF.ACT_SWISH, *se))
        return SF.bn_act(x, self._bn2, SF.ACT_NONE, resid=skip_in if skip else None, drop_connect=rate)


class EfficientNet(FoldableBackbone, nn.Module):
    def __init__(self, model_name='efficientnet-b4', stem_stride=2, drop_connect_rate=0.2, num_classes=1000):
        super().__init__()
        width, depth, res, _ = _PARAMS[model_name]
        self.drop_connect_rate = drop_connect_rate
        self.stem_stride = stem_stride
        c0 = round_filters(32, width)
        self._conv_stem = Conv2dStaticSamePadding(3, c0, 3, stride=stem_stride, image_size=res, bias=False)
        self._bn0 = nn.BatchNorm2d(c0, momentum=BN_MOM, eps=BN_EPS)
        size = math.ceil(res / 2)                               # N6: bookkeeping assumes a stride-2 stem
        self._blocks = nn.ModuleList([])
        self.endpoint_seg_indices = [0, 1, 2, 4]
        self.endpoint_blk_indices = []
        for i, (r, k, s, e, cin, cout, se) in enumerate(_BASE):
            cin, cout, r = round_filters(cin, width), round_filters(cout, width), round_repeats(r, depth)
            self._blocks.append(MBConvBlock(k, s, e, cin, cout, se, size))
            size = math.ceil(size / s)
            for _ in range(r - 1):
                self._blocks.append(MBConvBlock(k, 1, e, cout, cout, se, size))
            if i in self.endpoint_seg_indices:
                self.endpoint_blk_indices.append(len(self._blocks))
        chead = round_filters(1280, width)
        self._conv_head = Conv2dStaticSamePadding(cout, chead, 1, image_size=size, bias=False)
        self._bn1 = nn.BatchNorm2d(chead, momentum=BN_MOM, eps=BN_EPS)
        self._fc = nn.Linear(chead, num_classes)               # kept for checkpoint compatibility; never used (N3)

    # ---- inference with BatchNorm folded into the convolutions (opt-in; the lifecycle is fold.FoldableBackbone's) ---------------------------
    def _fold_build(self):
        """_folded = (stem, [per block], head, sources, versions): the stem, the three pairs of each MBConv block, the head"""
        pairs = [(self._conv_stem, self._bn0), (self._conv_head, self._bn1)] + \
                [(c, b) for blk in self._blocks for c, b in ((getattr(blk, '_expand_conv', None), getattr(blk, '_bn0', None)), (blk._depthwise_conv, blk._bn1),
                                                            (blk._project_conv, blk._bn2)) if c is not None]
        return (fold_conv_bn(self._conv_stem.weight, self._bn0), [blk.folded_operands() for blk in self._blocks],
                fold_conv_bn(self._conv_head.weight, self._bn1)), pair_sources(pairs)

    def _extract_endpoints_folded(self, inputs):
        (ws, bs), blocks, (wh, bh) = self._folded[:3]
        endpoints = {}
        with torch.no_grad():
            x = SF.conv2d_stem_bias_act(inputs, ws, bs, self._conv_stem.stride[0], self._conv_stem.static_pad, SF.ACT_SWISH)
            prev_x = x
            for idx, block in enumerate(self._blocks):
                x = block.forward_folded(x, blocks[idx])
                if idx in self.endpoint_blk_indices:
                    endpoints['reduction_%d' % (len(endpoints) + 1)] = prev_x
                prev_x = x
            endpoints['reduction_%d' % (len(endpoints) + 1)] = SF.conv1x1(x, wh, bh, act=SF.ACT_SWISH)
        return endpoints

    @classmethod
    def from_name(cls, model_name, stem_stride=2, **kw):
        return cls(model_name, stem_stride=stem_stride, **kw)

    @classmethod
    def from_pretrained(cls, model_name, weights_path=None, advprop=False, ignore_missing_keys=False, stem_stride=2, **kw):
        """reference efficientnet/model.py:357-398: build the model, then load the published lukemelas checkpoint.  There is no
        network here, so the file must already be on disk: `weights_path`, or `<$SEGX_PRETRAINED_DIR>/<published file name>`
        (efficientnet/utils.py:570-596: e.g. adv-efficientnet-b4-44fb3a87.pth for advprop b4)."""
        model = cls.from_name(model_name, stem_stride=stem_stride, **kw)
        load_pretrained_weights(model, model_name, weights_path=weights_path, load_fc=True, advprop=advprop,
                                ignore_missing_keys=ignore_missing_keys)
        return model

    fused_stem_entry = True    # the stem's _bn0 + swish inside block 0's depthwise convolution (SF.bn_act_dwconv_s1) where _stem_into_block0 says so; False: SF.bn_act

    def _stem_into_block0(self, inputs):
        """does block 0 take the stem convolution's raw output and the stem's _bn0?  Training, one process, not folded; block 0 without expansion and skip (the stem's
        activation then has no other consumer) and with a 'same' stride-1 depthwise convolution; a stem output the library serves."""
        blk = self._blocks[0]
        dw, st = blk._depthwise_conv, self._conv_stem
        if not (EfficientNet.fused_stem_entry and self.training and self._bn0.training and blk.training and SF._bn_stats_sync is None and not self.batchnorm_folded):
            return False
        if blk.expand_ratio != 1 or dw.stride != (1, 1) or dw.kernel_size[0] != dw.kernel_size[1] or (blk.stride == 1 and blk.input_filters == blk.output_filters):
            return False
        if inputs.dim() != 4 or inputs.dtype != torch.float32 or 0 in self.endpoint_blk_indices:
            return False
        pl, pr, pt, pb = st.static_pad
        H = (inputs.shape[2] + pt + pb - st.kernel_size[0]) // st.stride[0] + 1
        W = (inputs.shape[3] + pl + pr - st.kernel_size[1]) // st.stride[1] + 1
        return SF.bn_dw_s1_ok((inputs.shape[0], dw.in_channels, H, W), dw.kernel_size[0], 1, dw.static_pad)

    def extract_endpoints(self, inputs):
        if self.batchnorm_folded:
            return self._extract_endpoints_folded(inputs)
        endpoints = {}
        stem_bn = self._bn0 if self._stem_into_block0(inputs) else None          # block 0 then applies the stem's BatchNorm + swish inside its depthwise convolution
        x = self._conv_stem(inputs) if stem_bn is not None else SF.bn_act(self._conv_stem(inputs), self._bn0, SF.ACT_SWISH)
        prev_x = x                                                                # (never an endpoint: the first endpoint index is >= 1)
        nblk = len(self._blocks)
        for idx, block in enumerate(self._blocks):
            rate = self.drop_connect_rate * float(idx) / nblk if self.drop_connect_rate else None
            x = block(x, drop_connect_rate=rate, entry_bn=stem_bn) if idx == 0 and stem_bn is not None else block(x, drop_connect_rate=rate)
            if idx in self.endpoint_blk_indices:
                endpoints['reduction_%d' % (len(endpoints) + 1)] = prev_x
            prev_x = x
        x = SF.bn_act(self._conv_head(x), self._bn1, SF.ACT_SWISH)
        endpoints['reduction_%d' % (len(endpoints) + 1)] = x
        return endpoints


# published checkpoint file names (reference efficientnet/utils.py:570-596)
PRETRAINED_FILES = {False: {'efficientnet-b0': 'efficientnet-b0-355c32eb.pth', 'efficientnet-b1': 'efficientnet-b1-f1951068.pth',
                            'efficientnet-b2': 'efficientnet-b2-8bb594d6.pth', 'efficientnet-b3': 'efficientnet-b3-5fb5a3c3.pth',
                            'efficientnet-b4': 'efficientnet-b4-6ed6700e.pth', 'efficientnet-b5': 'efficientnet-b5-b6417697.pth',
                            'efficientnet-b6': 'efficientnet-b6-c76e70fd.pth', 'efficientnet-b7': 'efficientnet-b7-dcc49843.pth'},
                    True: {'efficientnet-b0': 'adv-efficientnet-b0-b64d5a18.pth', 'efficientnet-b1': 'adv-efficientnet-b1-0f3ce85a.pth',
                           'efficientnet-b2': 'adv-efficientnet-b2-6e9d97e5.pth', 'efficientnet-b3': 'adv-efficientnet-b3-cdd7c0f4.pth',
                           'efficientnet-b4': 'adv-efficientnet-b4-44fb3a87.pth', 'efficientnet-b5': 'adv-efficientnet-b5-86493f6b.pth',
                           'efficientnet-b6': 'adv-efficientnet-b6-ac80338e.pth', 'efficientnet-b7': 'adv-efficientnet-b7-4652b6dd.pth',
                           'efficientnet-b8': 'adv-efficientnet-b8-22a8fe65.pth'}}


def pretrained_path(model_name, advprop=False):
    import os
    d = os.environ.get('SEGX_PRETRAINED_DIR')
    if not d:
        raise RuntimeError('pretrained %s weights: no network access here -- download %s and pass weights_path=..., or put it '
                           'under $SEGX_PRETRAINED_DIR (or build with use_pretrained=False)' % (model_name, PRETRAINED_FILES[advprop][model_name]))
    path = os.path.join(d, PRETRAINED_FILES[advprop][model_name])
    if not os.path.exists(path):
        raise RuntimeError('pretrained weights not found: ' + path)
    return path


def load_pretrained_weights(model, model_name, weights_path=None, load_fc=True, advprop=False, ignore_missing_keys=False):
    """reference efficientnet/utils.py:601-636 with a local file instead of model_zoo.load_url; same key checks."""
    state_dict = torch.load(weights_path if isinstance(weights_path, str) else pretrained_path(model_name, advprop), map_location='cpu')
    if not load_fc:
        state_dict.pop('_fc.weight'); state_dict.pop('_fc.bias')
    ret = model.load_state_dict(state_dict, strict=False)
    if not ignore_missing_keys:
        expect = set() if load_fc else {'_fc.weight', '_fc.bias'}
        assert set(ret.missing_keys) == expect, 'Missing keys when loading pretrained weights: %s' % ret.missing_keys
    assert not ret.unexpected_keys, 'Unexpected keys when loading pretrained weights: %s' % ret.unexpected_keys
