"""Inception-v1 I3D feature extractor -- host-side mirror of /root/reference/code/networks/aj_i3d/aj_i3d.py.

Same module / parameter names (`Conv3d_1a_7x7.conv3d.weight`, `Mixed_4b.b1b.bn.running_mean`, ...), the
dynamic TF-'same' zero padding of N7 (front = pad // 2; aj_i3d.py:8-30, 68-90) and `do_pool1=False`
(`MaxPool3d_2a_3x3` = Identity, :206-210).

Kernel status: everything runs on libsegx -- the 38 1x1x1 convolutions on the MFMA GEMM, the 7x7x7 stem and the 19
3x3x3 convolutions as implicit GEMM on the same MFMA engine (conv3d.hip: forward, backward-data, backward-weight),
BatchNorm3d+ReLU as one fused kernel (backbone.hip), the 'same' max-pools in conv3d.hip; the backward-data of the stride-2 stem
(a transposed convolution onto 3 channels) is the residue-class gather kernel of conv3d.hip -- and is not needed at all when Segtran3d
composes its input bridge into the stem filters (the default).  No ATen / MIOpen / rocBLAS arithmetic anywhere.

Inference (opt-in): InceptionI3d.fold_batchnorm() folds every BatchNorm3d into the convolution in front of it; the layers then run as ONE launch each -- the GEMM's
ReLU epilogue, bias + ReLU inside the halo / implicit-GEMM kernels -- and an Inception module assembles its output without BatchNorm launches or torch.cat.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import functional as SF
from ...fold import FoldableBackbone, fold_conv_bn, pair_sources


class MaxPool3dSamePadding(nn.MaxPool3d):
    def forward(self, x, pass_input=False):
        return SF.maxpool3d_same(x, self.kernel_size, self.stride, pass_input)  # libsegx: zero 'same' padding + max-pool (pass_input: -> (y, alias of x))


class Unit3D(nn.Module):
    def __init__(self, in_channels, output_channels, kernel_shape=(1, 1, 1), stride=(1, 1, 1), activation_fn=F.relu,
                 use_batch_norm=True, use_bias=False, name='unit_3d'):
        super().__init__()
        self._kernel_shape, self._stride = tuple(kernel_shape), tuple(stride)
        self._activation_fn, self._use_batch_norm = activation_fn, use_batch_norm
        self.name = name
        self.conv3d = nn.Conv3d(in_channels, output_channels, self._kernel_shape, self._stride, padding=0, bias=use_bias)
        if use_batch_norm:
            self.bn = nn.BatchNorm3d(output_channels, eps=0.001, momentum=0.01)
        self.pointwise = self._kernel_shape == (1, 1, 1) and self._stride == (1, 1, 1)

    def forward(self, x, conv_out=None):
        """conv_out: the convolution's output computed by the caller (Segtran3d composes its input bridge into the stem's filters)."""
        if conv_out is not None:
            x = conv_out
        elif self.pointwise:
            x = SF.conv1x1(x, self.conv3d.weight, self.conv3d.bias)            # libsegx MFMA GEMM
        else:
            assert self.conv3d.bias is None
            x = SF.conv3d_same(x, self.conv3d.weight, self._stride)              # libsegx implicit-GEMM MFMA convolution
        if self._use_batch_norm:                                               # fused BatchNorm3d (+ReLU), libsegx
            return SF.bn_act(x, self.bn, SF.ACT_RELU if self._activation_fn is F.relu else SF.ACT_NONE)
        if self._activation_fn is not None:
            x = self._activation_fn(x)
        return x

    @property
    def foldable(self):
        """a bias-free convolution -> BatchNorm -> ReLU layer: every Unit3D of the feature extractor (not the classification head)"""
        return self._use_batch_norm and self._activation_fn is F.relu and self.conv3d.bias is None

    def forward_folded(self, x, f, out=None):
        """f = [w', b', ops] from InceptionI3d.fold_batchnorm: relu(conv(x, w') + b') in ONE launch -- the GEMM's ReLU epilogue for a pointwise layer, else the halo /
        implicit-GEMM kernel with bias + ReLU (SF.conv3d_bias_relu; ops: its derived filter banks, built at the first call).  No BatchNorm launch, no autograd graph."""
        if self.pointwise:
            return SF.conv1x1_relu(x, f[0], f[1], out=out)
        return SF.conv3d_bias_relu(x, f[0], f[1], self._stride, out=out, ops=f[2])


class InceptionModule(nn.Module):
    def __init__(self, in_channels, out_channels, name):
        super().__init__()
        o = out_channels
        self.b0 = Unit3D(in_channels, o[0], name=name + '/Branch_0/Conv3d_0a_1x1')
        self.b1a = Unit3D(in_channels, o[1], name=name + '/Branch_1/Conv3d_0a_1x1')
        self.b1b = Unit3D(o[1], o[2], (3, 3, 3), name=name + '/Branch_1/Conv3d_0b_3x3')
        self.b2a = Unit3D(in_channels, o[3], name=name + '/Branch_2/Conv3d_0a_1x1')
        self.b2b = Unit3D(o[3], o[4], (3, 3, 3), name=name + '/Branch_2/Conv3d_0b_3x3')
        self.b3a = MaxPool3dSamePadding(kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=0)
        self.b3b = Unit3D(in_channels, o[5], name=name + '/Branch_3/Conv3d_0b_1x1')
        self.name = name

    fuse_reductions = True     # False: the reference's op order (four independent branches)
    cat_in_place = True        # False: torch.cat assembles the module's output (tests: the two forms agree bit for bit)

    def forward(self, x):
        if InceptionModule.fuse_reductions:
            # The two 1x1x1 reductions b1a | b2a (16 .. 192 filters each: skinny GEMMs on their own) as ONE pointwise convolution with the
            # concatenated filters and ONE BatchNorm + ReLU over the concatenated channels (per-channel: exactly the two layers; one synchronised
            # exchange instead of two), the 3x3x3 convolutions reading their channel slices of that tensor in place (SF.conv3d_slices): x is read
            # once instead of twice, its gradient arrives as one tensor instead of two.
            # r03: branch 0's own 1x1x1 convolution joins them (its filters LAST, so the slices of the 3x3x3 convolutions still start at channel 0):
            # the three pointwise convolutions of the module's input are ONE GEMM, their three BatchNorm layers one statistics / apply pass and one
            # synchronised exchange; branch 0's output is the tail slice of that tensor.
            # r04: no accumulation kernels of autograd's around the module -- (a) x has two consumers (this convolution, the pooling branch): the second
            # goes through the alias the GEMM op returns, its gradient is added inside the dX GEMM; (b) branch 0's slice of t leaves through
            # conv3d_slices (its gradient is written into t's gradient there); (c) the concatenation's gradient is read IN PLACE by the BatchNorm
            # backward kernels of the four branches (channel slices with a batch stride: no contiguous copies).
            w120 = torch.cat([self.b1a.conv3d.weight, self.b2a.conv3d.weight, self.b0.conv3d.weight], dim=0)
            t, x2 = SF.conv1x1(x, w120, pass_input=True)
            t = SF.bn_act_multi(t, [self.b1a.bn, self.b2a.bn, self.b0.bn], SF.ACT_RELU)
            y1, y2, y0 = SF.conv3d_slices(t, self.b1b.conv3d.weight, self.b2b.conv3d.weight, with_tail=True)
            if InceptionModule.cat_in_place:
                # r05: the three BatchNorm + ReLU passes that end branches 1..3 write their channels straight into the concatenation (SF.bn_act_cat): torch.cat
                # copied every branch once more (four strided copy kernels per module, 0.6-0.8 ms of a cfg4 / cfg5 step); only branch 0's slice is still copied
                y3 = SF.conv1x1(self.b3a(x2), self.b3b.conv3d.weight, self.b3b.conv3d.bias)
                return SF.bn_act_cat(y0, [(y1, self.b1b.bn), (y2, self.b2b.bn), (y3, self.b3b.bn)], SF.ACT_RELU)
            return torch.cat([y0, SF.bn_act(y1, self.b1b.bn, SF.ACT_RELU), SF.bn_act(y2, self.b2b.bn, SF.ACT_RELU), self.b3b(self.b3a(x2))], dim=1)
        return torch.cat([self.b0(x), self.b1b(self.b1a(x)), self.b2b(self.b2a(x)), self.b3b(self.b3a(x))], dim=1)

    def folded_operands(self):
        """[[w', b', ops] of b0, b1a, b1b, b2a, b2b, b3b]: what forward_folded takes (InceptionI3d.fold_batchnorm derives the same per module)"""
        return [list(fold_conv_bn(u.conv3d.weight, u.bn)) + [{}] for u in (self.b0, self.b1a, self.b1b, self.b2a, self.b2b, self.b3b)]

    def forward_folded(self, x, layers):
        """The module with its six BatchNorm layers folded in (layers: [w', b', ops] of b0, b1a, b1b, b2a, b2b, b3b; folded_operands()): ONE ReLU GEMM writes t = the
        [b1a | b2a | b0] reductions; the two 3 x 3 x 3 convolutions read their slices of t and write their slices of the output (bias + ReLU in their kernels); the
        pooling branch's ReLU GEMM writes its slice; branch 0's tail of t is copied into its slice (the one copy of the unfolded form).  Channel order [b0, b1, b2, b3].
        No BatchNorm launch, no torch.cat; the concatenated reduction filters are kept in b1a's operand cache."""
        f0, f1a, f1b, f2a, f2b, f3b = layers
        ops = f1a[2]
        if 'reduce' not in ops:
            ops['reduce'] = (torch.cat([f1a[0], f2a[0], f0[0]], dim=0).contiguous(), torch.cat([f1a[1], f2a[1], f0[1]]).contiguous())
        w120, b120 = ops['reduce']
        t = SF.conv1x1_relu(x, w120, b120)
        r1, r2 = f1a[0].shape[0], f2a[0].shape[0]
        c0, c1, c2, c3 = f0[0].shape[0], f1b[0].shape[0], f2b[0].shape[0], f3b[0].shape[0]
        out = torch.empty((x.shape[0], c0 + c1 + c2 + c3) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        SF.conv3d_bias_relu(t[:, :r1], f1b[0], f1b[1], out=out[:, c0:c0 + c1], ops=f1b[2])
        SF.conv3d_bias_relu(t[:, r1:r1 + r2], f2b[0], f2b[1], out=out[:, c0 + c1:c0 + c1 + c2], ops=f2b[2])
        dst, pooled = out[:, c0 + c1 + c2:], self.b3a(x)
        if SF._chan_slice_bs(dst) is not None:
            SF.conv1x1_relu(pooled, f3b[0], f3b[1], out=dst)
        else:                                                   # (a slice that does not start on 16 bytes: no I3D stage -- its channel counts come in eights)
            dst.copy_(SF.conv1x1_relu(pooled, f3b[0], f3b[1]))
        out[:, :c0].copy_(t[:, r1 + r2:])
        return out


class InceptionI3d(FoldableBackbone, nn.Module):
    VALID_ENDPOINTS = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2b_1x1', 'Conv3d_2c_3x3', 'MaxPool3d_3a_3x3',
                       'Mixed_3b', 'Mixed_3c', 'MaxPool3d_4a_3x3', 'Mixed_4b', 'Mixed_4c', 'Mixed_4d', 'Mixed_4e',
                       'Mixed_4f', 'MaxPool3d_5a_2x2', 'Mixed_5b', 'Mixed_5c', 'Logits', 'Predictions')

    def __init__(self, num_classes=400, in_channels=3, do_pool1=True, name='inception_i3d'):
        super().__init__()
        ep = {}
        ep['Conv3d_1a_7x7'] = Unit3D(in_channels, 64, (7, 7, 7), (2, 2, 2), name=name + 'Conv3d_1a_7x7')
        ep['MaxPool3d_2a_3x3'] = MaxPool3dSamePadding((1, 3, 3), (1, 2, 2), padding=0) if do_pool1 else nn.Identity()
        ep['Conv3d_2b_1x1'] = Unit3D(64, 64, name=name + 'Conv3d_2b_1x1')
        ep['Conv3d_2c_3x3'] = Unit3D(64, 192, (3, 3, 3), name=name + 'Conv3d_2c_3x3')
        ep['MaxPool3d_3a_3x3'] = MaxPool3dSamePadding((1, 3, 3), (1, 2, 2), padding=0)
        ep['Mixed_3b'] = InceptionModule(192, [64, 96, 128, 16, 32, 32], name + 'Mixed_3b')
        ep['Mixed_3c'] = InceptionModule(256, [128, 128, 192, 32, 96, 64], name + 'Mixed_3c')
        ep['MaxPool3d_4a_3x3'] = MaxPool3dSamePadding((3, 3, 3), (2, 2, 2), padding=0)
        ep['Mixed_4b'] = InceptionModule(480, [192, 96, 208, 16, 48, 64], name + 'Mixed_4b')
        ep['Mixed_4c'] = InceptionModule(512, [160, 112, 224, 24, 64, 64], name + 'Mixed_4c')
        ep['Mixed_4d'] = InceptionModule(512, [128, 128, 256, 24, 64, 64], name + 'Mixed_4d')
        ep['Mixed_4e'] = InceptionModule(512, [112, 144, 288, 32, 64, 64], name + 'Mixed_4e')
        ep['Mixed_4f'] = InceptionModule(528, [256, 160, 320, 32, 128, 128], name + 'Mixed_4f')
        ep['MaxPool3d_5a_2x2'] = MaxPool3dSamePadding((2, 2, 2), (2, 2, 2), padding=0)
        ep['Mixed_5b'] = InceptionModule(832, [256, 160, 320, 32, 128, 128], name + 'Mixed_5b')
        ep['Mixed_5c'] = InceptionModule(832, [384, 192, 384, 48, 128, 128], name + 'Mixed_5c')
        self.end_points = ep
        # classification head: parameters kept for checkpoint compatibility (never used on the segtran path);
        # registered before the endpoints, as in the reference (aj_i3d.py:279-286), so parameter order matches.
        self.logits = Unit3D(1024, num_classes, activation_fn=None, use_batch_norm=False, use_bias=True, name='logits')
        for k, m in ep.items():
            self.add_module(k, m)

    def extract_features(self, x, stem_conv_out=None, stem_out=None):
        """stem_conv_out: output of the (bias-free) stem convolution computed by the caller; `x` is then not read.
        stem_out (folded only): the stem layer's output after BatchNorm and ReLU, from folded_stem_bridge."""
        if self.batchnorm_folded:
            assert stem_conv_out is None, 'the folded extractor takes the stem output from folded_stem_bridge (Segtran3d), not a raw convolution output'
            return self._extract_features_folded(x, stem_out)
        feat, prev = {}, None
        for name in self.VALID_ENDPOINTS:
            if name in self.end_points:
                m = self._modules[name]
                if name == 'Conv3d_1a_7x7' and stem_conv_out is not None:
                    x = m(None, conv_out=stem_conv_out)
                elif isinstance(m, MaxPool3dSamePadding) and prev in self.pyramid_endpoints and tuple(m.stride) != (1, 1, 1):
                    # the pooled tensor is also an endpoint the feature pyramid reads (segtran3d.py:436-441): the pyramid gets an alias, so that its gradient
                    # reaches the pool's backward kernel and is added there (SF._MaxPool3d) -- no accumulation kernel over two full-size tensors
                    x, feat[prev] = m(x, pass_input=True)
                else:
                    x = m(x)
                feat[name] = x
                prev = name
        return feat

    pyramid_endpoints = ('Conv3d_2c_3x3', 'Mixed_3c', 'Mixed_4f')      # feats[1..3] of Segtran3d (each is followed by a strided pool)

    # ---- inference with BatchNorm3d folded into the convolutions (opt-in; the lifecycle is fold.FoldableBackbone's) -----------
    def _foldable_units(self):
        """[(module path, Unit3D)]: 'Conv3d_1a_7x7', 'Mixed_3b.b1a', ..."""
        return [(name + ('.' + sub if sub else ''), m) for name in self.end_points for sub, m in self._modules[name].named_modules() if isinstance(m, Unit3D) and m.foldable]

    def _fold_build(self):
        """Derive (w', b') = (w gamma / sqrt(var + eps), beta - mean gamma / sqrt(var + eps)) of every convolution -> BatchNorm3d -> ReLU layer of the feature extractor
        (fp64 on the parameters' device, rounded once).  Eval mode only.  extract_features then issues no BatchNorm launch, no torch.cat and -- after the first call,
        which fills the per-layer operand cache (concatenated reduction filters, halo / packed filter banks, the stem's constants) -- no pack launch.  train(),
        load_state_dict(), a device / dtype move and an in-place change of a source tensor (torch's version counters) drop the fold and its cache.
        _folded = (layers, sources, versions): layers = {module path of a Unit3D: [w', b', ops]}"""
        units = self._foldable_units()
        return ({path: list(fold_conv_bn(u.conv3d.weight, u.bn)) + [{}] for path, u in units},), pair_sources([(u.conv3d, u.bn) for _, u in units])

    def folded_operands(self, path):
        """[w', b', ops] of one Unit3D of the folded extractor by its module path ('Conv3d_1a_7x7', 'Mixed_3b.b1b'; ops: the layer's operand cache)"""
        return self._folded[0][path]

    def folded_stem_bridge(self, batch, bridge_weight, bridge_bias, space_to_depth):
        """relu(bn(Conv3d_1a_7x7(in_bridge_to3(batch)))) of the folded model with the 4 -> 3 input bridge composed into the stem (Segtran3d.fuse_input_bridge).
        space_to_depth: the stride-(2, 2, 1) form -- the folded filters carry the BatchNorm factor, the bridge's bias map carries it too and the BatchNorm's folded
        bias on top; one convolution and ONE pass y = relu(y + map).  Else the 8-channel stride-2 form with a per-channel bias in the convolution's epilogue.  The
        composed constants live in the stem's operand cache (the bias map per input extent) and are rebuilt when the bridge's tensors change."""
        stem = self.Conv3d_1a_7x7
        w, b, ops = self.folded_operands('Conv3d_1a_7x7')
        key = (id(bridge_weight), bridge_weight._version, id(bridge_bias), bridge_bias._version)
        if ops.get('bridge_key') != key:
            ops.clear()
            ops['bridge_key'] = key
        with torch.no_grad():
            if space_to_depth:
                if 's2d' not in ops:
                    ops['s2d'] = SF.stem_s2d_folded_operands(w, bridge_weight.detach(), bridge_bias.detach(), b) + ({}, {})
                w2, v, bias, conv_ops, maps = ops['s2d']
                B, Cb, H, W, D = batch.shape
                if (D, H, W) not in maps:
                    maps[(D, H, W)] = SF.stem_s2d_bias_map(v, bias, D, H, W)
                return SF.stem_bridge_conv_s2d_folded(batch, w2, maps[(D, H, W)], ops=conv_ops)
            if 'composed' not in ops:
                ops['composed'] = (SF.stem_compose(w, bridge_weight.detach(), bridge_bias.detach(), 8), {})
            wc, conv_ops = ops['composed']
            return SF.conv3d_bias_relu(SF.bridge_input(batch, 8), wc, b, stem._stride, ops=conv_ops)

    def _extract_features_folded(self, x, stem_out=None):
        """stem_out: the stem layer's OUTPUT (after BatchNorm and ReLU) computed by the caller (folded_stem_bridge); `x` is then not read"""
        feat, L = {}, self._folded[0]
        with torch.no_grad():
            for name in self.VALID_ENDPOINTS:
                if name not in self.end_points:
                    continue
                m = self._modules[name]
                if name == 'Conv3d_1a_7x7' and stem_out is not None:
                    x = stem_out
                elif isinstance(m, Unit3D):
                    x = m.forward_folded(x, L[name])
                elif isinstance(m, InceptionModule):
                    x = m.forward_folded(x, [L[name + '.' + b] for b in ('b0', 'b1a', 'b1b', 'b2a', 'b2b', 'b3b')])
                else:
                    x = m(x)                                    # the pools (Identity without do_pool1); the pyramid reads feat[prev] as it is
                feat[name] = x
        return feat
