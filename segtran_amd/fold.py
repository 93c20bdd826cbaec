"""BatchNorm folded into the convolution in front of it, for inference: the arithmetic (fold_conv_bn) and the ONE lifecycle of a folded backbone (FoldableBackbone),
shared by EfficientNet, ResNet and InceptionI3d.  A backbone lists its conv -> BatchNorm pairs in `_fold_build()`; when a fold is dropped is decided here."""
import torch


def fold_conv_bn(weight, bn):
    """BatchNorm in eval mode is the per-channel affine map y = x * s + (beta - mu * s), s = gamma / sqrt(var + eps): folded into the convolution that feeds it,
    w' = w * s[out channel], b' = beta - mu * s.  Derived in fp64 on the parameters' device and rounded once to fp32; plain tensors (no Parameter, no buffer)."""
    with torch.no_grad():
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = (weight.double() * s.view(-1, *([1] * (weight.dim() - 1)))).float().contiguous()
        b = (bn.bias.double() - bn.running_mean.double() * s).float().contiguous()
    return w, b


def pair_sources(pairs):
    """every tensor the folded operands of (conv, bn) pairs are derived from: convolution weight, BatchNorm parameters and running statistics"""
    return [t for conv, bn in pairs for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)]


class FoldableBackbone:
    """Mixin, placed before nn.Module in the bases: inference with BatchNorm folded into the convolutions (opt-in).  The backbone supplies `_fold_build()` ->
    (operands, sources): the tuple of derived operands in its own layout and the list of tensors they were derived from.  Registers nothing: the derived tensors are
    neither Parameters nor buffers and never in state_dict()."""

    _folded = None             # None, or operands + (sources, versions)

    def fold_batchnorm(self):
        """Derive the folded operands of every conv -> BatchNorm pair (`_fold_build()`).  Eval mode only.  The feature extractor then issues no BatchNorm launch.
        train(), load_state_dict(), a device / dtype move and an in-place change of a source tensor (torch's version counters) drop the fold again."""
        if self.training:
            raise RuntimeError('fold_batchnorm() is for inference: call .eval() first (in training mode BatchNorm uses batch statistics and cannot be folded)')
        operands, src = self._fold_build()
        self._folded = tuple(operands) + (src, [t._version for t in src])
        return self

    def unfold_batchnorm(self):
        self._folded = None

    @property
    def batchnorm_folded(self):
        """True while the feature extractor runs on folded operands; a source tensor changed in place since fold_batchnorm() drops the fold here"""
        f = self._folded
        if f is not None and (self.training or any(t._version != v for t, v in zip(f[-2], f[-1]))):
            self._folded = f = None
        return f is not None

    def train(self, mode=True):
        if mode:
            self._folded = None
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._folded = None                # .to() / .cuda() / .float(): the derived tensors would stay behind
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._folded = None                # reached from load_state_dict() of this module and of any module that contains it
        return super()._load_from_state_dict(*args, **kwargs)
