"""CPU: the host-side pieces every backbone and both evaluations share (no kernels run) -- the lifecycle of the BatchNorm fold (fold.FoldableBackbone), the chunk
runner of the fused sliding-window sequence (infer_common.run_chunks) and the fold-for-a-block context manager (infer_common.folded)."""
import pytest
import torch
from torch import nn

from segtran_amd import resnet
from segtran_amd.efficientnet.model import EfficientNet
from segtran_amd.fold import FoldableBackbone, fold_conv_bn
from segtran_amd.infer_common import folded, run_chunks
from segtran_amd.networks.aj_i3d.aj_i3d import InceptionI3d


class Toy(FoldableBackbone, nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 3, 1, bias=False)
        self.bn = nn.BatchNorm2d(3)

    def sources(self):
        return [self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]

    def _fold_build(self):
        return (fold_conv_bn(self.conv.weight, self.bn),), self.sources()


class Parent(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = Toy()


def test_fold_lifecycle_drop_table():
    torch.manual_seed(0)
    toy = Toy()
    with pytest.raises(RuntimeError, match=r'fold_batchnorm\(\) is for inference: call \.eval\(\) first \(in training mode BatchNorm uses batch statistics and cannot be folded\)'):
        toy.fold_batchnorm()
    assert toy._folded is None and not toy.batchnorm_folded
    toy.eval()
    unfolded_keys = list(toy.state_dict())
    assert toy.fold_batchnorm() is toy and toy.batchnorm_folded
    assert list(toy.state_dict()) == unfolded_keys                      # the derived tensors are neither Parameters nor buffers
    (w, b), src, versions = toy._folded
    assert len(src) == len(versions) == 5 and all(s is t for s, t in zip(src, toy.sources()))
    s = toy.bn.weight.double() / torch.sqrt(toy.bn.running_var.double() + toy.bn.eps)
    assert torch.equal(w, (toy.conv.weight.double() * s.view(-1, 1, 1, 1)).float()) and torch.equal(b, (toy.bn.bias.double() - toy.bn.running_mean.double() * s).float())

    # what does not drop the fold
    toy.eval()
    assert toy.batchnorm_folded
    toy.train(False)
    assert toy.batchnorm_folded

    # what drops it
    toy.train()
    assert toy._folded is None and not toy.eval().batchnorm_folded

    toy.fold_batchnorm().to(torch.float64)                              # _apply
    assert toy._folded is None and not toy.batchnorm_folded
    toy.float()

    parent = Parent().eval()
    state = {k: v.clone() for k, v in parent.state_dict().items()}
    parent.backbone.fold_batchnorm()
    parent.load_state_dict(state)                                       # of a module that contains it
    assert parent.backbone._folded is None

    for i in range(5):                                                  # an in-place edit of each source tensor, one at a time
        assert toy.fold_batchnorm().batchnorm_folded
        with torch.no_grad():
            toy.sources()[i].mul_(1.5)
        assert not toy.batchnorm_folded and toy._folded is None, i

    toy.fold_batchnorm().unfold_batchnorm()
    assert toy._folded is None and not toy.batchnorm_folded


BACKBONES = {'efficientnet': lambda: EfficientNet('efficientnet-b0'), 'resnet': lambda: resnet.resnet34(do_pool1=False),
             'i3d': lambda: InceptionI3d(num_classes=2, do_pool1=False)}


@pytest.mark.parametrize('name', sorted(BACKBONES))
def test_real_backbones_take_the_lifecycle_from_the_mixin(name):
    bb = BACKBONES[name]()                                              # parameters only: no forward, no kernel
    assert isinstance(bb, FoldableBackbone)
    for m in ('fold_batchnorm', 'unfold_batchnorm', 'batchnorm_folded', 'train', '_apply', '_load_from_state_dict'):
        assert m not in vars(type(bb)), m                               # one copy: the mixin's
    keys = list(bb.state_dict())
    assert bb.eval().fold_batchnorm() is bb and bb.batchnorm_folded
    src, versions = bb._folded[-2:]
    assert isinstance(src, list) and len(src) == len(versions) > 0 and len(src) % 5 == 0
    assert all(isinstance(t, torch.Tensor) for t in src) and versions == [t._version for t in src]
    assert list(bb.state_dict()) == keys
    bb.train()
    assert bb._folded is None and not bb.batchnorm_folded


class StubNet:
    def __init__(self):
        self.shapes, self.last = [], None

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        self.last = x[:, :1] * 2
        return self.last


def test_run_chunks_one_chunk_returns_the_forward_itself():
    net, patches = StubNet(), torch.randn(6, 3, 4)
    out = run_chunks(net, patches, [(0, 6)])
    assert out is net.last and net.shapes == [(6, 3, 4)] and torch.equal(out, patches[:, :1] * 2)


@pytest.mark.parametrize('rows, chunks', [
    (8, [(0, 4), (4, 8)]),                                              # equal chunks
    (7, [(0, 3), (3, 6), (6, 7)]),                                      # a short last chunk
    (15, [(0, 2), (2, 4), (4, 5), (5, 7), (7, 9), (9, 10), (10, 12), (12, 14), (14, 15)]),     # 3-D: rows of 5 windows in batches of 2, restarting per x row
    (12, [(k * 2, min(k + 4, 6) * 2) for k in range(0, 6, 4)]),        # 2-D: 6 windows of 2 images, 4 windows per call
])
def test_run_chunks_stacks_the_chunks_side_by_side(rows, chunks):
    torch.manual_seed(rows)
    net, patches = StubNet(), torch.randn(rows, 3, 4)
    out = run_chunks(net, patches, chunks)
    assert out.shape == (rows, 1, 4) and torch.equal(out, patches[:, :1] * 2)
    assert net.shapes == [(r1 - r0, 3, 4) for r0, r1 in chunks]


class FakeNet:
    def __init__(self, is_folded=False):
        self.batchnorm_folded, self.folds, self.unfolds = is_folded, 0, 0

    def fold(self, net):
        assert net is self
        self.folds += 1
        self.batchnorm_folded = True

    def unfold(self, net):
        assert net is self
        self.unfolds += 1
        self.batchnorm_folded = False


def test_folded_context_manager():
    net = FakeNet()
    with folded(net, True, net.fold, net.unfold):
        assert net.batchnorm_folded and (net.folds, net.unfolds) == (1, 0)
    assert not net.batchnorm_folded and (net.folds, net.unfolds) == (1, 1)

    pre = FakeNet(is_folded=True)                                       # a net the caller folded stays as it is
    with folded(pre, True, pre.fold, pre.unfold):
        assert pre.batchnorm_folded
    assert pre.batchnorm_folded and (pre.folds, pre.unfolds) == (0, 0)

    net = FakeNet()
    with pytest.raises(KeyError):
        with folded(net, True, net.fold, net.unfold):
            raise KeyError('inside the block')
    assert not net.batchnorm_folded and (net.folds, net.unfolds) == (1, 1)

    for start in (False, True):
        net = FakeNet(is_folded=start)
        with folded(net, False, net.fold, net.unfold):
            assert net.batchnorm_folded == start
        assert net.batchnorm_folded == start and (net.folds, net.unfolds) == (0, 0)
