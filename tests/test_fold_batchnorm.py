"""BatchNorm folded into the 2-D backbone's kernels for inference (Segtran2d.fold_batchnorm): the swish GEMM epilogue, the fused depthwise kernel, a folded MBConv
block against an fp64 referee, the fold's lifecycle, and the absence of any BatchNorm launch.  Runs on the fiber emulator here and on the HIP build under -m gpu."""
import copy
import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd import segx
from segtran_amd.efficientnet.model import EfficientNet, MBConvBlock, Conv2dStaticSamePadding, BN_MOM, BN_EPS
from test_kernels_backbone import rnd, close

REFEREE = 2.25          # the project's fp64-referee factor (tests/test_gpu_fullshape.py)


def _swish(u):
    return u * torch.sigmoid(u)


@pytest.fixture(params=['x6', 'f32'])
def engine_name(request, backend):
    L = segx.lib()
    prev = L.set_engine(request.param)
    yield request.param
    L.set_engine(prev)


# (Cin, Cout): the expansion convolutions of EfficientNet-B4, at small spatial sizes; then ragged ones -- S no multiple of 4 (scalar loaders), Cout no multiple
# of any tile, and a float4-legal shape with partial edge tiles in both directions
@pytest.mark.parametrize('Cin,Cout,B,H,W', [(24, 144, 2, 8, 8), (32, 192, 2, 8, 8), (56, 336, 1, 8, 8), (112, 672, 1, 8, 8), (160, 960, 1, 8, 8), (272, 1632, 1, 8, 8),
                                            (24, 150, 2, 7, 9), (40, 200, 2, 10, 10), (56, 336, 1, 12, 16)])
def test_swish_epilogue_gemm(engine_name, Cin, Cout, B, H, W):
    x = rnd(B, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, 1, 1, seed=2, scale=Cin ** -0.5)
    b = rnd(Cout, seed=3, scale=0.5)
    L = segx.lib()
    L.x6_launches()
    y = SF.conv1x1(x, w, b, act=SF.ACT_SWISH)
    on_x6 = L.x6_launches() > 0
    assert on_x6 == (engine_name == 'x6' and (H * W) % 4 == 0 and Cin % 4 == 0 and H * W > 48)      # the engine under test really ran it
    close(y, _swish(F.conv2d(x, w, b)))
    close(SF.conv1x1(x, w, None, act=SF.ACT_SWISH), _swish(F.conv2d(x, w)))


def test_swish_epilogue_is_forward_only_and_refuses_other_uses(backend):
    x, w = rnd(1, 8, 4, 4, seed=1), rnd(16, 8, 1, 1, seed=2).requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.conv1x1(x, w, None, act=SF.ACT_SWISH)
    with torch.no_grad():
        assert not SF.conv1x1(x, w, None, act=SF.ACT_SWISH).requires_grad
    with pytest.raises(NotImplementedError):
        SF.conv1x1(x, w.detach(), None, act=SF.ACT_RELU)
    # the library itself: the swish epilogue takes no residual operand and no other operand layout
    L, wd = segx.lib(), w.detach().reshape(16, 8).contiguous()
    y = torch.empty(1, 16, 4, 4)
    with pytest.raises(RuntimeError, match='swish'):
        L.gemm(wd, x, y, 16, 16, 8, (0, 0, 8, 1), (128, 0, 1, 16), (256, 0, 16), epilogue=segx.EPI_SWISH, resid=torch.zeros_like(y))
    with pytest.raises(RuntimeError, match='swish'):
        L.gemm(wd, x, y, 16, 16, 8, (0, 0, 8, 1), (0, 0, 8, 1), (0, 0, 16), epilogue=segx.EPI_SWISH)


# the (k, stride, pad, H, W) list of test_kernels_backbone.py::test_dwconv2d
@pytest.mark.parametrize('k,stride,pad,H,W', [(3, 1, (1, 1, 1, 1), 20, 18), (5, 1, (2, 2, 2, 2), 17, 33), (3, 2, (0, 1, 0, 1), 32, 32),
                                              (5, 2, (2, 2, 2, 2), 16, 16), (5, 2, (1, 2, 1, 2), 24, 40), (3, 2, (0, 1, 0, 1), 7, 9),
                                              (3, 1, (0, 2, 2, 0), 12, 40),
                                              (3, 1, (1, 1, 1, 1), 37, 300),
                                              (5, 2, (1, 2, 1, 2), 150, 140),
                                              (5, 1, (2, 2, 2, 2), 130, 64),
                                              (3, 2, (1, 1, 1, 1), 16, 24),
                                              (3, 1, (1, 1, 1, 1), 100, 128),
                                              (5, 2, (2, 2, 2, 2), 96, 256),
                                              (5, 2, (1, 2, 1, 2), 22, 40), (3, 2, (0, 1, 0, 1), 18, 600),
                                              (5, 1, (2, 2, 2, 2), 64, 64), (3, 1, (1, 1, 1, 1), 32, 128), (5, 1, (2, 2, 2, 2), 24, 256), (3, 1, (1, 1, 1, 1), 20, 256)])
def test_dwconv_bias_swish_pool_fused(backend, k, stride, pad, H, W):
    B, C = (2, 5) if H * W < 4000 else (2, 2)
    x = rnd(B, C, H, W, seed=7)
    w = rnd(C, 1, k, k, seed=8)
    b = rnd(C, seed=9, scale=0.5)
    y, psum, nch = SF.dwconv2d_bias_act_pool(x, w, b, stride, pad, SF.ACT_SWISH)
    yr = _swish(F.conv2d(F.pad(x, pad), w, b, stride, 0, 1, C))
    assert y.shape == yr.shape and nch == backend.L.dwconv2d_pool_chunks(*yr.shape[2:]) and psum.numel() == B * C * nch
    close(y, yr)
    S = yr.shape[2] * yr.shape[3]
    close(psum.view(B, C, nch).sum(2) / S, yr.mean((2, 3)))
    # without the activation, and without pooling
    y0, p0, n0 = SF.dwconv2d_bias_act_pool(x, w, b, stride, pad, SF.ACT_NONE, pool=False)
    assert p0 is None and n0 == 0
    close(y0, F.conv2d(F.pad(x, pad), w, b, stride, 0, 1, C))


def _randomize_bn(mod, seed):
    """non-trivial BatchNorm state: mean != 0, var != 1, random gamma and beta"""
    i = 0
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.weight.copy_(1 + 0.3 * rnd(C, seed=seed + i)); m.bias.copy_(0.3 * rnd(C, seed=seed + i + 1))
                m.running_mean.copy_(0.4 * rnd(C, seed=seed + i + 2)); m.running_var.copy_(0.5 + rnd(C, seed=seed + i + 3).abs())
                i += 4


def _init_block(blk, seed):
    with torch.no_grad():
        for j, (n, p) in enumerate(blk.named_parameters()):
            if p.dim() == 4:
                fan = p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(rnd(*p.shape, seed=seed + j, scale=fan ** -0.5))
            elif 'bn' not in n:
                p.copy_(0.2 * rnd(*p.shape, seed=seed + j))
    _randomize_bn(blk, seed + 100)


def _block_fp64(blk, x):
    """the MBConv block in eval mode (efficientnet/model.py:82-126), plain PyTorch in fp64"""
    d = lambda t: t.detach().double()

    def bn(u, m):
        v = lambda t: d(t).view(1, -1, 1, 1)
        return (u - v(m.running_mean)) / torch.sqrt(v(m.running_var) + m.eps) * v(m.weight) + v(m.bias)
    u = x0 = d(x)
    if blk.expand_ratio != 1:
        u = _swish(bn(F.conv2d(u, d(blk._expand_conv.weight)), blk._bn0))
    dw = blk._depthwise_conv
    u = _swish(bn(F.conv2d(F.pad(u, dw.static_pad), d(dw.weight), None, dw.stride, 0, 1, u.shape[1]), blk._bn1))
    p = u.mean((2, 3), keepdim=True)
    g = torch.sigmoid(F.conv2d(_swish(F.conv2d(p, d(blk._se_reduce.weight), d(blk._se_reduce.bias))), d(blk._se_expand.weight), d(blk._se_expand.bias)))
    u = bn(F.conv2d(u * g, d(blk._project_conv.weight)), blk._bn2)
    if blk.stride == 1 and blk.input_filters == blk.output_filters:
        u = u + x0
    return u


# one block of each kind: e = 1; stride 2 with k = 5; skip with k = 3 (the last also at a plane size that is no float4 multiple)
@pytest.mark.parametrize('k,s,e,cin,cout,size', [(3, 1, 1, 32, 16, 16), (5, 2, 6, 24, 40, 16), (3, 1, 6, 24, 24, 16), (3, 1, 6, 24, 24, 18)],
                         ids=['e1', 'stride2-k5', 'skip-k3', 'skip-k3-18'])
def test_folded_mbconv_block_vs_fp64_referee(backend, k, s, e, cin, cout, size):
    blk = MBConvBlock(k, s, e, cin, cout, 0.25, size)
    _init_block(blk, 11)
    blk.eval()
    x = rnd(2, cin, size, size, seed=5)
    ref = _block_fp64(blk, x)
    with torch.no_grad():
        y_unfolded = blk(x)
        y_folded = blk.forward_folded(x, blk.folded_operands())
    assert y_folded.shape == ref.shape and not y_folded.requires_grad
    scale = ref.abs().max().item()
    d_unf = (y_unfolded.double() - ref).abs().max().item()
    d_fold = (y_folded.double() - ref).abs().max().item()
    print('mbconv k%d s%d e%d %d: |folded - fp64| = %.3e, |unfolded - fp64| = %.3e, scale %.3e' % (k, s, e, size, d_fold, d_unf, scale))
    assert d_fold <= max(3e-5 * scale, REFEREE * d_unf), (d_fold, d_unf, scale)


def _short_backbone(seed=3):
    """EfficientNet-B0 cut to its first four blocks (e = 1; stride 2; skip; stride 2 with k = 5) and a 64-channel head: every kind of conv -> BatchNorm pair, small enough
    for the emulator"""
    torch.manual_seed(seed)
    net = EfficientNet.from_name('efficientnet-b0', stem_stride=2)
    net._blocks = torch.nn.ModuleList(list(net._blocks)[:4])
    net.endpoint_blk_indices = [1, 3]
    net._conv_head = Conv2dStaticSamePadding(net._blocks[-1].output_filters, 64, 1, image_size=28, bias=False)
    net._bn1 = torch.nn.BatchNorm2d(64, momentum=BN_MOM, eps=BN_EPS)
    net._fc = torch.nn.Linear(64, 4)
    for j, blk in enumerate(net._blocks):
        _init_block(blk, 20 + 7 * j)
    with torch.no_grad():
        net._conv_stem.weight.copy_(rnd(*net._conv_stem.weight.shape, seed=1, scale=27 ** -0.5))
        net._conv_head.weight.copy_(rnd(*net._conv_head.weight.shape, seed=2, scale=40 ** -0.5))
    _randomize_bn(net, 500)
    return net


def test_folded_backbone_issues_no_batchnorm_launch(backend, monkeypatch):
    net = _short_backbone().eval()
    x = rnd(2, 3, 32, 32, seed=4)
    with torch.no_grad():
        want = net.extract_endpoints(x)
    net.fold_batchnorm()
    assert net.batchnorm_folded

    def boom(*a, **k):
        raise AssertionError('segx_bn_act_fwd2 launched')
    monkeypatch.setattr(type(segx.lib()), 'bn_act_fwd2', boom)
    got = net.extract_endpoints(x)                            # no BatchNorm launch, no autograd graph (grad mode is on here)
    assert sorted(got) == sorted(want)
    for name in want:
        assert not got[name].requires_grad
        close(got[name], want[name], 1e-4)
    net.unfold_batchnorm()
    with pytest.raises(AssertionError, match='bn_act_fwd2 launched'), torch.no_grad():
        net.extract_endpoints(x)


def test_fold_is_dropped_by_train_and_the_model_is_the_unfolded_one_bit_for_bit(backend):
    """after train(), a train step (here: the backbone's forward, a loss on its endpoints, backward) gives loss and gradients bit-identical to a never-folded twin"""
    net = _short_backbone()
    twin = copy.deepcopy(net)
    net.eval().fold_batchnorm()
    assert net.batchnorm_folded
    net.train()
    assert not net.batchnorm_folded
    twin.train()
    x = rnd(2, 3, 32, 32, seed=4)
    out = []
    for m in (net, twin):
        SF.manual_seed(5)
        ep = m.extract_endpoints(x)
        loss = sum((v * v).mean() for v in ep.values())
        loss.backward()
        out.append(loss.detach())
    assert torch.equal(out[0], out[1])
    n = 0
    for (na, pa), (nb, pb) in zip(net.named_parameters(), twin.named_parameters()):
        assert na == nb and (pa.grad is None) == (pb.grad is None)
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), na
            n += 1
    assert n > 40
    for (na, ba), (nb, bb) in zip(net.named_buffers(), twin.named_buffers()):
        assert torch.equal(ba, bb), na                         # running statistics moved identically


def test_fold_lifecycle_of_the_model():
    """host side only (no kernel runs): state_dict untouched, train mode refused, train() / load_state_dict() / an in-place parameter change drop the fold"""
    import segtran_amd
    from segtran_amd import engine
    net = engine.build_model(dict(engine.CONFIGS['cfg1'], size=(64, 64)), 'cpu', attractors=32)
    _randomize_bn(net.backbone, 9)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(RuntimeError, match='eval'):
        net.fold_batchnorm()
    assert not net.batchnorm_folded
    net.eval()
    assert segtran_amd.fold_batchnorm(net) is net and net.batchnorm_folded
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) and after[k].shape == before[k].shape for k in before)
    assert not any('fold' in n for n, _ in list(net.named_parameters()) + list(net.named_buffers()))
    # the fold algebra, against fp64 on the host: w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps)
    bb = net.backbone
    (ws, bs), blocks, (wh, bh) = bb._folded[:3]
    assert len(blocks) == len(bb._blocks) and all((f[0] is None) == (blk.expand_ratio == 1) for f, blk in zip(blocks, bb._blocks))
    for (w, b), conv, bn in [((ws, bs), bb._conv_stem, bb._bn0), ((wh, bh), bb._conv_head, bb._bn1), (blocks[5][0], bb._blocks[5]._expand_conv, bb._blocks[5]._bn0),
                             (blocks[5][1], bb._blocks[5]._depthwise_conv, bb._blocks[5]._bn1), (blocks[5][2], bb._blocks[5]._project_conv, bb._blocks[5]._bn2)]:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        assert w.dtype == torch.float32 and not w.requires_grad and not isinstance(w, torch.nn.Parameter)
        assert torch.equal(w, (conv.weight.detach().double() * s.view(-1, 1, 1, 1)).float())
        assert torch.equal(b, (bn.bias.detach().double() - bn.running_mean.double() * s).float())
    net.train()
    assert not net.batchnorm_folded
    net.eval().fold_batchnorm()
    net.load_state_dict(before)
    assert not net.batchnorm_folded
    net.fold_batchnorm()
    with torch.no_grad():
        bb._bn0.running_var.mul_(2.0)                          # a source tensor changed in place: the folded operands are stale
    assert not net.batchnorm_folded
    net.fold_batchnorm().unfold_batchnorm()
    assert not net.batchnorm_folded


def test_segtran3d_refuses_to_fold():
    from segtran_amd import engine
    net = engine.build_model(dict(engine.CONFIGS['cfg4'], size=(112, 112, 16)), 'cpu', synth=False, attractors=64)
    net.eval()
    with pytest.raises(NotImplementedError):
        net.fold_batchnorm()
    assert not net.batchnorm_folded
