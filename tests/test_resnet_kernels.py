"""resnet.hip (the block-closing add + ReLU) bit for bit against its fp32 CPU expression, one ResNet block of each kind against a plain-torch restatement on ATen's
CPU kernels (train mode, eval mode, BatchNorm folded), and the max-pool form of the stem.  Runs on the fiber emulator here and on the HIP build under -m gpu."""
import copy

import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd import resnet
from test_kernels_backbone import close                     # the tolerances of BatchNorm + convolution compositions: 3e-5 outputs, 1e-4 gradients, 1e-5 statistics
from test_fold_batchnorm import _init_block, REFEREE

# One sweep of a full grid of resnet.hip: AR_FLAT_CAP (1024) workgroups x 256 threads x AR_UNROLL (4) float4 = 4,194,304 floats in the flat kernels, and AR_GRID_CAP
# (2048) runs of at most AR_RUN (512) float4 = 4,194,304 floats in the bias kernels.  (2056, 8, 2048) = 4,210,688 floats in 2056 one-plane runs is beyond both.
BEYOND_SPAN = (2056, 8, 2048)
SHAPES = [(1, 1, 1), (3, 3, 3), (5, 5, 4), (6, 3, 24), (7, 7, 25), (4, 2, 1024), (4, 4, 1028), (2, 2, 4099), (70000, 8, 4), BEYOND_SPAN]


def _eighths(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device='cpu').float() / 8


def _case(planes, C, S, seed=0):
    """z, r [planes, S], bias [C]: multiples of 1/8 (every sum is exact), about a quarter of the sums (z + b) + r exactly 0; -0.0, one +inf and one NaN each in z, r and
    bias where the tensor has room for them"""
    g = torch.Generator(device='cpu').manual_seed(1000 * seed + planes + 7 * S)
    z, r, b = _eighths(g, -16, 16, planes, S), _eighths(g, -16, 16, planes, S), _eighths(g, -8, 8, C)
    cancel = torch.rand(planes, S, generator=g, device='cpu') < 0.25
    r = torch.where(cancel, -(z + b.repeat(planes // C).view(-1, 1)), r)
    zf, rf = z.view(-1), r.view(-1)
    n = planes * S
    if n >= 6:
        zf[1], rf[1] = -0.0, 0.0
        zf[2] = float('inf')
        zf[3] = float('nan')
        rf[4] = float('nan')
    if C >= 2:
        b[C - 1] = float('nan')
    return z, r, b


def _expr(z, r, b, C):
    """the stated expression on the CPU: relu((z + bias[p % C]) + r), the additions in that order in fp32"""
    v = z
    if b is not None:
        v = v + b.repeat(z.shape[0] // C).view(-1, 1)
    if r is not None:
        v = v + r
    return torch.relu(v)


def _same(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what + ': NaN positions differ'
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), what + ': values differ'


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_add_relu_forward_and_backward_bit_for_bit(backend, shape):
    planes, C, S = shape
    B = planes // C
    z, r, b = _case(planes, C, S)
    dev = backend.dev
    zd, rd, bd = z.view(B, C, S).to(dev), r.view(B, C, S).to(dev), b.to(dev)
    nan_in = int(torch.isnan(z).sum() + torch.isnan(r).sum())
    for with_r in (False, True):
        for with_b in (False, True):
            want = _expr(z, r if with_r else None, b if with_b else None, C)
            if with_b or with_r:
                assert planes * S < 6 or torch.isnan(want).any()
            got = SF.add_relu(zd, rd if with_r else None, bias=bd if with_b else None)
            _same(got.view(planes, S), want, 'r=%s bias=%s' % (with_r, with_b))
    assert nan_in == (2 if planes * S >= 6 else 0)
    want = _expr(z, r, b, C)
    if planes * S >= 64:
        finite = ~torch.isnan(want)                                    # (a NaN bias takes its whole channel)
        zero = (want[finite] == 0).float().mean().item()
        assert 0.3 < zero < 0.8, zero                                  # negative sums and the exact cancellations
        assert (((z + b.repeat(B).view(-1, 1)) + r)[finite] == 0).float().mean().item() > 0.15
    # Y aliasing Z
    z2 = zd.clone()
    out = SF.add_relu(z2, rd, bias=bd, out=z2)
    assert out is z2
    _same(z2.view(planes, S), want, 'in place')
    # backward: dz = y > 0 ? dy : 0, from y alone; one tensor for z and r
    g = torch.Generator(device='cpu').manual_seed(5 + planes)
    dy = _eighths(g, -16, 16, planes, S)
    y = _expr(z, r, None, C)
    want_dz = torch.where(y > 0, dy, torch.zeros_like(dy))
    finite = ~torch.isnan(y)
    assert torch.equal(want_dz[finite], torch.ops.aten.threshold_backward(dy, y, 0)[finite])
    za, ra = zd.clone().requires_grad_(True), rd.clone().requires_grad_(True)
    ya = SF.add_relu(za, ra)
    _same(ya.view(planes, S), y, 'autograd forward')
    ya.backward(dy.view(B, C, S).to(dev))
    _same(za.grad.view(planes, S), want_dz, 'dz')
    _same(ra.grad.view(planes, S), want_dz, 'dr')
    assert (za.grad.view(planes, S).cpu()[y == 0] == 0).all()
    # the entry point itself, on misaligned planes of the same buffers (scalar paths)
    if S > 1 and planes * S <= 70000 * 4:
        L = backend.L
        zs, rs = zd.reshape(-1)[1:1 + (planes - C) * S], rd.reshape(-1)[1:1 + (planes - C) * S]
        if planes > C:
            p2 = planes - C
            ys = torch.empty(p2 * S + 1, device=dev)[1:]
            L.add_relu_fwd(zs, rs, bd, ys, p2, C, S)
            zc, rc = z.reshape(-1)[1:1 + p2 * S].view(p2, S), r.reshape(-1)[1:1 + p2 * S].view(p2, S)
            _same(ys.view(p2, S), _expr(zc, rc, b, C), 'misaligned')


def test_add_relu_refusals(backend):
    L, dev = backend.L, backend.dev
    z, y = torch.zeros(2, 3, 4, device=dev), torch.empty(2, 3, 4, device=dev)
    with pytest.raises(RuntimeError, match='segx_add_relu_fwd'):
        L.add_relu_fwd(None, None, None, y, 6, 3, 4)
    with pytest.raises(RuntimeError, match='segx_add_relu_fwd'):
        L.add_relu_fwd(z, None, None, y, 6, 3, 0)
    with pytest.raises(RuntimeError, match='segx_add_relu_fwd'):
        L.add_relu_fwd(z, None, torch.zeros(4, device=dev), y, 6, 4, 4)          # planes no multiple of C
    with pytest.raises(RuntimeError, match='segx_add_relu_bwd'):
        L.add_relu_bwd(None, y, z, 6, 4)
    with pytest.raises(RuntimeError, match='segx_add_relu_bwd'):
        L.add_relu_bwd(z, y, torch.empty_like(y), 6, -1)
    bias = torch.zeros(3, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match='bias gradient is not built'):
        SF.add_relu(z, None, bias=bias)
    with torch.no_grad():
        assert not SF.add_relu(z, None, bias=bias).requires_grad
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.add_relu(z.clone().requires_grad_(True), None, bias=bias.detach())
    with pytest.raises(ValueError, match='resid'):
        SF.add_relu(z, torch.zeros(2, 3, 5, device=dev))


# ---- one block of each kind ----------------------------------------------------------------------------------------------------------------------------------------
def _make_block(kind, dev):
    def down(cin, cout, s):
        return torch.nn.Sequential(resnet._Conv(cin, cout, kernel_size=1, stride=s, bias=False), torch.nn.BatchNorm2d(cout))
    blk = {'basic': lambda: resnet.BasicBlock(8, 8),
           'basic-down-s2': lambda: resnet.BasicBlock(8, 16, 2, down(8, 16, 2)),
           'bottleneck': lambda: resnet.Bottleneck(16, 4),
           'bottleneck-down': lambda: resnet.Bottleneck(8, 4, 1, down(8, 16, 1)),
           'bottleneck-down-s2': lambda: resnet.Bottleneck(8, 4, 2, down(8, 16, 2))}[kind]()
    _init_block(blk, 31)
    return blk.to(dev)


def _restated(blk, x):
    """resnet.py:42-69 / :89-120 of the reference in plain torch, on the parameters of `blk`"""
    def conv(c, u):
        return F.conv2d(u, c.weight, None, c.stride, c.padding)

    def bn(m, u):
        return F.batch_norm(u, m.running_mean, m.running_var, m.weight, m.bias, m.training, m.momentum, m.eps)
    shortcut = x if blk.downsample is None else bn(blk.downsample[1], conv(blk.downsample[0], x))
    pairs, out = blk._pairs(), x
    for c, m in pairs[:-1]:
        out = F.relu(bn(m, conv(c, out)))
    c, m = pairs[-1]
    return F.relu(bn(m, conv(c, out)) + shortcut)


KINDS = ['basic', 'basic-down-s2', 'bottleneck', 'bottleneck-down', 'bottleneck-down-s2']


@pytest.mark.parametrize('plane', [(4, 6), (9, 7)], ids=['4x6', '9x7'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('kind', KINDS)
def test_block_vs_plain_torch(backend, kind, training, plane):
    blk = _make_block(kind, backend.dev)
    ref = copy.deepcopy(blk).cpu()
    blk.train(training); ref.train(training)
    cin = blk.conv1.in_channels
    g = torch.Generator(device='cpu').manual_seed(3)
    x0 = torch.randn(2, cin, *plane, generator=g, device='cpu')
    x, xr = x0.clone().to(backend.dev).requires_grad_(True), x0.clone().requires_grad_(True)
    y, yr = blk(x), _restated(ref, xr)
    assert y.shape == yr.shape
    close(y.detach().cpu(), yr.detach())
    G = torch.randn(*yr.shape, generator=g, device='cpu')
    y.backward(G.to(backend.dev)); yr.backward(G)
    close(x.grad.cpu(), xr.grad, 1e-4)
    got, want = dict(blk.named_parameters()), dict(ref.named_parameters())
    assert sorted(got) == sorted(want)
    for k in want:
        close(got[k].grad.cpu(), want[k].grad, 1e-4)
    for (k, b), (_, br) in zip(blk.named_buffers(), ref.named_buffers()):
        if k.endswith('num_batches_tracked'):
            assert int(b) == (1 if training else 0), k                 # F.batch_norm keeps no counter: nn.BatchNorm2d would have counted one step
        else:
            close(b.cpu(), br, 1e-5)
            assert training != torch.equal(br, dict(_make_block(kind, 'cpu').named_buffers())[k]), k     # the statistics moved in train mode only


@pytest.mark.parametrize('plane', [(4, 6), (9, 7)], ids=['4x6', '9x7'])
@pytest.mark.parametrize('kind', KINDS)
def test_folded_block_vs_fp64_referee(backend, kind, plane):
    """the bar of test_fold_batchnorm.py for MBConv blocks: folded within 3e-5 of the scale of the fp64 restatement, or within REFEREE x the unfolded forward's distance"""
    blk = _make_block(kind, backend.dev).eval()
    g = torch.Generator(device='cpu').manual_seed(4)
    x0 = torch.randn(2, blk.conv1.in_channels, *plane, generator=g, device='cpu')
    with torch.no_grad():
        ref = _restated(copy.deepcopy(blk).cpu().double(), x0.double())
        x = x0.to(backend.dev)
        y_unfolded = blk(x)
        y_folded = blk.forward_folded(x, blk.folded_operands())
    assert y_folded.shape == ref.shape and not y_folded.requires_grad
    scale = ref.abs().max().item()
    d_unf = (y_unfolded.cpu().double() - ref).abs().max().item()
    d_fold = (y_folded.cpu().double() - ref).abs().max().item()
    print('%s %s: |folded - fp64| = %.3e, |unfolded - fp64| = %.3e, scale %.3e' % (kind, plane, d_fold, d_unf, scale))
    assert d_fold <= max(3e-5 * scale, REFEREE * d_unf), (d_fold, d_unf, scale)


# ---- the stem's max-pool: zero padding behind a ReLU equals torch's -inf padding ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('plane', [(9, 7), (8, 12)], ids=['9x7', '8x12'])
def test_maxpool_behind_relu_vs_aten(backend, plane):
    g = torch.Generator(device='cpu').manual_seed(9)
    x0 = torch.randn(2, 3, *plane, generator=g, device='cpu')
    x0[:, :, :2, :2] = -x0[:, :, :2, :2].abs() - 0.1                    # the window of output (0, 0) holds zeros only behind the ReLU (and five padded cells)
    x0[1, 2, -3:, -3:] = -1.0                                          # ... and the last window of one plane
    x, xr = x0.clone().to(backend.dev).requires_grad_(True), x0.clone().requires_grad_(True)
    y = resnet.ResNet._maxpool(SF.add_relu(x))
    yr = F.max_pool2d(F.relu(xr), 3, 2, 1)
    assert y.shape == yr.shape and (yr[:, :, 0, 0] == 0).all() and yr[1, 2, -1, -1] == 0
    assert torch.equal(y.detach().cpu(), yr.detach())
    G = torch.randint(-16, 17, yr.shape, generator=g, device='cpu').float() / 8      # eighths: the sums over the windows that share a maximum are exact
    y.backward(G.to(backend.dev)); yr.backward(G)
    assert torch.equal(x.grad.cpu(), xr.grad)
