"""The stride-1 siblings of the fused MBConv entry (segx_bn_dw_s1_fwd / _bwd, SF.bn_act_dwconv_s1, MBConvBlock.fused_entry_s1, EfficientNet.fused_stem_entry): BatchNorm +
swish + a 'same' k x k stride-1 depthwise convolution as one team launch per direction, against torch on the CPU in float64 -- on the emulator and on the device.

Yardstick: tests/test_bn_dw_s2.py's, reused literally (_within_rule): both routes run on the same seeded inputs; for every output
    err_new <= max(2 * err_old, 4 ulp of the reference tensor's largest magnitude),
each error the largest absolute difference from the float64 reference, err_old the route SF.bn_act -> SF.dwconv2d.  The BatchNorm's mean, var and running statistics are
required to be bit-identical to SF.bn_act's, num_batches_tracked to tick once on both routes.  One channel has mean ~ 50 and unit variance.

Shapes: under knob BN_PATH = 2 the team BatchNorm -- and with it the pair -- holds a plane of <= 4096 floats as one chunk of 4 float4 per lane and larger planes in chunks of
16 float4 per lane (16384 floats).  New against stride 2: a member's windows reach (k - 1) / 2 rows into BOTH neighbours' chunks, forward (rows of e) and backward (rows
of g_d)."""
import functools
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd.efficientnet.model import MBConvBlock, EfficientNet, Conv2dStaticSamePadding
from test_bn_dw_s2 import _within_rule, _params, _swish, KEYS, STATS, EPS

_id = lambda c: 'x'.join(map(str, c))


def _pad(case):
    k = case[4]
    return ((k - 1) // 2,) * 4


def _chunk_rows(case):
    """rows of one team member's chunk under BN_PATH = 2"""
    B, C, H, W, k = case
    return (4096 if H * W <= 4096 else 16384) // W


def _inputs(case, edge):
    B, C, H, W, k = case
    g = torch.Generator(device='cpu').manual_seed(23 + B + 3 * C + H + 5 * k)
    e = torch.randn(B, C, H, W, generator=g, device='cpu') * 1.5 + 0.3
    e[:, C - 1] = torch.randn(B, H, W, generator=g, device='cpu') + 50.0          # mean ~ 50, unit variance: the variance must not cancel
    gd = torch.randn(B, C, H, W, generator=g, device='cpu')
    keep = torch.zeros(H, W, dtype=torch.bool, device='cpu')
    if edge == 'members':                                              # the two rows either side of every member boundary
        for r in range(_chunk_rows(case), H, _chunk_rows(case)):
            keep[r - 2:r + 2] = True
    elif edge == 'first':
        keep[0, :] = True; keep[:, 0] = True
    elif edge == 'last':
        keep[-1, :] = True; keep[:, -1] = True
    else:
        keep[:] = True
    return e, gd * keep


def _run(dev, L, case, fused, path, edge=None):
    B, C, H, W, k = case
    bn, wdw = _params(C, k)
    bn, wdw = bn.to(dev), wdw.to(dev).requires_grad_(True)
    e0, gd = _inputs(case, edge)
    e = e0.to(dev).requires_grad_(True)
    with L.tuned(bn_path=path):
        if fused:
            assert SF.bn_dw_s1_ok(e.shape, k, 1, _pad(case)), case
            d = SF.bn_act_dwconv_s1(e, bn, wdw, 1, _pad(case))
        else:
            a = SF.bn_act(e, bn, SF.ACT_SWISH)
            d = SF.dwconv2d(a, wdw, 1, _pad(case))
        fn = d.grad_fn if fused else a.grad_fn          # the saved batch statistics: (e, [mean, var], ...) of the fused op, (x, mean, var, ...) of SF.bn_act
        assert not fused or len(fn.saved_tensors) == 5, 'the fused op saves e, the statistics and the parameters: no swish(bn(e))'
        mean, var = [t.detach().clone() for t in ((fn.saved_tensors[1][0], fn.saved_tensors[1][1]) if fused else (fn.saved_tensors[1], fn.saved_tensors[2]))]
        (d * gd.to(dev)).sum().backward()
    L.team_check()
    out = dict(d=d, de=e.grad, dw0=bn.weight.grad, db0=bn.bias.grad, dWdw=wdw.grad, mean=mean, var=var, rm=bn.running_mean, rv=bn.running_var)
    return {n: t.detach().cpu().clone() for n, t in out.items()}, int(bn.num_batches_tracked)


@functools.lru_cache(maxsize=None)
def _reference(case, edge=None):
    """float64 on the CPU: BatchNorm (batch statistics) -> swish -> zero 'same' padding -> depthwise convolution; computed once per case"""
    B, C, H, W, k = case
    bn, wdw = _params(C, k)
    e0, gd = _inputs(case, edge)
    e, w, wb, bb = e0.double().requires_grad_(True), wdw.double().requires_grad_(True), bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    m, v = e.mean((0, 2, 3)), e.var((0, 2, 3), unbiased=False)
    a = (e - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS) * wb[None, :, None, None] + bb[None, :, None, None]
    d = F.conv2d(F.pad(_swish(a), _pad(case)), w, stride=1, groups=C)
    assert d.shape == e.shape
    (d * gd.double()).sum().backward()
    out = dict(d=d, de=e.grad, dw0=wb.grad, db0=bb.grad, dWdw=w.grad)
    return {n: t.detach().clone() for n, t in out.items()}


def _compare(backend, case, path, edge=None):
    new, tick_new = _run(backend.dev, backend.L, case, True, path, edge)
    old, tick_old = _run(backend.dev, backend.L, case, False, path, edge)
    assert tick_new == tick_old == 1
    for n in STATS:
        assert torch.equal(new[n], old[n]), '%s: BatchNorm %s is not bit-identical to SF.bn_act\'s' % (case, n)
    _within_rule(new, old, _reference(case, edge), KEYS, '%s%s' % (case, ' ' + edge if edge else ''))


# (B, C, H, W, k), 'same' padding
TEAM = [(2, 3, 48, 64, 3),          # one partial member of 4 float4 per lane, odd C, H != W
        (1, 2, 32, 128, 5),         # exactly one full member of 4 float4 per lane, B = 1
        (5, 2, 32, 128, 5),         # B = 5
        (1, 2, 72, 16, 5),          # the narrowest rows served (a k index is 64 rows), partial single member
        (1, 2, 160, 256, 3),        # a first, an interior and a half-filled last member of 16 float4 per lane: halos cross both member boundaries in both directions
        (2, 1, 96, 512, 5),         # three whole members, the widest rows: a k index is two rows, so each k = 5 halo is a whole k index
        (1, 1, 640, 64, 5)]         # three members, partial last, a k index is 16 rows


@pytest.mark.parametrize('case', TEAM, ids=_id)
def test_fused_pair_matches_fp64_like_two_launches(backend, case):
    _compare(backend, case, 2)


BOUNDARY = [(1, 2, 160, 256, 3), (2, 2, 96, 512, 5)]


@pytest.mark.parametrize('edge', ['members', 'first', 'last'])
@pytest.mark.parametrize('case', BOUNDARY, ids=_id)
def test_gradient_on_boundary_rows_only(backend, case, edge):
    B, C, H, W, k = case
    P = (k - 1) // 2
    nz = _reference(case, edge)['dWdw'][:, 0] != 0                      # dWdw[ky][kx] = sum e'[y][x] g_d[y - ky + P][x - kx + P]
    want = torch.ones(k, k, dtype=torch.bool, device='cpu')
    if edge == 'first':                                                 # g_d's row 0 reaches the taps ky >= P, its column 0 the taps kx >= P
        want[:P, :P] = False
    elif edge == 'last':
        want[P + 1:, P + 1:] = False
    assert torch.equal(nz, want[None].expand(C, k, k)), 'the case would pass on zeros'
    _compare(backend, case, 2, edge=edge)


# the forms the library picks by itself: 16 float4 per lane (both directions) and 32 forward / 16 backward; device only
@pytest.mark.gpu
@pytest.mark.parametrize('case', [(1, 2, 256, 256, 3), (1, 2, 128, 128, 5), (3, 1, 512, 512, 3)], ids=_id)
def test_fused_pair_at_the_products_own_form(case):
    from conftest import _Backend
    from segtran_amd import segx
    segx.use_library(None)
    _compare(_Backend('hip'), case, 0)


def test_predicate(backend):
    ok = backend.L.bn_dw_s1_ok
    with backend.L.tuned(bn_path=2):
        assert ok(2, 3, 48, 64, 3, 1, 1, 1) and ok(1, 2, 72, 16, 5, 1, 2, 2) and ok(1, 1, 640, 64, 5, 1, 2, 2) and ok(2, 3, 47, 64, 3, 1, 1, 1)
        assert not ok(2, 3, 48, 64, 3, 2, 1, 1) and not ok(2, 3, 48, 64, 3, 2, 0, 0)                # stride 2
        assert not backend.L.bn_dw_s2_ok(2, 3, 48, 64, 3, 1, 1, 1)                                  # and the stride-2 pair keeps refusing stride 1
        assert not ok(2, 3, 48, 64, 4, 1, 1, 1) and not ok(2, 3, 48, 64, 7, 1, 3, 3) and not ok(2, 3, 48, 64, 1, 1, 0, 0)        # even or other k
        assert not ok(2, 3, 48, 64, 3, 1, 0, 0) and not ok(2, 3, 48, 64, 5, 1, 1, 1) and not ok(2, 3, 48, 64, 3, 1, 1, 0) and not ok(2, 3, 48, 64, 5, 1, 2, 1)    # pads
        assert not ok(2, 3, 48, 96, 3, 1, 1, 1) and not ok(2, 3, 48, 66, 3, 1, 1, 1) and not ok(2, 3, 480, 8, 3, 1, 1, 1) and not ok(2, 3, 4, 1024, 3, 1, 1, 1)   # W
        assert not ok(2, 3, 96, 64, 3, 1, 1, 1)                                                     # 6144 floats: the team BatchNorm's 8 float4 per lane are not instantiated
        assert not ok(1, 2, 1200, 16, 3, 1, 1, 1)                                                   # 16 float4 per lane of 16-float rows: the backward's image of g_d does not fit
        assert SF.bn_dw_s1_ok((2, 3, 48, 64), 3, 1, (1, 1, 1, 1)) and SF.bn_dw_s1_ok((2, 3, 48, 64), 5, 1, (2, 2, 2, 2))
        assert not SF.bn_dw_s1_ok((2, 3, 48, 64), 3, 1, (1, 0, 1, 0)) and not SF.bn_dw_s1_ok((2, 3, 48, 64), 5, 1, (2, 2, 2, 1)) and not SF.bn_dw_s1_ok((2, 3, 48, 64), 3, 1, (0, 0, 0, 0))
        assert not SF.bn_dw_s1_ok((2, 3, 48, 64), 3, 2, (1, 1, 1, 1)) and not SF.bn_dw_s1_ok((3, 48, 64), 3, 1, (1, 1, 1, 1))
    # the default policy: the model's shapes at batch 6 (stage 2, stage 3, the stem pair); planes under 16384 floats keep the resident / two-launch BatchNorm
    assert ok(6, 192, 256, 256, 3, 1, 1, 1) and ok(6, 336, 128, 128, 5, 1, 2, 2) and ok(6, 48, 512, 512, 3, 1, 1, 1)
    assert not ok(6, 4, 64, 64, 3, 1, 1, 1) and not ok(2, 3, 48, 64, 3, 1, 1, 1) and not ok(1, 2, 64, 128, 5, 1, 2, 2)
    with backend.L.tuned(bn_path=1):                                                                # no teams: no fused pair
        assert not ok(6, 192, 256, 256, 3, 1, 1, 1)


# ---- block level: one stride-1 MBConv block (k 3, expansion 6, 4 -> 4 channels: the skip is live) at 2 x 4 x 48 x 64, training -----------------------------------
def _fill(mod, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.2) + (1.0 if n.endswith('.weight') and p.dim() == 1 else 0.0))
    return mod


def _make_block(dev):
    with torch.device('cpu'):
        blk = _fill(MBConvBlock(3, 1, 6, 4, 4, 0.25, 64), 79)
    return blk.to(dev).train()


def _block_io():
    g = torch.Generator(device='cpu').manual_seed(8)
    return torch.randn(2, 4, 48, 64, generator=g, device='cpu'), torch.randn(2, 4, 48, 64, generator=g, device='cpu')


def _count(monkeypatch, L):
    calls = []
    real = type(L).bn_dw_s1_fwd

    def counted(self, *a):
        calls.append(1)
        return real(self, *a)
    monkeypatch.setattr(type(L), 'bn_dw_s1_fwd', counted)
    return calls


def _grads(res, mod):
    res.update({n: p.grad.detach().cpu().clone() for n, p in mod.named_parameters() if not n.startswith('_fc')})       # (_fc: kept for checkpoints, never used)
    return res


def _run_block(dev, L, monkeypatch, fused):
    blk = _make_block(dev)
    x0, G = _block_io()
    x = x0.to(dev).requires_grad_(True)
    monkeypatch.setattr(MBConvBlock, 'fused_entry_s1', fused)
    with L.tuned(bn_path=2):
        if SF.mbconv_mid_ok((2, 24, 48, 64), 3):
            monkeypatch.setattr(MBConvBlock, 'fused_middle', False)
        out = blk(x)
        (out * G.to(dev)).sum().backward()
    return _grads({'out': out.detach().cpu().clone(), 'dx': x.grad.cpu().clone()}, blk), [int(bn.num_batches_tracked) for bn in (blk._bn0, blk._bn1, blk._bn2)]


def _bn64(t, m):
    mu, v = t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=False)
    return (t - mu[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + m.eps) * m.weight[None, :, None, None] + m.bias[None, :, None, None]


def _block64(blk, a, skip_in):
    """float64 MBConv block from swish(bn0(.)) = a on: depthwise convolution, bn1 + swish, squeeze-excite, projection, bn2 (+ skip)"""
    dw = blk._depthwise_conv
    d = F.conv2d(F.pad(a, dw.static_pad), dw.weight, stride=1, groups=a.shape[1])
    y = _swish(_bn64(d, blk._bn1))
    gate = torch.sigmoid(F.conv2d(_swish(F.conv2d(y.mean((2, 3), keepdim=True), blk._se_reduce.weight, blk._se_reduce.bias)), blk._se_expand.weight, blk._se_expand.bias))
    out = _bn64(F.conv2d(y * gate, blk._project_conv.weight), blk._bn2)
    return out if skip_in is None else out + skip_in


def _reference_block():
    blk = _make_block('cpu').double()
    x0, G = _block_io()
    x = x0.double().requires_grad_(True)
    out = _block64(blk, _swish(_bn64(F.conv2d(x, blk._expand_conv.weight), blk._bn0)), x)
    (out * G.double()).sum().backward()
    return _grads({'out': out.detach(), 'dx': x.grad.clone()}, blk)


def test_block_fused_entry_s1_on_and_off(backend, monkeypatch):
    calls = _count(monkeypatch, backend.L)
    new, ticks_new = _run_block(backend.dev, backend.L, monkeypatch, True)
    assert len(calls) == 1, 'the fused stride-1 entry did not run'
    old, ticks_old = _run_block(backend.dev, backend.L, monkeypatch, False)
    assert len(calls) == 1, 'fused_entry_s1 = False still took the fused route'
    assert ticks_new == ticks_old == [1, 1, 1]
    ref = _reference_block()
    _within_rule(new, old, ref, sorted(ref), 'block')


def test_block_under_synchronised_batchnorm_or_eval_keeps_the_old_route(backend, monkeypatch):
    calls = _count(monkeypatch, backend.L)
    x = _block_io()[0].to(backend.dev)
    with backend.L.tuned(bn_path=2), torch.no_grad():
        if SF.mbconv_mid_ok((2, 24, 48, 64), 3):
            monkeypatch.setattr(MBConvBlock, 'fused_middle', False)
        want = _make_block(backend.dev)(x).cpu()
        assert len(calls) == 1
        monkeypatch.setattr(SF, '_bn_stats_sync', lambda loc: (loc, 1))      # a world of one rank: the gathered partials are the local ones
        got = _make_block(backend.dev)(x).cpu()
        assert len(calls) == 1, 'the fused entry ran under synchronised BatchNorm'
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4)
        monkeypatch.setattr(SF, '_bn_stats_sync', None)
        _make_block(backend.dev).eval()(x)
        assert len(calls) == 1, 'the fused entry ran in eval mode'


# ---- the stem pair: stem convolution -> [_bn0 + swish -> block 0's depthwise convolution] -> rest of block 0 -> head, on a 2 x 3 x 32 x 128 input -------------------
def _make_stem_net(dev):
    """EfficientNet-B0 cut down to its stem, block 0 (no expansion, no skip: 32 -> 16 channels) and a head of 8 channels; stem stride 1, so the stem's planes are 32 x 128"""
    with torch.device('cpu'):
        net = EfficientNet.from_name('efficientnet-b0', stem_stride=1, drop_connect_rate=0.0)
        net._blocks = torch.nn.ModuleList([net._blocks[0]])
        net.endpoint_blk_indices = [1]
        net._conv_head = Conv2dStaticSamePadding(16, 8, 1, image_size=128, bias=False)
        net._bn1 = torch.nn.BatchNorm2d(8, momentum=net._bn0.momentum, eps=net._bn0.eps)
        net._fc = torch.nn.Linear(8, 2)
        _fill(net, 80)
    return net.to(dev).train()


def _stem_io():
    g = torch.Generator(device='cpu').manual_seed(9)
    return torch.randn(2, 3, 32, 128, generator=g, device='cpu'), torch.randn(2, 8, 32, 128, generator=g, device='cpu')


def _run_stem(dev, L, monkeypatch, fused):
    net = _make_stem_net(dev)
    x0, G = _stem_io()
    x = x0.to(dev).requires_grad_(True)
    monkeypatch.setattr(EfficientNet, 'fused_stem_entry', fused)
    with L.tuned(bn_path=2):
        assert net._stem_into_block0(x) == fused
        ends = net.extract_endpoints(x)
        assert list(ends) == ['reduction_1']
        out = ends['reduction_1']
        (out * G.to(dev)).sum().backward()
    res = _grads({'out': out.detach().cpu().clone(), 'dx': x.grad.cpu().clone()}, net)
    return res, [int(bn.num_batches_tracked) for bn in (net._bn0, net._blocks[0]._bn1, net._blocks[0]._bn2, net._bn1)]


def _reference_stem():
    net = _make_stem_net('cpu').double()
    x0, G = _stem_io()
    x = x0.double().requires_grad_(True)
    st = net._conv_stem
    a = _swish(_bn64(F.conv2d(F.pad(x, st.static_pad), st.weight, stride=1), net._bn0))
    out = _swish(_bn64(F.conv2d(_block64(net._blocks[0], a, None), net._conv_head.weight), net._bn1))
    (out * G.double()).sum().backward()
    return _grads({'out': out.detach(), 'dx': x.grad.clone()}, net)


def test_stem_pair_on_and_off(backend, monkeypatch):
    calls = _count(monkeypatch, backend.L)
    new, ticks_new = _run_stem(backend.dev, backend.L, monkeypatch, True)
    assert len(calls) == 1, 'the stem pair did not run'
    old, ticks_old = _run_stem(backend.dev, backend.L, monkeypatch, False)
    assert len(calls) == 1, 'fused_stem_entry = False still took the fused route'
    assert ticks_new == ticks_old == [1, 1, 1, 1]
    ref = _reference_stem()
    assert sorted(ref) == sorted(new) == sorted(old)
    _within_rule(new, old, ref, sorted(ref), 'stem')


def test_stem_pair_not_in_eval_folded_or_synchronised_mode(backend, monkeypatch):
    calls = _count(monkeypatch, backend.L)
    net = _make_stem_net(backend.dev)
    x = _stem_io()[0].to(backend.dev)
    with backend.L.tuned(bn_path=2), torch.no_grad():
        assert net._stem_into_block0(x)
        monkeypatch.setattr(SF, '_bn_stats_sync', lambda loc: (loc, 1))
        assert not net._stem_into_block0(x)
        monkeypatch.setattr(SF, '_bn_stats_sync', None)
        net.eval()
        assert not net._stem_into_block0(x)
        want = net.extract_endpoints(x)['reduction_1'].cpu()
        net.fold_batchnorm()
        assert net.batchnorm_folded and not net._stem_into_block0(x)
        got = net.extract_endpoints(x)['reduction_1'].cpu()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    assert not calls
    with backend.L.tuned(bn_path=1):                                    # no team BatchNorm: the shape is not served
        assert not net.train()._stem_into_block0(x)
