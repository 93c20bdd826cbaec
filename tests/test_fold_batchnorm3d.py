"""BatchNorm3d folded into the I3D backbone's kernels for inference (InceptionI3d.fold_batchnorm, infer3d.fold_batchnorm): the ReLU GEMM epilogue, the implicit-GEMM
and halo convolutions with bias + ReLU, a folded Inception module against an fp64 referee, a short folded backbone (no BatchNorm launch, no pack launch after the
first call, the fold dropped by train()), and the fold's lifecycle.  Runs on the fiber emulator here and on the HIP build under -m gpu."""
import copy
import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd import infer3d, segx
from segtran_amd.networks.aj_i3d.aj_i3d import InceptionI3d, InceptionModule, Unit3D
from test_kernels_backbone import rnd, close
from test_fold_batchnorm import REFEREE

FOLD_ABS = 3e-5          # test_fold_batchnorm.py's rule: d_fold <= max(3e-5 * scale, REFEREE * d_unfolded)


@pytest.fixture(params=['x6', 'f32'])
def engine_name(request, backend):
    L = segx.lib()
    prev = L.set_engine(request.param)
    yield request.param
    L.set_engine(prev)


def _clamping_bias(ref_nobias, seed):
    """a per-channel bias shifted negative so that a good share of relu(ref + b) clamps; returns (bias, clamped share of the fp64 reference)"""
    C = ref_nobias.shape[1]
    b = rnd(C, seed=seed, scale=0.5) - 0.3 * ref_nobias.std().item()
    share = ((ref_nobias + b.double().view(1, -1, *([1] * (ref_nobias.dim() - 2)))) <= 0).double().mean().item()
    return b, share


# ---- 1. the GEMM's ReLU epilogue ------------------------------------------------------------------------------------------------------------------
# I3D channel pairs at 4 x 4 x 4 (528: K % 32 == 16), and a ragged one with S = 63 (no float4 multiple: the scalar loaders)
@pytest.mark.parametrize('Cin,Cout,B,size', [(192, 176, 2, (4, 4, 4)), (528, 448, 1, (4, 4, 4)), (832, 128, 1, (4, 4, 4)), (24, 150, 2, (3, 3, 7))])
def test_relu_epilogue_gemm(engine_name, Cin, Cout, B, size):
    x = rnd(B, Cin, *size, seed=1)
    w = rnd(Cout, Cin, 1, 1, 1, seed=2, scale=Cin ** -0.5)
    S = size[0] * size[1] * size[2]
    ref0 = F.conv3d(x.double(), w.double())
    b, share = _clamping_bias(ref0, 3)
    print('relu gemm %d -> %d: %.1f %% of the outputs clamp' % (Cin, Cout, 100 * share))
    assert 0.2 <= share <= 0.8
    ref = torch.relu(F.conv3d(x.double(), w.double(), b.double()))
    L = segx.lib()
    L.x6_launches()
    y = SF.conv1x1_relu(x, w, b)
    assert (L.x6_launches() > 0) == (engine_name == 'x6' and S % 4 == 0 and Cin % 4 == 0 and S > 48)        # the engine under test really ran it
    assert y.shape == ref.shape and not y.requires_grad
    close(y.double(), ref)
    close(SF.conv1x1_relu(x, w, None).double(), torch.relu(ref0))
    # into a channel slice of a wider tensor (the branch's place in an Inception module's concatenation): nothing else is touched
    if S % 4 == 0:
        wide = torch.full((B, Cout + 16, *size), 7.0)
        out = SF.conv1x1_relu(x, w, b, out=wide[:, 8:8 + Cout])
        assert out.data_ptr() == wide[:, 8:].data_ptr()
        assert torch.equal(wide[:, 8:8 + Cout], y)
        assert torch.equal(wide[:, :8], torch.full((B, 8, *size), 7.0)) and torch.equal(wide[:, 8 + Cout:], torch.full((B, 8, *size), 7.0))
    else:
        with pytest.raises(ValueError, match='16-byte'):
            SF.conv1x1_relu(x, w, b, out=torch.empty(B, Cout + 1, *size)[:, 1:])


def test_relu_epilogue_refusals(backend):
    x, w = rnd(1, 8, 4, 4, seed=1), rnd(16, 8, 1, 1, seed=2)
    L, wd = segx.lib(), w.reshape(16, 8).contiguous()
    y = torch.empty(1, 16, 4, 4)
    with pytest.raises(RuntimeError, match='relu'):
        L.gemm(wd, x, y, 16, 16, 8, (0, 0, 8, 1), (128, 0, 1, 16), (256, 0, 16), epilogue=segx.EPI_RELU, resid=torch.zeros_like(y))
    with pytest.raises(RuntimeError, match='relu'):
        L.gemm(wd, x, y, 16, 16, 8, (0, 0, 8, 1), (0, 0, 8, 1), (0, 0, 16), epilogue=segx.EPI_RELU)
    with pytest.raises(RuntimeError, match='split-K'):
        L.gemm(wd, x, y, 16, 16, 8, (0, 0, 8, 1), (128, 0, 1, 16), (256, 0, 16), epilogue=segx.EPI_RELU, splitk=2, workspace=torch.empty(2 * 256))
    assert L.gemm_route(wd, x, 16, 16, 8, (0, 0, 8, 1), (128, 0, 1, 16), epilogue=segx.EPI_RELU)[1] == L.gemm_route(wd, x, 16, 16, 8, (0, 0, 8, 1), (128, 0, 1, 16),
                                                                                                                  epilogue=segx.EPI_SWISH)[1]


# ---- 2. implicit GEMM with bias + ReLU -------------------------------------------------------------------------------------------------------------
# (Cin, Cout, input extent, window, stride, pads): the space-to-depth stem's geometry; rows that are no multiple of 4; unpacked filters (Cin = 4); Cout 40 and 136
IGEMM = {'s2d-stem': (8, 64, (8, 8, 7), (7, 7, 4), (2, 2, 1), ((2, 3), (2, 3), (0, 0))),
         'rows-of-7': (16, 24, (6, 7, 7), (3, 3, 3), (1, 1, 1), ((1, 1), (1, 1), (1, 1))),
         'unpacked-cin4': (4, 16, (4, 5, 6), (3, 3, 3), (1, 1, 1), ((1, 1), (1, 1), (1, 1))),
         'cout40': (8, 40, (4, 4, 8), (3, 3, 3), (1, 1, 1), ((1, 1), (1, 1), (1, 1))),
         'cout136': (8, 136, (4, 4, 8), (3, 3, 3), (1, 1, 1), ((1, 1), (1, 1), (1, 1)))}


@pytest.fixture(params=[('x6', 6), ('x6', 3), ('f32', 6)], ids=['x6', 'x6-3term', 'f32'])          # (the term count is a property of the bf16 engine)
def engine_terms(request, backend):
    L = segx.lib()
    prev = L.set_engine(request.param[0])
    yield request.param
    L.set_engine(prev)


@pytest.mark.parametrize('splitk', [1, 2])
@pytest.mark.parametrize('case', sorted(IGEMM))
def test_implicit_gemm_bias_relu(engine_terms, case, splitk):
    engine_name, terms = engine_terms
    Cin, Cout, size, k, stride, pads = IGEMM[case]
    B = 2
    L = segx.lib()
    out = tuple((n + p[0] + p[1] - kk) // s + 1 for n, p, kk, s in zip(size, pads, k, stride))
    geom = (Cin,) + size + out + k + stride + tuple(p[0] for p in pads)
    P, KV = out[0] * out[1] * out[2], k[0] * k[1] * k[2]
    packed = Cin % 8 == 0
    x = rnd(B, Cin, *size, seed=11)
    w = rnd(Cout, Cin, *k, seed=12, scale=(Cin * KV) ** -0.5)
    pad6 = (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1])
    ref0 = F.conv3d(F.pad(x.double(), pad6), w.double(), None, stride)
    b, share = _clamping_bias(ref0, 13)
    assert 0.2 <= share <= 0.8
    wk = w
    if packed:
        wk = torch.empty_like(w)
        L.conv3d_pack_weights(w, wk, Cout, Cin, KV, 0)

    def ws():
        return torch.empty(splitk * B * Cout * P) if splitk > 1 else None
    with L.tuned(x6_terms=terms):
        route = L.conv3d_route(B, Cout, geom, False, splitk, True, packed)         # the one route of the plain and of the bias + ReLU launch (conv_route)
        assert route[0] == ('x6' if engine_name == 'x6' and packed else 'f32') and route[4] == splitk
        plain, y = torch.empty(B, Cout, *out), torch.full((B, Cout, *out), -5.0)
        L.x6_launches(); L.x3_launches()
        L.conv3d_fwd(x, wk, plain, B, Cout, geom, splitk, ws(), packed=packed)
        counted = (L.x6_launches(), L.x3_launches())
        L.conv3d_fwd_bias_act(x, wk, b, y, B, Cout, geom, splitk, ws(), packed=packed, act=SF.ACT_RELU)
        assert (L.x6_launches(), L.x3_launches()) == counted == (int(route[0] == 'x6'), int(route[0] == 'x6' and terms == 3))
        want = torch.relu(plain + b.view(1, -1, 1, 1, 1))                            # fp32 add, then max
        assert torch.equal(y, want), 'not relu(plain + bias) bit for bit: max diff %.3e' % (y - want).abs().max().item()
        if terms == 6:
            close(y.double(), torch.relu(ref0 + b.double().view(1, -1, 1, 1, 1)))
        # act = 0: the bias alone
        L.conv3d_fwd_bias_act(x, wk, b, y, B, Cout, geom, splitk, ws(), packed=packed, act=SF.ACT_NONE)
        assert torch.equal(y, plain + b.view(1, -1, 1, 1, 1))
        if packed:
            # channel slices on both sides: x = channels 8.. of a wider tensor, y = channels 8 .. 8 + Cout of a wider one
            xw = torch.cat([rnd(B, 8, *size, seed=14), x], 1)
            yw = torch.full((B, Cout + 16, *out), 7.0)
            L.conv3d_fwd_bias_act(xw[:, 8:], wk, b, yw[:, 8:], B, Cout, geom, splitk, ws(), packed=True, x_bs=xw.stride(0), y_bs=yw.stride(0), act=SF.ACT_RELU)
            assert torch.equal(yw[:, 8:8 + Cout], want)
            assert torch.equal(yw[:, :8], torch.full((B, 8, *out), 7.0)) and torch.equal(yw[:, 8 + Cout:], torch.full((B, 8, *out), 7.0))
    with pytest.raises(RuntimeError, match='act'):
        L.conv3d_fwd_bias_act(x, wk, b, y, B, Cout, geom, 1, None, packed=packed, act=SF.ACT_SWISH)


# ---- 3. the halo kernel with bias + ReLU -----------------------------------------------------------------------------------------------------------
# extents: 5 x 6 x 9 and 9 x 5 x 4 tile in rows of 4, 4 x 5 x 16 in rows of 8; each mtile with a Cout that fills it partly, and two with several / one partial channel tile
@pytest.mark.parametrize('terms', [6, 3])
@pytest.mark.parametrize('size', [(5, 6, 9), (9, 5, 4), (4, 5, 16)])
@pytest.mark.parametrize('mtile,Cout', [(64, 40), (128, 136), (192, 200), (64, 136), (192, 40)])
def test_halo_bias_relu(backend, mtile, Cout, size, terms):
    L = backend.L
    B, Cin = 2, 8
    D, H, W = size
    geom = (Cin, D, H, W, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    x = rnd(B, Cin, *size, seed=21)
    w = rnd(Cout, Cin, 3, 3, 3, seed=22, scale=(Cin * 27) ** -0.5)
    b = rnd(Cout, seed=23, scale=0.5) - 0.3
    with L.tuned(engine=L.ENGINES['x6'], x6_terms=terms):
        wq = L.conv3d_halo_pack(w, Cout, Cin, 0)
        plain = torch.empty(B, Cout, *size)
        L.x6_launches(); L.x3_launches()
        L.conv3d_halo_fwd(x, wq, plain, B, Cout, geom, mtile=mtile)
        assert (L.x6_launches(), L.x3_launches()) == (1, int(terms == 3))
        want = torch.relu(plain + b.view(1, -1, 1, 1, 1))
        share = (want == 0).float().mean().item()
        assert 0.2 <= share <= 0.8
        xw = torch.cat([rnd(B, 8, *size, seed=24), x], 1)
        yw = torch.full((B, Cout + 3, *size), 7.0)
        L.conv3d_halo_bias_act_fwd(xw[:, 8:], wq, b, yw[:, 3:], B, Cout, geom, x_bs=xw.stride(0), y_bs=yw.stride(0), mtile=mtile, act=SF.ACT_RELU)
        assert (L.x6_launches(), L.x3_launches()) == (1, int(terms == 3))
    assert torch.equal(yw[:, 3:], want), 'not relu(halo + bias) bit for bit: max diff %.3e' % (yw[:, 3:] - want).abs().max().item()
    assert torch.equal(yw[:, :3], torch.full((B, 3, *size), 7.0))
    if terms == 6:
        close(want.double(), torch.relu(F.conv3d(x.double(), w.double(), b.double(), padding=1)))
    with pytest.raises(RuntimeError, match='act'):
        L.conv3d_halo_bias_act_fwd(x, wq, b, plain, B, Cout, geom, act=SF.ACT_SWISH)


# ---- 4. a folded Inception module against an fp64 referee -------------------------------------------------------------------------------------------
def _randomize(mod, seed):
    """convolution weights at fan-in scale; non-trivial BatchNorm state: mean != 0, var != 1, random gamma and beta"""
    i = 0
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv3d):
                fan = m.weight[0].numel()
                m.weight.copy_(rnd(*m.weight.shape, seed=seed + i, scale=(2.0 / fan) ** 0.5)); i += 1
            elif isinstance(m, torch.nn.BatchNorm3d):
                C = m.num_features
                m.weight.copy_(1 + 0.3 * rnd(C, seed=seed + i)); m.bias.copy_(0.3 * rnd(C, seed=seed + i + 1))
                m.running_mean.copy_(0.4 * rnd(C, seed=seed + i + 2)); m.running_var.copy_(0.5 + rnd(C, seed=seed + i + 3).abs())
                i += 4


def _unit_fp64(u, x):
    d = lambda t: t.detach().double()
    k, s = u._kernel_shape, u._stride
    pads = SF._same_pads(x.shape[2:], k, s)
    y = F.conv3d(F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1])), d(u.conv3d.weight), None, s)
    v = lambda t: d(t).view(1, -1, 1, 1, 1)
    return torch.relu((y - v(u.bn.running_mean)) / torch.sqrt(v(u.bn.running_var) + u.bn.eps) * v(u.bn.weight) + v(u.bn.bias))


def _pool_fp64(x, k, s):
    pads = SF._same_pads(x.shape[2:], k, s)
    return F.max_pool3d(F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1])), k, s)


def _module_fp64(m, x):
    return torch.cat([_unit_fp64(m.b0, x), _unit_fp64(m.b1b, _unit_fp64(m.b1a, x)), _unit_fp64(m.b2b, _unit_fp64(m.b2a, x)),
                      _unit_fp64(m.b3b, _pool_fp64(x, (3, 3, 3), (1, 1, 1)))], 1)


def _referee_rule(what, folded, unfolded, ref):
    scale = ref.abs().max().item()
    d_unf, d_fold = (unfolded.double() - ref).abs().max().item(), (folded.double() - ref).abs().max().item()
    print('%s: |folded - fp64| = %.3e, |unfolded - fp64| = %.3e, scale %.3e' % (what, d_fold, d_unf, scale))
    assert folded.shape == ref.shape and not folded.requires_grad
    assert d_fold <= max(FOLD_ABS * scale, REFEREE * d_unf), (what, d_fold, d_unf, scale)


@pytest.mark.parametrize('halo', [False, True], ids=['igemm', 'halo'])
def test_folded_inception_module_vs_fp64_referee(backend, halo):
    L = backend.L
    m = InceptionModule(32, [16, 16, 24, 8, 16, 8], 'm')
    _randomize(m, 31)
    m.eval()
    x = rnd(2, 32, 4, 6, 8, seed=5).abs()                      # (a module's input is a ReLU output)
    ref = _module_fp64(m, x.double())
    geom = (16, 4, 6, 8, 4, 6, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    with L.tuned(engine=L.ENGINES['x6'], **({'conv_halo_min_tiles': 1} if halo else {})):
        assert L.conv3d_halo_ok(2, 24, geom) == halo
        with torch.no_grad():
            y_unfolded = m(x)
        y_folded = m.forward_folded(x, m.folded_operands())      # grad mode is on here: no graph all the same
    _referee_rule('inception module (%s)' % ('halo' if halo else 'implicit GEMM'), y_folded, y_unfolded, ref)


# ---- 5. a short backbone: stem through Mixed_3b ----------------------------------------------------------------------------------------------------
SHORT = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2b_1x1', 'Conv3d_2c_3x3', 'MaxPool3d_3a_3x3', 'Mixed_3b')


def _short_backbone(seed=3):
    net = InceptionI3d(num_classes=4, in_channels=3, do_pool1=False)
    for name in list(net.end_points):
        if name not in SHORT:
            del net.end_points[name]
            delattr(net, name)
    _randomize(net, seed)
    return net


@pytest.fixture(scope='module')
def short_reference():
    """(input, fp64 endpoints of the short backbone) on the CPU, computed once"""
    net = _short_backbone()
    x = torch.randn(1, 3, 8, 32, 32, generator=torch.Generator().manual_seed(4))
    ref, u = {}, x.double()
    for name in SHORT:
        m = getattr(net, name)
        u = _unit_fp64(m, u) if isinstance(m, Unit3D) else _module_fp64(m, u) if isinstance(m, InceptionModule) else u if isinstance(m, torch.nn.Identity) else \
            _pool_fp64(u, m.kernel_size, m.stride)
        ref[name] = u
    return x, ref


def test_folded_short_backbone(backend, short_reference, monkeypatch):
    L = backend.L
    net = _short_backbone().to(backend.dev).eval()
    x = short_reference[0].to(backend.dev)
    with torch.no_grad():
        want = net.extract_features(x)
    assert net.fold_batchnorm() is net and net.batchnorm_folded

    def boom(name):
        def f(*a, **k):
            raise AssertionError(name + ' launched')
        return f
    bn_entries = [n for n in dir(type(L)) if n.startswith('bn_act')]
    assert 'bn_act_fwd2' in bn_entries
    packs = []
    with monkeypatch.context() as mp:
        for n in bn_entries:
            mp.setattr(type(L), n, boom(n))
        for n in ('conv3d_halo_pack', 'conv3d_pack_weights', 'conv3d_flip_weights'):
            orig = getattr(type(L), n)
            mp.setattr(type(L), n, (lambda o, nn: lambda self, *a, **k: (packs.append(nn), o(self, *a, **k))[1])(orig, n))
        got = net.extract_features(x)                          # no BatchNorm launch, no autograd graph (grad mode is on here)
        first = len(packs)
        again = net.extract_features(x)
        assert first > 0 and len(packs) == first, 'the second folded call launched a pack kernel: %s' % packs[first:]
    assert sorted(got) == sorted(want) == sorted(SHORT)
    for name in SHORT:
        assert torch.equal(again[name], got[name])
        _referee_rule(name, got[name].cpu(), want[name].cpu(), short_reference[1][name])
    net.unfold_batchnorm()
    assert not net.batchnorm_folded
    with monkeypatch.context() as mp:
        mp.setattr(type(L), 'bn_act_fwd2', boom('bn_act_fwd2'))
        with pytest.raises(AssertionError, match='bn_act_fwd2 launched'), torch.no_grad():
            net.extract_features(x)


def test_fold_is_dropped_by_train_and_the_backbone_is_the_unfolded_one_bit_for_bit(backend):
    """after train(), a train step (the short backbone's forward, a loss on its endpoints, backward) gives loss, gradients and running statistics bit-identical to a
    never-folded twin"""
    net = _short_backbone().to(backend.dev)
    twin = copy.deepcopy(net)
    net.eval().fold_batchnorm()
    assert net.batchnorm_folded
    net.train()
    assert not net.batchnorm_folded
    twin.train()
    x = rnd(2, 3, 4, 8, 8, seed=6)                           # (2 x 4 x 4 behind the stem, 2 x 2 x 2 in Mixed_3b: every layer still normalises over >= 16 values)
    out = []
    for m in (net, twin):
        ep = m.extract_features(x)
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
    assert n >= 27                                             # 9 convolutions + 9 BatchNorm layers (weight, bias)
    for (na, ba), (nb, bb) in zip(net.named_buffers(), twin.named_buffers()):
        assert torch.equal(ba, bb), na                         # running statistics moved identically


# ---- 6. lifecycle (host only) ---------------------------------------------------------------------------------------------------------------------------
def test_fold_lifecycle_of_the_3d_model():
    """no kernel runs: state_dict untouched, train mode refused, train() / load_state_dict() / an in-place change of a source tensor drop the fold; Segtran3d's own
    fold_batchnorm() keeps refusing and names the entry point"""
    import segtran_amd
    from segtran_amd import engine
    net = engine.build_model(dict(engine.CONFIGS['cfg4'], size=(112, 112, 16)), 'cpu', synth=False, attractors=64)
    bb = net.backbone
    _randomize(bb, 9)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(RuntimeError, match='eval'):
        infer3d.fold_batchnorm(net)
    assert not net.batchnorm_folded
    net.eval()
    with pytest.raises(NotImplementedError, match='infer3d.fold_batchnorm'):
        net.fold_batchnorm()
    with pytest.raises(NotImplementedError):
        segtran_amd.fold_batchnorm(net)
    assert not net.batchnorm_folded and not bb.batchnorm_folded
    assert infer3d.fold_batchnorm(net) is net and net.batchnorm_folded and bb.batchnorm_folded
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) and after[k].shape == before[k].shape for k in before)
    assert not any('fold' in n for n, _ in list(net.named_parameters()) + list(net.named_buffers()))
    # the fold algebra, against fp64 on the host: the stem, one pointwise layer and one 3 x 3 x 3 layer
    assert len(bb._folded[0]) == 57
    for path, unit in [('Conv3d_1a_7x7', bb.Conv3d_1a_7x7), ('Mixed_4c.b2a', bb.Mixed_4c.b2a), ('Mixed_3c.b1b', bb.Mixed_3c.b1b)]:
        w, b, ops = bb.folded_operands(path)
        bn = unit.bn
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        assert w.dtype == torch.float32 and not w.requires_grad and not isinstance(w, torch.nn.Parameter) and ops == {}
        assert torch.equal(w, (unit.conv3d.weight.detach().double() * s.view(-1, 1, 1, 1, 1)).float())
        assert torch.equal(b, (bn.bias.detach().double() - bn.running_mean.double() * s).float())
    net.train()
    assert not net.batchnorm_folded
    infer3d.fold_batchnorm(net.eval())
    net.load_state_dict(before)
    assert not net.batchnorm_folded
    infer3d.fold_batchnorm(net)
    with torch.no_grad():
        bb.Mixed_5c.b3b.bn.running_var.mul_(2.0)               # a source tensor changed in place: the folded operands are stale
    assert not net.batchnorm_folded
    assert infer3d.unfold_batchnorm(infer3d.fold_batchnorm(net)) is net
    assert not net.batchnorm_folded
    # fold_bn semantics of the evaluation entry point (infer2d._folded): folds for the block, leaves a net the caller folded as it is
    with infer3d._folded(net, True):
        assert net.batchnorm_folded
    assert not net.batchnorm_folded
    infer3d.fold_batchnorm(net)
    with infer3d._folded(net, True):
        pass
    assert net.batchnorm_folded
    with infer3d._folded(infer3d.unfold_batchnorm(net), False):
        assert not net.batchnorm_folded


def test_folded_functions_are_forward_only():
    x = torch.zeros(1, 8, 4, 4, 4)
    w1, w3, b = torch.zeros(8, 8, 1, 1, 1, requires_grad=True), torch.zeros(8, 8, 3, 3, 3, requires_grad=True), torch.zeros(8)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.conv1x1_relu(x, w1, b)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.conv3d_bias_relu(x, w3, b)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.conv3d_bias_relu(x.requires_grad_(True), w3.detach(), b)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.stem_bridge_conv_s2d_folded(torch.zeros(1, 4, 8, 8, 8), torch.zeros(64, 8, 7, 7, 4, requires_grad=True), torch.zeros(64, 4, 4, 4))
