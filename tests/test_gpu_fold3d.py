"""GPU (-m gpu): the 3-D eval forward with BatchNorm3d folded into the I3D backbone's kernels (infer3d.fold_batchnorm) at the small fixture size: the
reference fixtures' logits within the project's parity bar on both engines, the hardened maps wherever the unfolded forward decides them by more than that, no
BatchNorm launch; the same under inference_precision('bf16x3'); the sliding-window evaluation with fold_bn=True; and the replay from a captured graph."""
import numpy as np
import pytest
import torch

from segtran_amd import engine, infer3d, segx
from segtran_amd.synth import sample, synth_brats
from util import golden, assert_close
from test_gpu_x3_infer3d import BAR, DECIDED, EXCUSED_CAP

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.fixture(params=['x6', 'f32'])
def L(request):
    lib = segx.lib()
    prev = lib.set_engine(request.param)
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    yield lib
    lib.set_engine(prev)
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6, 'a test left the three-term mode on'


def _no_batchnorm(monkeypatch):
    """every bn_act* entry of the library object counts its calls (the pyramid's --inbn layers are off in these configurations)"""
    calls, cls = [], type(segx.lib())
    for n in [n for n in dir(cls) if n.startswith('bn_act')]:
        monkeypatch.setattr(cls, n, (lambda real, nn: lambda self, *a, **k: (calls.append(nn), real(self, *a, **k))[1])(getattr(cls, n), n))
    return calls


def _model(tag, cfg):
    g = golden(tag)
    net = engine.build_model(dict(engine.CONFIGS[cfg], size=(112, 112, 16)), DEV, dropout_prob=0.0, attractors=int(g['A'])).eval()
    x = synth_brats(1, 112, 112, 16, 1337)[0]
    assert torch.equal(sample(x), g['x_sample'])
    return g, net, x.to(DEV)


def _check_against_fixture(tag, g, y_fold, y_unf):
    want = g['logits']
    labels = torch.from_numpy(np.unpackbits(g['labels'].numpy())[:y_fold.numel()].astype(bool)).reshape(y_fold.shape)
    e_fold, e_unf = (sample(y_fold.cpu(), 65536) - want).abs().max().item(), (sample(y_unf.cpu(), 65536) - want).abs().max().item()
    print('%s: max |folded - unfolded| %.3e, max |folded - fixture| %.3e, max |unfolded - fixture| %.3e' % (tag, (y_fold - y_unf).abs().max().item(), e_fold, e_unf))
    assert e_fold < BAR
    decided = y_unf.cpu().abs() >= DECIDED
    assert torch.equal((y_fold.cpu() > 0)[decided], labels[decided]), 'a hardened label differs where the unfolded forward decides it by more than the bar'
    left_out = (~decided).float().mean().item()
    print('%s: %.3f %% of the cells have |unfolded| < %.1e' % (tag, 100 * left_out, DECIDED))
    assert left_out <= EXCUSED_CAP


@pytest.mark.parametrize('tag,cfg', [('seg3d_cfg4_eval', 'cfg4'), ('seg3d_cfg5_eval', 'cfg5')])
def test_folded_eval_forward_meets_the_parity_bar(L, tag, cfg, monkeypatch):
    g, net, x = _model(tag, cfg)
    with torch.no_grad():
        y_unf = net(x)
    assert infer3d.fold_batchnorm(net) is net and net.batchnorm_folded
    calls = _no_batchnorm(monkeypatch)
    y = net(x)                                              # grad mode on: the folded backbone builds no graph by itself
    assert not calls, 'the folded forward launched BatchNorm: %s' % calls
    with torch.no_grad():
        y2 = net(x)
    assert torch.equal(y2, y.detach())
    _check_against_fixture('%s folded' % tag, g, y.detach(), y_unf)
    infer3d.unfold_batchnorm(net)
    with torch.no_grad():
        assert torch.equal(net(x), y_unf) and calls


@pytest.mark.parametrize('tag,cfg', [('seg3d_cfg4_eval', 'cfg4'), ('seg3d_cfg5_eval', 'cfg5')])
def test_folded_eval_forward_in_three_terms(tag, cfg, monkeypatch):
    lib = segx.lib()
    prev = lib.set_engine('x6')
    try:
        g, net, x = _model(tag, cfg)
        with torch.no_grad():
            y_unf = net(x)
            infer3d.fold_batchnorm(net)
            y6 = net(x)
            calls = _no_batchnorm(monkeypatch)
            # the convolutions of the folded forward: every launch of the bf16 engine runs three-term
            conv, gemm = [], [0, 0]                       # per convolution call (name, bf16-engine launches, three-term launches); the GEMMs' share of both counters

            def counted(real, name):
                def f(self, *a, **k):
                    gemm[0] += self.x6_launches(); gemm[1] += self.x3_launches()
                    out = real(self, *a, **k)
                    conv.append((name, self.x6_launches(), self.x3_launches()))
                    return out
                return f
            for n in ('conv3d_halo_bias_act_fwd', 'conv3d_fwd_bias_act', 'conv3d_fwd', 'conv3d_halo_fwd'):
                monkeypatch.setattr(type(lib), n, counted(getattr(type(lib), n), n))
            lib.x6_launches(); lib.x3_launches()
            with infer3d.inference_precision('bf16x3'):
                y3 = net(x)
            gemm[0] += lib.x6_launches(); gemm[1] += lib.x3_launches()
        assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6          # the knob is back
        assert not calls
        n6, n3 = gemm[0] + sum(c[1] for c in conv), gemm[1] + sum(c[2] for c in conv)
        print('%s folded bf16x3: %d of %d bf16 tile-engine launches three-term (convolutions %d of %d in %d calls); max |y3 - y6| %.3e'
              % (tag, n3, n6, sum(c[2] for c in conv), sum(c[1] for c in conv), len(conv), (y3 - y6).abs().max().item()))
        assert n3 > 0 and any(c[0] == 'conv3d_halo_bias_act_fwd' for c in conv)
        assert all(c[1] == c[2] for c in conv), [c for c in conv if c[1] != c[2]]     # every bf16 convolution launch three-term
        assert not torch.equal(y3, y6)
        _check_against_fixture('%s folded bf16x3' % tag, g, y3, y_unf)
    finally:
        lib.set_engine(prev)


@pytest.mark.parametrize('form', ['composed-8-channel', 'bridge-not-composed'])
def test_folded_eval_forward_on_the_other_stem_forms(form, monkeypatch):
    """SEGX_STEM_S2D=0 (the 8-channel stride-2 composed stem) and fuse_input_bridge = False (the 3-channel stem behind the bridge): the implicit GEMM with a
    per-channel bias + ReLU instead of the bias-map pass"""
    g, net, x = _model('seg3d_cfg4_eval', 'cfg4')
    if form == 'composed-8-channel':
        net.stem_space_to_depth = False
    else:
        net.fuse_input_bridge = False
    with torch.no_grad():
        y_unf = net(x)
        infer3d.fold_batchnorm(net)
        calls = _no_batchnorm(monkeypatch)
        y = net(x)
    assert not calls
    _check_against_fixture('seg3d_cfg4_eval folded, %s stem' % form, g, y, y_unf)


def test_sliding_window_3d_folded_vs_reference():
    """tests/test_gpu_model.py::test_eval_path_3d_vs_reference with fold_bn=True, at its tolerances"""
    g = golden('eval3d')
    net = engine.build_model(dict(engine.CONFIGS['cfg4'], size=(112, 112, 16)), DEV, dropout_prob=0.0, attractors=int(g['A'])).eval()
    vol = synth_brats(1, 112, 168, 16, int(g['seed']))[0][0].to(DEV)
    args = (net, vol, (112, 112, 16), (112, 112, 16), 2, 56, 16, 'brats')
    hard, soft = infer3d.test_single_case(*args, fold_bn=True)
    assert not net.batchnorm_folded                          # folded for the call only
    assert_close(sample(soft.cpu(), 65536), g['soft'], 1e-5, 'soft')
    ref_bits = np.unpackbits(g['hard'].numpy())[:hard.numel()].astype(bool).reshape(hard.shape)
    safe = ((soft.cpu() - 0.5).abs() > 1e-5).numpy()
    assert np.array_equal((hard.cpu().numpy() > 0)[safe], ref_bits[safe]), 'hardened label map differs'
    infer3d.fold_batchnorm(net)
    hard2, soft2 = infer3d.test_single_case(*args, fold_bn=True)
    assert net.batchnorm_folded                              # a net the caller folded stays folded
    assert torch.equal(soft2, soft) and torch.equal(hard2, hard)


def test_folded_3d_eval_forward_replays_from_a_captured_graph():
    """one stream, warm-up on the capture stream (it fills the per-layer operand cache), default queue settings: the replay gives the eager folded result bit for bit"""
    g, net, x = _model('seg3d_cfg4_eval', 'cfg4')
    infer3d.fold_batchnorm(net)
    with torch.no_grad():
        eager = net(x).clone()
        xs = x.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(xs)                                          # warm-up on the capture stream: every workspace size is planned before the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(xs)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
