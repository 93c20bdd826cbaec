"""GPU (-m gpu): the non-squeezed self-attention (--nosqueeze with --pos bias / lsinu) and the multi-scale Mince attention at the token counts
they run at -- 64 x 64 = 4096 tokens (cfg2, 512^2), 72 x 72 = 5184 (576^2), 14 x 14 x 12 = 2352 (cfg4) -- where the score and P.V products take
other GEMM kernels than at toy size, rows of 4096 take the register-row softmax and rows of 5184 the generic one, the bias-table gradient sums
10^4 .. 10^5 terms per entry, and the score tensors pass 2^31 elements.

References are the oracle (oracle/segtran_oracle.py) run in fp64 on the device.  Bars are those of the toy-size tests: Y 2e-5 and dX 1e-4 of the
tensor's scale, parameter gradients 3e-4 of the largest gradient (test_modules.check_grads).  A tensor that misses its bar is referred to the
referee of test_gpu_fullshape.py: the same oracle in fp32 on ATen, which the HIP result may be at most REFEREE times as far from fp64 as.
No tensor needed the referee when these tests were written (both engines); SEGX_REFEREE_LOG=<file> logs every comparison."""
import math
import os

import pytest
import torch

from oracle import segtran_oracle as O
from segtran_amd import engine, segx, functional as SF
from segtran_amd.networks import segtran_shared as ss
from segtran_amd.synth import synth_image2d, synth_state_dict
from test_modules import mk_config, load
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
REFEREE = float(os.environ.get('SEGX_REFEREE_FACTOR', '2.25'))          # the factor of test_gpu_model.py / test_gpu_fullshape.py
CFG2, CFG4 = [1792, 1792], [1024, 1024]                                 # first fusion layer: C = 1792, d = 448 (cfg2); C = 1024, d = 256 (cfg4)


def _log(line):
    path = os.environ.get('SEGX_REFEREE_LOG')
    if path:
        with open(path, 'a') as f:
            f.write('%s %s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0], line))


@pytest.fixture(params=['x6', 'f32'])
def tile_engine(request):
    """bf16x6 (the product default) and the fp32 MFMA engine (segx_tune knob 4), as in test_gpu_model.py."""
    L = segx.lib()
    prev = L.set_engine(request.param)
    yield request.param
    L.set_engine(prev)


@pytest.fixture(autouse=True)
def _free_device_memory():
    torch.empty(1, device=DEV)                           # the caching allocator exists before its statistics are reset
    torch.cuda.reset_peak_memory_stats(DEV)
    yield
    _log('peak device memory %.2f GB' % (torch.cuda.max_memory_allocated(DEV) / 2 ** 30))
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) one fusion layer, forward and backward, against the oracle in fp64
# ---------------------------------------------------------------------------------------------------------------------------------------
def _encoder(dims, shape, pos, R, scales, props, clip, drop=0.0):
    cfg = mk_config(dims, 16, pos_dim=len(shape))
    cfg.use_squeezed_transformer = False
    cfg.use_mince_transformer = scales is not None
    cfg.mince_scales, cfg.mince_channel_props = scales, props
    cfg.pos_code_type, cfg.pos_bias_radius, cfg.max_pos_size = pos, R, tuple(shape)
    cfg.attn_clip = clip
    cfg.attention_probs_dropout_prob = drop
    mod = ss.SegtranFusionEncoder(cfg, 'Fusion')
    load(mod, 'voxel_fusion.')                           # synthetic weights, query/key tied (N2) in CrossAttFeatTrans
    mod.to(DEV)
    assert all(m.key.weight is m.query.weight for m in mod.modules() if isinstance(m, ss.CrossAttFeatTrans))
    g = torch.Generator(device='cpu').manual_seed(17)
    with torch.no_grad():                                # trained tables hold O(1) entries (synth gives 0.02): the bias must move the scores
        for k, p in mod.named_parameters():
            if k.endswith('pos_coder.biases'):
                p.copy_(torch.randn(p.shape, generator=g, device='cpu'))
    return mod


def _inputs(B, shape, C, Fo, seed):
    g = _gen(seed)
    N = math.prod(shape)
    X = torch.randn(B, N, C, generator=g, device=DEV)
    coords = torch.stack(torch.meshgrid(*[torch.arange(s, device=DEV) for s in shape], indexing='ij'), -1).reshape(1, N, len(shape))
    pos = (coords.float() * 8).expand(B, N, len(shape)).contiguous()
    vmask = (torch.rand(B, N, 1, generator=g, device=DEV) > 0.1).float()            # ~10% masked tokens (image border)
    G = torch.randn(B, N, Fo, generator=g, device=DEV)
    return X, pos, vmask, G


def _oracle(mod, dims, shape, pos, scales, props, clip, X, posv, vmask, G, dtype):
    """The oracle over the module's own state dict in `dtype` on the device; tied query/key stay ONE tensor (their gradients sum, N2)."""
    sd, seen, first = {}, {}, {}
    for k, v in mod.state_dict().items():
        key = (v.data_ptr(), tuple(v.shape))
        if key not in seen:
            seen[key] = v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v
            first[k] = seen[key]
        sd['voxel_fusion.' + k] = seen[key]
    Xo = X.detach().to(dtype).requires_grad_(True)
    stats = []
    with torch.device(DEV):                              # the oracle builds its index tensors on the default device
        Y = O.fusion_encoder(sd, 'voxel_fusion', Xo, posv.to(dtype), vmask.to(dtype), dims, attn_clip=clip, pos_code_weight=mod.translayers[0].pos_code_weight
                             if pos == 'bias' else 1.0, stats=stats, squeezed=False, pos_code_type=pos, feat_shape=tuple(shape), mince_scales=scales,
                             mince_channel_props=props)
    (Y * G.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in first.items() if v.grad is not None}
    return Y.detach(), Xo.grad, grads, stats


def _check(name, got, ref64, tol, scale, ref32_fn):
    e64 = (got.detach().double() - ref64.double()).abs().max().item() / scale
    if e64 <= tol:
        _log('%s err %.3e of scale (bar %.0e)' % (name, e64, tol))
        return
    r64 = (ref32_fn().double() - ref64.double()).abs().max().item() / scale
    _log('%s REFEREE err %.3e ref32 %.3e ratio %.2f' % (name, e64, r64, e64 / max(r64, 1e-30)))
    assert e64 <= REFEREE * r64, '%s: |hip - fp64| %.2e > %.0e of scale, and %.2f x |fp32 - fp64| (%.2e)' % (name, e64, tol, e64 / max(r64, 1e-30), r64)


LAYER_CASES = {
    'bias2d_64x64': dict(dims=CFG2, shape=(64, 64), pos='bias', R=7),
    'bias2d_64x64_clamped': dict(dims=CFG2, shape=(64, 64), pos='bias', R=7, clamp=True),
    'bias2d_72x72': dict(dims=CFG2, shape=(72, 72), pos='bias', R=7),                                   # 5184 tokens: the generic softmax
    'lsinu2d_64x64_clamped': dict(dims=CFG2, shape=(64, 64), pos='lsinu', clamp=True),                  # no bias: the softmax clamps
    'bias3d_14x14x12': dict(dims=CFG4, shape=(14, 14, 12), pos='bias', R=7),                            # 15^3 = 3375 table entries
    'mince2d_64x64': dict(dims=CFG2, shape=(64, 64), pos='bias', R=7, scales=[4, 2, 1], props=[1, 1, 2]),  # grids 16^2, 32^2, 64^2
    'mince3d_14x14x12': dict(dims=CFG4, shape=(14, 14, 12), pos='bias', R=7, scales=[4, 2, 1], props=[1, 1, 2]),  # 3x3x3, 7x7x6, 14x14x12
}


@pytest.mark.parametrize('case', list(LAYER_CASES))
def test_fusion_layer_at_size_vs_fp64(tile_engine, case):
    """One cfg2 / cfg4 fusion layer (B = 2, product widths, random weights) at the product token count: Y, dX and every parameter gradient --
    the bias tables included -- against the oracle in fp64.  `clamped` lowers attn_clip below the global score maximum (checked on both sides).
    Measured: Y <= 3.5e-6 and dX <= 3.8e-6 of scale on both engines.  The bias table's gradient is also held to 3e-4 of its OWN scale: at
    N >= 2352 on the bf16x6 engine it sits 1.1e-4 .. 2.4e-4 from fp64 (the fp32 engine: <= 2.3e-5), the closest any tensor here comes to a bar."""
    c = LAYER_CASES[case]
    dims, shape, pos, R = c['dims'], c['shape'], c['pos'], c.get('R', 7)
    scales, props = c.get('scales'), c.get('props')
    B = 2
    X, posv, vmask, G = _inputs(B, shape, dims[0], dims[-1], seed=len(case))
    clip = 500.0
    if c.get('clamp'):
        mod = _encoder(dims, shape, pos, R, scales, props, clip)
        with torch.no_grad():
            mod.eval()(X, posv, vmask, torch.Size(shape))
        gm = mod.translayers[0].attn_max_dev
        clip = 0.6 * float(max(t.item() for t in gm) if isinstance(gm, list) else gm.item())
        del mod
    mod = _encoder(dims, shape, pos, R, scales, props, clip).eval()
    Xh = X.clone().requires_grad_(True)
    Y = mod(Xh, posv, vmask, torch.Size(shape))
    (Y * G).sum().backward()
    gm = mod.translayers[0].attn_max_dev
    hip_max = max(t.item() for t in gm) if isinstance(gm, list) else gm.item()
    Y64, dX64, g64, stats = _oracle(mod, dims, shape, pos, scales, props, clip, X, posv, vmask, G, torch.float64)
    if c.get('clamp'):
        assert hip_max > clip and max(stats) > clip, 'the clamp did not fire: max %.3f / %.3f, clip %.3f' % (hip_max, max(stats), clip)
    else:
        assert max(stats) < clip
    assert abs(hip_max - max(stats)) <= 1e-4 * abs(max(stats))
    ref32 = {}

    def r32(key):
        if not ref32:
            ref32['Y'], ref32['dX'], ref32['g'], _ = _oracle(mod, dims, shape, pos, scales, props, clip, X, posv, vmask, G, torch.float32)
        return ref32[key] if key in ('Y', 'dX') else ref32['g'][key]
    _check('Y', Y, Y64, 2e-5, Y64.abs().max().item(), lambda: r32('Y'))
    _check('dX', Xh.grad, dX64, 1e-4, dX64.abs().max().item(), lambda: r32('dX'))
    named = dict(mod.named_parameters())
    assert set(g64) <= set(named) and len(g64) >= 10, sorted(set(g64) - set(named))
    gscale = max(v.abs().max().item() for v in g64.values())
    tables = [k for k in named if k.endswith('pos_coder.biases')]
    assert len(tables) == (0 if pos != 'bias' else len(scales) if scales else 1) and set(tables) <= set(g64)
    for k, p in named.items():
        if k not in g64:                                     # outside the FFN branch's graph (first_norm_layer): no gradient on either side
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        _check(k, p.grad, g64[k], 3e-4, gscale, lambda k=k: r32(k))
    for k in tables:                                         # the table gradient on its OWN scale too (it is far below the largest gradient)
        _check(k + ' (own scale)', named[k].grad, g64[k], 3e-4, g64[k].abs().max().item(), lambda k=k: r32(k))


def test_attention_dropout_at_4096_tokens(monkeypatch):
    """p = 0.2 on [M = 4, B = 2, 4096, 4096] scores (1.3e8 Philox counters per call): the backward regenerates the forward's mask (the construction
    of test_softmax_dropout_consistent_fwd_bwd, here against fp64), and two consecutive attention layers of one forward reserve disjoint counter
    ranges and draw independent masks."""
    p, M, B, N = 0.2, 4, 2, 4096
    g = _gen(5)
    S = (torch.randn(M, B, N, N, generator=g, device=DEV) * 2).requires_grad_(True)
    SF.manual_seed(21)
    SF._Rng.reserve(3 * 10 ** 8)                                                    # start deep in the stream, as a late layer of a step does
    Pd = SF.softmax(S, 500.0, None, p)
    keep = Pd.detach() != 0
    assert abs((1 - keep.float().mean().item()) - p) < 1e-3
    Gd = torch.randn(M, B, N, N, generator=g, device=DEV)
    Pd.backward(Gd)
    S64 = S.detach().double().requires_grad_(True)
    P64 = S64.softmax(-1)
    (P64 * keep / (1 - p)).backward(Gd.double())
    assert_close(Pd.detach(), (P64.detach() * keep / (1 - p)), 2e-6, 'Pd')
    for m in range(M):
        assert_close(S.grad[m], S64.grad[m], 2e-5, 'dS mode %d' % m)
    del S, S64, P64, Pd, Gd, keep

    masks, ranges = [], []
    real_softmax, real_reserve = SF.softmax, SF._Rng.reserve.__func__

    def softmax(S, clip=500.0, gmax=None, drop_p=0.0):
        out = real_softmax(S, clip, gmax, drop_p)
        masks.append((out.detach() != 0).cpu())
        return out

    def reserve(cls, n):
        r = real_reserve(cls, n)
        ranges.append((r[1], r[1] + int(n)))
        return r
    monkeypatch.setattr(SF, 'softmax', softmax)
    monkeypatch.setattr(SF._Rng, 'reserve', classmethod(reserve))
    mod = _encoder([1792, 1792, 896], (64, 64), 'bias', 7, None, None, 500.0, drop=p).train()
    X, posv, vmask, _ = _inputs(1, (64, 64), 1792, 896, seed=6)
    SF.manual_seed(22)
    mod(X, posv, vmask, torch.Size((64, 64))).sum().backward()
    assert len(masks) == 2
    for m in masks:
        assert abs((1 - m.float().mean().item()) - p) < 1e-3
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), ranges
    same = (masks[0] == masks[1]).float().mean().item()
    assert abs(same - (p * p + (1 - p) ** 2)) < 2e-3, same                        # independent masks agree on p^2 + (1-p)^2 of the entries


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the positional-bias and softmax kernels at product sizes, through segx
# ---------------------------------------------------------------------------------------------------------------------------------------
def _entries(shape, R):
    """[N, N] int64: the table entry of every (query, key) pair, -1 outside the radius (the oracle's lookup applied to the entry numbers)."""
    nd = len(shape)
    ids = torch.arange(1, (2 * R + 1) ** nd + 1, dtype=torch.float64, device=DEV).view([2 * R + 1] * nd)
    with torch.device(DEV):
        return (O.sliding_pos_biases(ids, shape) - 1).long()


def _geom(shape, R):
    return (((1,) + tuple(shape)) if len(shape) == 2 else tuple(shape)) + (R, len(shape))


def _check_fwd(out, S, bias64, w, clip, clamped, mats):
    w = torch.tensor(w, dtype=torch.float32).item()                   # the weight the kernel multiplies by
    for z in mats:
        s = S[z].double()
        s = s.clamp(-clip, clip) if clamped else s
        ref = s + w * bias64
        bound = 2.0 ** -23 * (s.abs() + abs(w) * bias64.abs()) + 1e-30      # one fp32 product and one fp32 add
        bad = ((out[z].double() - ref).abs() > bound).sum().item()
        assert bad == 0, 'posbias_fwd: %d wrong elements in score matrix %d' % (bad, z)


def _check_dtable(dtable, dOut, idx, w, nmat):
    """dtable per ENTRY against fp64, each bounded by that entry's sum of |terms| (a global bound would hide one badly summed entry)."""
    inside = idx >= 0
    sel = idx[inside]
    ref = torch.zeros(dtable.numel(), dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(ref)
    for z in range(nmat):
        d = dOut[z].double()[inside]
        ref.index_add_(0, sel, d)
        mag.index_add_(0, sel, d.abs())
    ref, mag = ref * w, mag * abs(w)
    assert (mag > 0).all()
    rel = ((dtable.reshape(-1).double() - ref).abs() / mag)
    _log('dtable worst entry %d: err %.3e of its sum |terms|' % (rel.argmax().item(), rel.max().item()))
    assert rel.max().item() < 1e-6, 'dtable entry %d: error %.3e of its sum |terms|' % (rel.argmax().item(), rel.max().item())


@pytest.mark.parametrize('clamped', [False, True])
@pytest.mark.parametrize('shape,nmat', [((64, 64), 24),            # cfg2 batch 6 x 4 modes: 98 304 terms per table entry
                                        ((14, 14, 12), 16)])       # cfg4 batch 4 x 4 modes, 3-D: 3375 entries, 37 632 terms each
def test_posbias_kernels_at_product_size(shape, nmat, clamped):
    L = segx.lib()
    R, w, clip = 7, 0.7, 4.0
    N = math.prod(shape)
    g = _gen(nmat + len(shape))
    table = torch.randn([2 * R + 1] * len(shape), generator=g, device=DEV)
    S = torch.randn(nmat, N, N, generator=g, device=DEV) * 3
    gmax = S.max().reshape(1) if clamped else torch.ones(1, device=DEV)
    assert (gmax.item() > clip) == clamped
    out = torch.empty_like(S)
    L.posbias_fwd(S, out, table, nmat, N, _geom(shape, R), w, clip, gmax)
    idx = _entries(shape, R)
    bias64 = torch.where(idx >= 0, table.double().reshape(-1)[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=DEV))
    _check_fwd(out, S, bias64, w, clip, clamped, range(nmat))
    dOut = out.normal_(generator=g)
    dS = torch.empty_like(S) if clamped else None
    dtable = torch.full_like(table, float('nan'))
    L.posbias_bwd(dOut, S if clamped else None, dS, dtable, nmat, N, _geom(shape, R), w, clip)
    if clamped:
        assert torch.equal(dS, torch.where(S.abs() <= clip, dOut, torch.zeros((), device=DEV)))
    _check_dtable(dtable, dOut, idx, w, nmat)


def test_row_kernels_past_2e31_elements():
    """[130, 4096, 4096] scores: 2.18e9 elements, 8.7 GB per tensor.  Element 2^31 is the first element of score matrix 128 (row 524 288 of the
    softmax), so int32 index math goes wrong from there on.  posbias_fwd (clamped), posbias_bwd (clamp mask and table) and softmax_fwd; the
    elementwise results checked on matrices 0, 127, 128 and 129, the table gradient on all 130."""
    L = segx.lib()
    shape, R, w, clip = (64, 64), 7, 0.7, 4.0
    N, nmat = 4096, 130
    assert nmat * N * N > 2 ** 31 and (128 * N * N == 2 ** 31)
    mats = (0, 127, 128, 129)
    g = _gen(31)
    table = torch.randn(2 * R + 1, 2 * R + 1, generator=g, device=DEV)
    S = torch.randn(nmat, N, N, generator=g, device=DEV) * 3
    gmax = S.max().reshape(1)
    out = torch.empty_like(S)
    try:
        L.posbias_fwd(S, out, table, nmat, N, _geom(shape, R), w, clip, gmax)
        idx = _entries(shape, R)
        bias64 = torch.where(idx >= 0, table.double().reshape(-1)[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=DEV))
        _check_fwd(out, S, bias64, w, clip, True, mats)
        dOut = out.normal_(generator=g)
        dS = torch.empty_like(S)
        dtable = torch.full_like(table, float('nan'))
        L.posbias_bwd(dOut, S, dS, dtable, nmat, N, _geom(shape, R), w, clip)
        for z in mats:
            assert torch.equal(dS[z], torch.where(S[z].abs() <= clip, dOut[z], torch.zeros((), device=DEV))), z
        _check_dtable(dtable, dOut, idx, w, nmat)
        P = dS                                                                   # reuse the 8.7 GB
        P.fill_(float('nan'))
        L.softmax_fwd(S, P, None, nmat * N, N, clip, gmax, 0.0, 0, 0)
        for z in mats:
            ref = S[z].double().clamp(-clip, clip).softmax(-1)
            rel = ((P[z].double() - ref).abs() / ref).max().item()
            assert rel < 1e-5, 'softmax_fwd: matrix %d relative error %.3e' % (z, rel)
    finally:
        S = out = dOut = dS = P = None                                            # nothing of the 26 GB outlives the test, failed or not
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) the whole 2-D model at the cfg2 shape (512^2 -> 64 x 64 tokens)
# ---------------------------------------------------------------------------------------------------------------------------------------
_MODEL_ORACLE = {}
MODEL_VARIANTS = {
    'nosqueeze_bias': (dict(use_squeezed_transformer=False, pos_code_type='bias', pos_bias_radius=7),
                       dict(squeezed=False, pos_code_type='bias', pos_code_weight=1.0)),
    'mince_bias': (dict(use_squeezed_transformer=False, use_mince_transformer=True, mince_scales=[4, 2, 1], mince_channel_props=[1, 1, 2],
                        pos_code_type='bias', pos_bias_radius=7),
                   dict(squeezed=False, pos_code_type='bias', pos_code_weight=1.0, mince_scales=[4, 2, 1], mince_channel_props=[1, 1, 2])),
}


@pytest.mark.parametrize('variant', list(MODEL_VARIANTS))
def test_segtran2d_512_nosqueeze_vs_oracle(tile_engine, variant):
    """Segtran2d at the cfg2 shape (512^2, batch 1) with --nosqueeze --pos bias --posr 7, and with --mince 4,2,1 / 1,1,2: eval-mode logits
    against the CPU oracle (1e-4 of scale; hardened labels bit-exact where |logit| >= 1e-5), then one train-mode backward: every gradient
    finite, every bias table with a non-zero gradient."""
    over, fusion_kw = MODEL_VARIANTS[variant]
    c = dict(engine.CONFIGS['cfg2'], size=(512, 512))
    net = engine.build_model(c, DEV, dropout_prob=0.0, attractors=32, **over)
    net.eval()
    x = synth_image2d(1, 512, seed=11)
    with torch.no_grad():
        y = net(x.to(DEV)).cpu()
    if variant not in _MODEL_ORACLE:
        sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()})
        with torch.no_grad(), torch.device('cpu'):
            _MODEL_ORACLE[variant] = O.segtran2d_forward(sd, x, [1792, 1792, 896, 448], fusion_kw=fusion_kw)
    yo = _MODEL_ORACLE[variant]
    _log('logits err %.3e of scale' % ((y - yo).abs().max().item() / yo.abs().max().item()))
    assert_close(y, yo, 1e-4, 'logits')
    # Labels bit-exact where |logit| >= 1e-5 on the bf16x6 engine (|hip - fp64| 5.6e-6 absolute, scale 1.8).  The fp32 engine's logits sit
    # 1.8e-5 .. 3.7e-5 from fp64 at 4096 tokens (2e-5 of scale: inside the logits bar, 7x the fp32 CPU oracle's own 2.5e-6), and one mince
    # label at |logit| = 1.0e-5 flipped: there the margin is 1e-4, as in test_segtran3d_vs_reference's train mode.
    safe = yo.abs() >= (1e-5 if tile_engine == 'x6' else 1e-4)
    assert torch.equal((y > 0)[safe], (yo > 0)[safe])
    net.train()
    net.backbone.drop_connect_rate = 0.0
    net(x.to(DEV)).sum().backward()
    named = dict(net.named_parameters())
    for k, p in named.items():
        assert p.grad is None or torch.isfinite(p.grad).all(), k
    tables = [k for k in named if k.endswith('pos_coder.biases')]
    assert len(tables) == (3 if 'mince' in variant else 1)
    for k in tables:
        assert named[k].grad is not None and named[k].grad.abs().max().item() > 0, k
