"""The opt-in three-term bf16 GEMM precision (segx_tune knob X6_TERMS = 3): exactness on bf16-representable operands, the derived error bound
against an fp64 referee, range, routing and counters, and the Python interface.  Runs on the fiber emulator here and on the HIP build under -m gpu.

The bound.  split2_pair / split3_pair round to nearest even at both steps: hi = bf16(x), a = x - hi (exact), mid = bf16(a), r = a - mid.  bf16 carries 8
significand bits, so |a| <= 2^-8 |x| (x = 1 + 2^-8 rounds to 1 and reaches it), |mid| <= 2^-8 |x| =: c2 |x| and |r| <= 2^-8 |a| <= 2^-16 |x| =: c1 |x|.  The three
products that are kept sum to (a - r_a)(b - r_b) - mid_a mid_b, so an element is off the exact inner product by at most (2 c1 + c2^2) (|A|.|B|) -- the c1^2 term is
below fp32 resolution and rides in the accumulation term -- plus gamma_K (|A|.|B|), gamma_K = K u / (1 - K u), u = 2^-24: the fp32 accumulation the six-term
kernel has as well.  (Round-to-nearest on an 8-bit significand gives 2^-8 and 2^-16; 2^-9 / 2^-17 would hold for nine bits.)  Nothing here is measured."""
import pytest
import torch

from segtran_amd import infer2d, segx

C1, C2, U = 2.0 ** -16, 2.0 ** -8, 2.0 ** -24
FOURWAVE = [segx.TILE_128x128, segx.TILE_64x128, segx.TILE_64x64]
WS = [segx.TILE_256x128, segx.TILE_WS128x128]
# the few-channel wave-specialised tiles the planner's table picks for some product shapes, with the B layouts their three-term kernels are built for
WS_FEW = [(segx.TILE_WS128x256, True), (segx.TILE_WS128x256, False), (segx.TILE_WS64x256, False), (segx.TILE_WS96x256, True), (segx.TILE_WS96x256, False),
          (segx.TILE_WS256x96, True)]
# the smallest M x N that puts more than one workgroup tile in M (and leaves ragged edges in M and N) on each kernel; both sides > 48 rows (the engine's floor)
SHAPE = {segx.TILE_128x128: (132, 68), segx.TILE_64x128: (68, 132), segx.TILE_64x64: (68, 52), segx.TILE_256x128: (260, 68), segx.TILE_WS128x128: (132, 68),
         segx.TILE_WS128x256: (132, 260), segx.TILE_WS64x256: (68, 260), segx.TILE_WS96x256: (100, 260), segx.TILE_WS256x96: (260, 100)}


@pytest.fixture
def L(backend):
    lib = backend.L
    prev = lib.set_engine('x6')
    lib.x6_launches(); lib.x3_launches()
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    yield lib
    lib.set_engine(prev)
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6, 'a test left the three-term mode on'


def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def _bf16_exact(shape, seed):
    """values with 8 significant bits, random signs and exponents: every one is its own hi plane, mid and lo are zero"""
    g = _gen(seed)
    mant = torch.randint(128, 256, shape, generator=g, device='cpu').float()
    expo = torch.randint(-12, 5, shape, generator=g, device='cpu').float()
    sign = torch.randint(0, 2, shape, generator=g, device='cpu').float() * 2 - 1
    v = sign * mant * torch.exp2(expo)
    assert torch.equal(v.bfloat16().float(), v)
    return v


def _run(L, dev, A, B, terms, akc=True, bkc=True, tile=segx.TILE_AUTO, want=None, **kw):
    """C[m][n] = sum_k A[m][k] B[n][k] for A [M, K], B [N, K] (cpu tensors) in the given layouts at the given term count; want = the route to assert
    (family, tile, terms)"""
    (M, K), N = A.shape, B.shape[0]
    Am = (A if akc else A.t().contiguous()).to(dev)
    Bm = (B if bkc else B.t().contiguous()).to(dev)
    a_str = (0, 0, K, 1) if akc else (0, 0, 1, M)
    b_str = (0, 0, K, 1) if bkc else (0, 0, 1, N)
    C = torch.full((M, N), float('nan'), device=dev)
    with L.tuned(x6_terms=terms):
        if want is not None:
            got = L.gemm_route(Am, Bm, M, N, K, a_str, b_str, tile=tile, epilogue=kw.get('epilogue', segx.EPI_NONE))
            assert got[:3] == want, (got, want)
        L.gemm(Am, Bm, C, M, N, K, a_str, b_str, (0, 0, N), tile=tile, **kw)
    return C.cpu()


def _family(tile, K):
    return 'ws' if tile in WS or tile in [t for t, _ in WS_FEW] else ('x6_lean' if K % 32 == 0 else 'x6')


def _bound(A, B, K):
    absab = A.double().abs() @ B.double().abs().t()
    return (2 * C1 + C2 * C2) * absab + (K * U / (1 - K * U)) * absab


# ---- exactness --------------------------------------------------------------------------------------------------------------------------------------------
# K = 40 leaves a K tail on the four-wave kernels (dense loaders; their three-term forms are the pointwise-convolution layout: B row-contiguous); the
# wave-specialised kernels take whole 32-k stages only (gemm_ws_ok: any other K routes to the four-wave default tile), so their smallest K with more than one
# stage, 64, stands in -- and runs the lean four-wave forms as well, in every layout that has a three-term kernel
@pytest.mark.parametrize('tile,K,akc,bkc', [(t, 40, True, False) for t in FOURWAVE] + [(t, 64, True, b) for t in FOURWAVE[:1] + WS for b in (True, False)] +
                         [(segx.TILE_128x128, 64, False, True), (segx.TILE_64x64, 64, False, True), (segx.TILE_64x64, 64, True, True), (segx.TILE_64x128, 64, False, True)] +
                         [(t, 64, True, b) for t, b in WS_FEW])
def test_bf16_representable_operands_give_the_six_term_bits(L, backend, tile, K, akc, bkc):
    M, N = SHAPE[tile]
    A, B = _bf16_exact((M, K), 1), _bf16_exact((N, K), 2)
    fam = _family(tile, K)
    c6 = _run(L, backend.dev, A, B, 6, akc=akc, bkc=bkc, tile=tile, want=(fam, tile, 6))
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    c3 = _run(L, backend.dev, A, B, 3, akc=akc, bkc=bkc, tile=tile, want=(fam, tile, 3))
    assert (L.x6_launches(), L.x3_launches()) == (1, 1)
    assert torch.equal(c3, c6) and torch.isfinite(c3).all()
    assert ((c3.double() - A.double() @ B.double().t()).abs() <= (K * U / (1 - K * U)) * (A.double().abs() @ B.double().abs().t())).all()


# ---- bound ------------------------------------------------------------------------------------------------------------------------------------------------
def _check_bound(c3, c6, ref, bound, what):
    e3, e6 = (c3.double() - ref).abs(), (c6.double() - ref).abs()
    print('%s: max err3 / bound %.3f, max err3 %.3e, max err6 %.3e' % (what, (e3 / bound).max().item(), e3.max().item(), e6.max().item()))
    assert torch.isfinite(c3).all()
    assert (e3 <= bound).all(), '%s: %.3e of the bound' % (what, (e3 / bound).max().item())
    assert (e3 > e6).any(), what + ': no element is further off than the six-term product -- was the mode on?'


# the wave-specialised kernels take K % 32 == 0 only: 32, 64 and 288 stand in for 16, 40 and 272 there
@pytest.mark.parametrize('tile,K', [(t, k) for t in FOURWAVE for k in (16, 40, 272)] + [(t, k) for t in WS for k in (32, 64, 288)] + [(segx.TILE_128x128, 64)] +
                         [(t, 64) for t in (segx.TILE_WS128x256, segx.TILE_WS64x256, segx.TILE_WS96x256, segx.TILE_WS256x96)])
def test_random_operands_stay_within_the_derived_bound(L, backend, tile, K):
    M, N = SHAPE[tile]
    A, B = torch.randn(M, K, generator=_gen(3), device='cpu'), torch.randn(N, K, generator=_gen(4), device='cpu') * 0.3
    fam = _family(tile, K)
    bkc = fam != 'x6' and tile != segx.TILE_WS64x256        # the dense loaders' three-term forms, and the 64 x 256 tile's, take a row-contiguous B
    c6 = _run(L, backend.dev, A, B, 6, bkc=bkc, tile=tile, want=(fam, tile, 6))
    c3 = _run(L, backend.dev, A, B, 3, bkc=bkc, tile=tile, want=(fam, tile, 3))
    assert L.x3_launches() == 1
    _check_bound(c3, c6, A.double() @ B.double().t(), _bound(A, B, K), 'tile %d K %d' % (tile, K))


def test_batched_strided_attention_product_within_the_bound(L, backend):
    """Q . K^T over (batch 2, heads 4) with the heads interleaved in memory: [B, L, H, d] operands addressed through their strides"""
    Bn, H, Ln, d = 2, 4, 72, 64
    Q, Kt = torch.randn(Bn, Ln, H, d, generator=_gen(5), device='cpu'), torch.randn(Bn, Ln, H, d, generator=_gen(6), device='cpu')
    strides = (Ln * H * d, d, H * d, 1)
    out = []
    for terms in (6, 3):
        C = torch.full((Bn, H, Ln, Ln), float('nan'), device=backend.dev)
        with L.tuned(x6_terms=terms):
            L.gemm(Q.to(backend.dev), Kt.to(backend.dev), C, Ln, Ln, d, strides, strides, (H * Ln * Ln, Ln * Ln, Ln), nb=(Bn, H), alpha=0.25, tile=segx.TILE_64x64)
        out.append(C.cpu())
    assert (L.x6_launches(), L.x3_launches()) == (2, 1)
    ref = 0.25 * torch.einsum('blhd,bmhd->bhlm', Q.double(), Kt.double())
    absab = 0.25 * torch.einsum('blhd,bmhd->bhlm', Q.double().abs(), Kt.double().abs())
    bound = (2 * C1 + C2 * C2 + d * U / (1 - d * U) + 2 * U) * absab              # + the rounding of alpha * acc
    _check_bound(out[1], out[0], ref, bound, 'attention nb=(2, 4)')


@pytest.mark.parametrize('epi', ['bias', 'swish', 'gelu'])
def test_epilogues_within_the_bound(L, backend, epi):
    """bias, the fused swish (a folded pointwise convolution: weights k-contiguous, activations row-contiguous) and the fused GELU (nn.Linear), no dropout.
    The activation is applied to the biased sum t in fp32: |f(t3) - f(t)| <= Lip(f) |t3 - t| with Lip(swish) < 1.1 and Lip(GELU) < 1.13, plus the fp32 evaluation
    of f itself (fast exponential / erf: a few units in the last place), taken as 16 u (|t| + |f(t)|)."""
    M, N, K = (100, 64, 64) if epi == 'gelu' else (72, 68, 40)
    A, B = torch.randn(M, K, generator=_gen(7), device='cpu'), torch.randn(N, K, generator=_gen(8), device='cpu') * 0.3
    dev = backend.dev
    t64 = A.double() @ B.double().t()
    bound = _bound(A, B, K)
    if epi == 'gelu':
        bias = torch.randn(N, generator=_gen(9), device='cpu')
        kw = dict(bias=bias.to(dev), bias_mode=segx.BIAS_N, epilogue=segx.EPI_GELU)
        t64 = t64 + bias.double()[None, :]
        ref, lip, bkc = torch.nn.functional.gelu(t64), 1.13, True
    else:
        bias = torch.randn(M, generator=_gen(9), device='cpu')
        kw = dict(bias=bias.to(dev), bias_mode=segx.BIAS_M)
        t64 = t64 + bias.double()[:, None]
        ref, lip, bkc = t64, 1.0, False
        if epi == 'swish':
            kw['epilogue'] = segx.EPI_SWISH
            ref, lip, bkc = t64 * torch.sigmoid(t64), 1.1, False
    bound = lip * (bound + 2 * U * t64.abs()) + 16 * U * (t64.abs() + ref.abs())
    out = []
    for terms in (6, 3):
        if epi == 'gelu':
            kw['aux'] = torch.zeros(M, N, device=dev)
        out.append(_run(L, dev, A, B, terms, bkc=bkc, **kw))
    assert (L.x6_launches(), L.x3_launches()) == (2, 1)
    _check_bound(out[1], out[0], ref, bound, epi)


# ---- range ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', [segx.TILE_128x128, segx.TILE_WS128x128])
def test_wide_ranging_operands_stay_finite_and_within_the_bound(L, backend, tile):
    """bf16 planes carry fp32's exponent: operands 60 orders of magnitude apart need no scales (what the removed fp16 split lacked).  The rows of A^T (A's
    entries along k) are scaled by 1e-30, 1 and 1e30 in turn and those of B^T inversely, so every product stays O(1) and finite."""
    (M, N), K = SHAPE[tile], 96
    tk = torch.tensor([1e-30, 1.0, 1e30], device='cpu').repeat(K // 3)
    A = torch.randn(M, K, generator=_gen(10), device='cpu') * tk[None, :]
    B = torch.randn(N, K, generator=_gen(11), device='cpu') / tk[None, :]
    assert torch.isfinite(A).all() and torch.isfinite(B).all() and A.abs().max() > 1e30 and B.abs().max() > 1e30 and A.abs().min() < 1e-30
    c6 = _run(L, backend.dev, A, B, 6, tile=tile)
    c3 = _run(L, backend.dev, A, B, 3, tile=tile, want=(_family(tile, K), tile, 3))
    assert L.x3_launches() == 1
    _check_bound(c3, c6, A.double() @ B.double().t(), _bound(A, B, K), 'range, tile %d' % tile)


# ---- routing and counters ------------------------------------------------------------------------------------------------------------------------------------
def test_routing_counters_and_the_knob(L, backend):
    dev = backend.dev
    A, B = torch.randn(132, 64, generator=_gen(12), device='cpu'), torch.randn(68, 64, generator=_gen(13), device='cpu')
    # knob at 6: nothing counts as three-term
    c6 = _run(L, dev, A, B, 6, tile=segx.TILE_128x128)
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    # knob at 3, a routed shape: one launch, one three-term launch
    c3 = _run(L, dev, A, B, 3, tile=segx.TILE_128x128, want=('x6_lean', segx.TILE_128x128, 3))
    assert (L.x6_launches(), L.x3_launches()) == (1, 1) and not torch.equal(c3, c6)
    # a route without a three-term kernel (both operands row-contiguous: a gradient layout) runs six-term, says so, and gives the six-term bits
    t3 = _run(L, dev, A, B, 3, akc=False, bkc=False, want=('x6_lean', segx.TILE_128x128, 6), tile=segx.TILE_128x128)
    t6b = _run(L, dev, A, B, 6, akc=False, bkc=False, tile=segx.TILE_128x128)
    assert (L.x6_launches(), L.x3_launches()) == (2, 0)
    assert torch.equal(t3, t6b) and torch.isfinite(t3).all()
    # off the bf16 tile engine the knob means nothing
    with L.tuned(x6_terms=3):
        Af, Bf = A.to(dev), B.to(dev)
        route = L.gemm_route(Af, Bf, 132, 68, 64, (0, 0, 64, 1), (0, 0, 64, 1), engine='f32')
        assert (route[0], route[2]) == ('f32', 0)
    # only 6 and 3 are settings
    for bad in (4, 5, 0, 2, 7):
        assert L.c.segx_tune(segx.Knob.X6_TERMS, bad) == -1
        with pytest.raises(ValueError):
            L.tune(segx.Knob.X6_TERMS, bad)
    assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    with L.tuned(x6_terms=3):
        assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 3
    assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6


def test_the_precision_selector_has_one_id_in_header_binding_and_library(L):
    """SEGX_KNOB_X6_TERMS is a #define beside the enum of tuning knobs (a precision selector, not a knob with identical results) and Knob.X6_TERMS an attribute beside
    the enumeration's members: header, binding and the library's knob table name the same id"""
    import os, re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'segx.h')).read()
    ids = re.findall(r'^#define\s+SEGX_KNOB_X6_TERMS\s+(\d+)\s*$', hdr, flags=re.M)
    assert ids == ['20'] and segx.Knob.X6_TERMS == 20 and segx.knob_id('x6_terms') == 20
    assert 20 not in [int(k) for k in segx.Knob] and L.c.segx_tune_get(20) == 6
    assert L.c.segx_tune_get(21) == -1 and L.c.segx_tune(21, 3) == -1
    with pytest.raises(KeyError):
        with L.tuned(x7_terms=3):
            pass


# ---- interface ----------------------------------------------------------------------------------------------------------------------------------------------
def test_inference_precision_context_manager(L):
    import segtran_amd
    get = lambda: L.c.segx_tune_get(segx.Knob.X6_TERMS)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match='inference'):
            with segtran_amd.inference_precision('bf16x3'):
                pass
    assert get() == 6
    with torch.no_grad():
        with pytest.raises(ValueError):
            with segtran_amd.inference_precision('fp16x3'):
                pass
        with segtran_amd.inference_precision('bf16x3'):
            assert get() == 3
            with infer2d.inference_precision('fp32'):
                assert get() == 6
            assert get() == 3
        assert get() == 6
        with pytest.raises(KeyError):
            with segtran_amd.inference_precision('bf16x3'):
                assert get() == 3
                raise KeyError('boom')
        assert get() == 6
    with pytest.raises(ValueError):
        infer2d.test_single_batch(None, torch.zeros(1, 3, 8, 8), (8, 8), (8, 8), (4, 4), 'fundus', 3, precision='tf32')
