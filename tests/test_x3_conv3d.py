"""The three-term bf16 product in the forward 3-D convolutions (knob X6_TERMS = 3): conv3d_halo_fwd_x6_kernel<..., 3> and conv3d_fwd_x6_kernel<..., 3>
against an fp64 referee within the derived bound, exactness on bf16-representable operands, counters and the term query, and the weight gradients, which stay
six-term whatever the knob says.  Runs on the fiber emulator here and on the HIP build under -m gpu.

The bound is the one of DESIGN.md 5m / tests/test_x3_precision.py, with nothing measured in it: an element is off the exact convolution by at most
(2 c1 + c2^2 + gamma_K') conv(|x|, |w|), c1 = 2^-16, c2 = 2^-8 (the two round-to-nearest-even steps of split2_pair on an 8-bit significand), gamma_K' =
K' u / (1 - K' u), u = 2^-24, K' = Cin * window + the number of k slabs (the fp32 accumulation over the contraction and the sum of the slabs)."""
import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd import segx
from test_x3_precision import _bf16_exact, _bound, _check_bound, _run, C1, C2, U

HALO_CASES = [(2, 8, 24, (4, 4, 8), 0),            # 64-row tile, rows of 8
              (1, 24, 136, (8, 4, 4), 0),          # 128-row tile, rows of 4, three channel blocks
              (1, 8, 200, (8, 8, 4), 192),         # 192-row tile
              (1, 8, 40, (7, 11, 15), 0)]          # masked edge tiles
IGEMM_CASES = [(2, 8, 12, (4, 6, 5), (3, 3, 3), (1, 1, 1)),        # 64-row tile, ragged positions
               (1, 24, 140, (3, 9, 9), (3, 3, 3), (1, 1, 1)),      # 128-row tile, two M tiles
               (1, 8, 8, (6, 8, 8), (3, 3, 3), (2, 2, 2)),
               (1, 8, 24, (2, 4, 32), (1, 5, 5), (1, 2, 2))]


@pytest.fixture
def L(backend):
    lib = backend.L
    prev = lib.set_engine('x6')
    lib.x6_launches(); lib.x3_launches()
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    yield lib
    lib.set_engine(prev)
    assert lib.c.segx_tune_get(segx.Knob.X6_TERMS) == 6, 'a test left the three-term mode on'


def _rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device='cpu').manual_seed(seed), device='cpu') * scale


def _referee(x, w, stride=(1, 1, 1)):
    """(F.conv3d in fp64 with the layer's 'same' pads, F.conv3d(|x|, |w|) in fp64) on the CPU"""
    pads = SF._same_pads(x.shape[2:], w.shape[2:], stride)
    pad = (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1])
    xd, wd = x.double().cpu(), w.double().cpu()
    return F.conv3d(F.pad(xd, pad), wd, None, stride), F.conv3d(F.pad(xd.abs(), pad), wd.abs(), None, stride)


def _geom(x, w, stride):
    pads = SF._same_pads(x.shape[2:], w.shape[2:], stride)
    out = tuple((n + p[0] + p[1] - k) // s + 1 for n, p, k, s in zip(x.shape[2:], pads, w.shape[2:], stride))
    return (x.shape[1],) + tuple(x.shape[2:]) + out + tuple(w.shape[2:]) + tuple(stride) + tuple(p[0] for p in pads)


def _check(y3, y6, ref, absref, kprime, what):
    bound = (2 * C1 + C2 * C2 + kprime * U / (1 - kprime * U)) * absref
    e3, e6 = (y3.double().cpu() - ref).abs(), (y6.double().cpu() - ref).abs()
    print('%s: max err3 / bound %.3f, max err3 %.3e, max err6 %.3e' % (what, (e3 / bound).max().item(), e3.max().item(), e6.max().item()))
    assert torch.isfinite(y3).all()
    assert (e3 <= bound).all(), '%s: %.3f of the bound' % (what, (e3 / bound).max().item())
    assert (e3 > e6).any(), what + ': no element is further off than the six-term result -- was the mode on?'


def _halo(L, dev, x, w, B, Cin, Cout, size, mtile, terms):
    """the halo kernel on channel-slice operands (x: channels 8.. of a wider tensor, y: channels 3.. of a wider one); returns the whole output tensor"""
    D, H, W = size
    geom = (Cin, D, H, W, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    xw = torch.cat([_rnd((B, 8) + size, 70), x], 1).to(dev)
    y = torch.full((B, Cout + 3, D, H, W), 7.0, device=dev)
    with L.tuned(engine=L.ENGINES['x6'], conv_halo_min_tiles=1, x6_terms=terms):
        assert L.conv3d_halo_ok(B, Cout, geom) and L.conv3d_fwd_terms(B, Cout, geom) == terms
        L.conv3d_halo_fwd(xw[:, 8:], L.conv3d_halo_pack(w.to(dev), Cout, Cin, 0), y[:, 3:], B, Cout, geom, x_bs=(Cin + 8) * D * H * W, y_bs=(Cout + 3) * D * H * W,
                          mtile=mtile)
    assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    return y


@pytest.mark.parametrize('B,Cin,Cout,size,mtile', HALO_CASES)
def test_halo_kernel_in_three_terms_within_the_derived_bound(L, backend, B, Cin, Cout, size, mtile):
    x, w = _rnd((B, Cin) + size, 81), _rnd((Cout, Cin, 3, 3, 3), 82, 0.2)
    y6 = _halo(L, backend.dev, x, w, B, Cin, Cout, size, mtile, 6)
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    y3 = _halo(L, backend.dev, x, w, B, Cin, Cout, size, mtile, 3)
    assert (L.x6_launches(), L.x3_launches()) == (1, 1)
    untouched = torch.full((B, 3) + size, 7.0, device=backend.dev)
    assert torch.equal(y3[:, :3], untouched) and torch.equal(y6[:, :3], untouched)      # nothing written outside the slice
    ref, absref = _referee(x, w)
    _check(y3[:, 3:], y6[:, 3:], ref, absref, Cin * 27 + 1, 'halo %s' % ((B, Cin, Cout, size, mtile),))


def _same(L, dev, x, w, stride, terms):
    """SF.conv3d_same without gradients on the implicit GEMM (halo kernels off); returns (y, k slabs)"""
    B, Cout = x.shape[0], w.shape[0]
    geom = _geom(x, w, stride)
    with L.tuned(engine=L.ENGINES['x6'], conv_halo_min_tiles=1, conv_halo=0, x6_terms=terms):
        sk = L.conv3d_splitk(B, Cout, geom, False)
        assert L.conv3d_route(B, Cout, geom, False, sk)[0] == 'x6'
        assert L.conv3d_fwd_terms(B, Cout, geom, sk) == terms
        with torch.no_grad():
            y = SF.conv3d_same(x.to(dev), w.to(dev), stride)
    assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    return y, sk


@pytest.mark.parametrize('B,Cin,Cout,size,k,stride', IGEMM_CASES)
def test_implicit_gemm_forward_in_three_terms_within_the_derived_bound(L, backend, B, Cin, Cout, size, k, stride):
    x, w = _rnd((B, Cin) + size, 61), _rnd((Cout, Cin) + k, 62, 0.2)
    y6, sk = _same(L, backend.dev, x, w, stride, 6)
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    y3, sk3 = _same(L, backend.dev, x, w, stride, 3)
    assert (L.x6_launches(), L.x3_launches()) == (1, 1) and sk3 == sk
    ref, absref = _referee(x, w, stride)
    assert y3.shape == ref.shape
    _check(y3, y6, ref, absref, Cin * k[0] * k[1] * k[2] + sk, 'implicit GEMM %s' % ((B, Cin, Cout, size, k, stride),))


def _packed_splitk(L, dev, x, w, terms, splitk=2):
    """L.conv3d_fwd_packed with two k slabs in a workspace, on channel-slice operands as the Inception branches call it"""
    B, Cin, Cout, size = x.shape[0], x.shape[1], w.shape[0], tuple(x.shape[2:])
    P = size[0] * size[1] * size[2]
    geom = _geom(x, w, (1, 1, 1))
    xw = torch.cat([_rnd((B, 8) + size, 71), x], 1).to(dev)
    wd = w.to(dev)
    wp = torch.empty_like(wd)
    L.conv3d_pack_weights(wd, wp, Cout, Cin, 27, 0)
    y = torch.full((B, Cout + 4) + size, 7.0, device=dev)
    ws = torch.full((splitk * B * Cout * P,), float('nan'), device=dev)
    with L.tuned(engine=L.ENGINES['x6'], conv_halo_min_tiles=1, conv_halo=0, x6_terms=terms):
        assert L.conv3d_route(B, Cout, geom, False, splitk)[::4] == ('x6', splitk)
        assert L.conv3d_fwd_terms(B, Cout, geom, splitk) == terms
        L.conv3d_fwd_packed(xw[:, 8:], wp, y[:, 4:], B, Cout, geom, splitk, ws, x_bs=(Cin + 8) * P, y_bs=(Cout + 4) * P)
    return y


def test_packed_forward_with_split_k_in_three_terms(L, backend):
    B, Cin, Cout, size = 2, 16, 40, (5, 6, 7)
    x, w = _rnd((B, Cin) + size, 21), _rnd((Cout, Cin, 3, 3, 3), 22, 0.2)
    y6 = _packed_splitk(L, backend.dev, x, w, 6)
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    y3 = _packed_splitk(L, backend.dev, x, w, 3)
    assert (L.x6_launches(), L.x3_launches()) == (1, 1)
    untouched = torch.full((B, 4) + size, 7.0, device=backend.dev)
    assert torch.equal(y3[:, :4], untouched) and torch.equal(y6[:, :4], untouched)
    ref, absref = _referee(x, w)
    _check(y3[:, 4:], y6[:, 4:], ref, absref, Cin * 27 + 2, 'packed, two k slabs')


def test_term_query_follows_engine_and_knob(L, backend):
    geom = (8, 4, 6, 5, 4, 6, 5, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    assert L.conv3d_fwd_terms(2, 12, geom) == 6                            # the default knob, whichever kernel serves the call
    with L.tuned(conv_halo=0):
        assert L.conv3d_fwd_terms(2, 12, geom) == 6
        with L.tuned(x6_terms=3):
            assert L.conv3d_fwd_terms(2, 12, geom) == 3
            assert L.conv3d_fwd_terms(2, 12, geom, packed=False) == 0      # unpacked filters run on the fp32-MFMA kernels
            with L.tuned(engine=L.ENGINES['f32']):
                assert L.conv3d_fwd_terms(2, 12, geom) == 0                # off the bf16 tile engine
    with L.tuned(x6_terms=3):                                            # the nine outputs of the route do not depend on the knob
        r3 = L.conv3d_route(2, 12, geom, False)
    assert r3 == L.conv3d_route(2, 12, geom, False)


# ---- exactness ----------------------------------------------------------------------------------------------------------------------------------------------
def test_bf16_representable_operands_give_the_six_term_bits(L, backend):
    """every operand value is its own hi plane: the three dropped products are zero, so the two kernels add the same numbers in the same order"""
    B, Cin, Cout, size, mtile = HALO_CASES[1]
    x, w = _bf16_exact((B, Cin) + size, 1), _bf16_exact((Cout, Cin, 3, 3, 3), 2)
    h6, h3 = (_halo(L, backend.dev, x, w, B, Cin, Cout, size, mtile, t) for t in (6, 3))
    assert (L.x6_launches(), L.x3_launches()) == (2, 1)
    assert torch.equal(h3, h6) and torch.isfinite(h3).all()
    B, Cin, Cout, size, k, stride = IGEMM_CASES[1]
    x, w = _bf16_exact((B, Cin) + size, 3), _bf16_exact((Cout, Cin) + k, 4)
    (g6, _), (g3, _) = (_same(L, backend.dev, x, w, stride, t) for t in (6, 3))
    assert (L.x6_launches(), L.x3_launches()) == (2, 1)
    assert torch.equal(g3, g6) and torch.isfinite(g3).all()


# ---- the weight gradients stay six-term -------------------------------------------------------------------------------------------------------------------------
def test_halo_weight_gradient_ignores_the_knob(L, backend):
    B, Cin, Cout, size = 2, 8, 40, (4, 4, 8)
    D, H, W = size
    geom = (Cin, D, H, W, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    x, dy = _rnd((B, Cin) + size, 101).to(backend.dev), _rnd((B, Cout) + size, 102).to(backend.dev)
    out = {}
    for terms in (6, 3):
        with L.tuned(engine=L.ENGINES['x6'], conv_halo_min_tiles=1, x6_terms=terms):
            assert L.conv3d_halo_wgrad_ok(B, Cout, geom)
            dw = torch.full((Cout, Cin, 3, 3, 3), 7.0, device=backend.dev)
            L.conv3d_halo_wgrad(dy, x, dw, B, Cout, geom)
            out[terms] = dw
        assert (L.x6_launches(), L.x3_launches()) == (1, 0)
        assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
    assert torch.equal(out[3], out[6]) and torch.isfinite(out[3]).all()


@pytest.mark.parametrize('B,Cin,Cout,size,k', [(1, 8, 16, (2, 3, 16), (1, 3, 3)), (1, 8, 96, (2, 3, 8), (3, 3, 3))])
def test_implicit_gemm_weight_gradient_ignores_the_knob(L, backend, B, Cin, Cout, size, k):
    """SF.conv3d_same(...).backward with gradients enabled and the knob set through the C ABI (inference_precision would refuse): the weight gradient -- on the bf16
    engine's row-of-eight loader at these widths -- runs six-term and gives the bits it gives at 6"""
    x, G = _rnd((B, Cin) + size, 61).to(backend.dev), _rnd((B, Cout) + size, 63).to(backend.dev)
    out = {}
    for terms in (6, 3):
        w = _rnd((Cout, Cin) + k, 62, 0.2).to(backend.dev).requires_grad_(True)
        with L.tuned(engine=L.ENGINES['x6'], conv_halo_min_tiles=1, conv_halo=0, x6_terms=terms), torch.enable_grad():
            y = SF.conv3d_same(x, w, (1, 1, 1))
            assert (L.x6_launches(), L.x3_launches()) == (1, 1 if terms == 3 else 0)       # the forward follows the knob ...
            y.backward(G)
            assert L.x6_launches() >= 1 and L.x3_launches() == 0                           # ... the weight gradient ran on the bf16 engine, six-term
        assert L.c.segx_tune_get(segx.Knob.X6_TERMS) == 6
        out[terms] = w.grad.clone()
    assert torch.equal(out[3], out[6]) and torch.isfinite(out[3]).all()


# ---- the GEMM route the 3-D eval forward added ------------------------------------------------------------------------------------------------------------------
def test_nt_product_on_the_64x128_lean_tile_runs_three_term(L, backend):
    """both operands k-contiguous on the four-wave 64 x 128 tile with the lean loaders (K % 32 == 0): the [2352 x 1024 x 256] x 16 attention product of the cfg4
    forward, the one bf16 GEMM launch of the 3-D eval forwards that ran six-term under the knob.  Two tiles in M, ragged edges, two k-tiles."""
    tile, (M, N, K) = segx.TILE_64x128, (68, 132, 64)
    A, B = _rnd((M, K), 3), _rnd((N, K), 4, 0.3)
    c6 = _run(L, backend.dev, A, B, 6, tile=tile, want=('x6_lean', tile, 6))
    assert (L.x6_launches(), L.x3_launches()) == (1, 0)
    c3 = _run(L, backend.dev, A, B, 3, tile=tile, want=('x6_lean', tile, 3))
    assert (L.x6_launches(), L.x3_launches()) == (1, 1)
    _check_bound(c3, c6, A.double() @ B.double().t(), _bound(A, B, K), 'NT, lean 64 x 128')
    Ae, Be = _bf16_exact((M, K), 5), _bf16_exact((N, K), 6)
    e6, e3 = (_run(L, backend.dev, Ae, Be, t, tile=tile) for t in (6, 3))
    assert L.x3_launches() == 1 and torch.equal(e3, e6) and torch.isfinite(e3).all()
