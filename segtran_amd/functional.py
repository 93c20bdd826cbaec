"""Autograd surface over libsegx (include/segx.h): every op here runs hand-written HIP kernels forward AND
backward -- there is no PyTorch-eager fallback.  Tensors are fp32 and live on the GPU (or on the CPU only
when a test has installed the fiber-emulated build of the same kernels through `segx.use_library`).
"""
import math
import torch
import torch.nn.functional as F
from . import segx
from .segx import EPI_NONE, EPI_GELU, EPI_SWISH, EPI_RELU, BIAS_NONE, BIAS_N, BIAS_M

LN_EPS = 1e-12      # every LayerNorm of the Squeeze-and-Expansion transformer (segtran_shared.py:262,361,889,985)


# -------------------------------------------------------------------------------------------------
# _Fn: base of every op of this file.  Outside a functorch transform, torch.autograd.Function.apply binds default arguments (only for a class with a
# setup_context: no op here has one), unwraps tensors left over from a finished functorch transform (this library never receives one) and calls
# _FunctionBase.apply.  _Fn.apply calls _FunctionBase.apply directly (4 us less per op) where that is exactly what Function.apply would do:
#   _fast_apply   checked once, at import: _FunctionBase follows Function in torch's (private) class order and no class between them defines `apply`,
#                 so super(Function, cls).apply is _FunctionBase.apply.  Otherwise every op goes through Function.apply.
#   functorch     under vmap / grad / ... Function.apply takes another route (for these ops: torch's setup_context error) -- one C call per op checks
#                 for it, so the kernels never run on a transform's wrapper tensors.
# -------------------------------------------------------------------------------------------------
_MRO = torch.autograd.Function.__mro__
_fast_apply = torch._C._FunctionBase in _MRO and not any('apply' in c.__dict__ for c in _MRO[1:_MRO.index(torch._C._FunctionBase)])


class _Fn(torch.autograd.Function):
    """Base of every op of this file: torch.autograd.Function with the fast path of apply above."""

    @classmethod
    def apply(cls, *args):
        if _fast_apply and not torch._C._are_functorch_transforms_active():
            return super(torch.autograd.Function, cls).apply(*args)
        return super().apply(*args)


def _live(t):
    """does a gradient flow back through t?"""
    return t.requires_grad and torch.is_grad_enabled()


# -------------------------------------------------------------------------------------------------
# Dropout RNG: one Philox stream per process; ops reserve disjoint counter ranges (multiples of 4).
# -------------------------------------------------------------------------------------------------
class _Rng:
    seed = 0x5E67AD
    offset = 0

    @classmethod
    def manual_seed(cls, s):
        cls.seed, cls.offset = int(s) & 0x7FFFFFFFFFFFFFFF, 0

    @classmethod
    def reserve(cls, n):
        o = cls.offset
        cls.offset += (int(n) + 3) // 4 * 4
        return cls.seed, o


manual_seed = _Rng.manual_seed


def _empty(ref, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=ref.device)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# -------------------------------------------------------------------------------------------------
# Generic batched strided GEMM with autograd
# -------------------------------------------------------------------------------------------------
class GemmSpec:
    """C[z0,z1][m][n] = alpha * sum_k A(z,m,k) B(z,n,k) (+bias); strides in elements (see segx.h)."""
    __slots__ = ('M', 'N', 'K', 'nb', 'a', 'b', 'c', 'out_shape', 'alpha', 'bias_mode', 'bias_b1', 'bias_b0')

    def __init__(self, M, N, K, a, b, c, out_shape, nb=(1, 1), alpha=1.0, bias_mode=BIAS_NONE, bias_b1=0, bias_b0=0):
        self.M, self.N, self.K, self.nb, self.a, self.b, self.c = M, N, K, nb, tuple(a), tuple(b), tuple(c)
        self.out_shape, self.alpha, self.bias_mode, self.bias_b1, self.bias_b0 = tuple(out_shape), alpha, bias_mode, bias_b1, bias_b0


def _run_gemm(L, A, B, C, M, N, K, a, b, c, nb, alpha, **kw):
    # splitk=0: the library plans tile shape + split-K (segx_gemm_plan); fused epilogues / gmax never split
    L.gemm(A, B, C, M, N, K, a, b, c, nb=nb, alpha=alpha, splitk=0, **kw)


def _grad_operand(L, dC, other, s, which, like, resid=None):
    """Gradient of operand `which` ('a' or 'b') of spec s.  `other` is the other operand.  resid (same shape as `like`, operand not shared over
    a batch dim): added to the gradient inside the GEMM launch (segx_gemm_desc.resid)."""
    nb = s.nb
    if which == 'a':
        rows, cols, st, ost = s.M, s.K, s.a, s.b      # dA(m,k) = alpha sum_n dC(m,n) B(n,k)
    else:
        rows, cols, st, ost = s.N, s.K, s.b, s.a      # dB(n,k) = alpha sum_m dC(m,n) A(m,k)
    inner = s.N if which == 'a' else s.M
    bcast = [(st[i] == 0 and nb[i] > 1) for i in (0, 1)]
    assert resid is None or (not any(bcast) and like.is_contiguous() and resid.is_contiguous() and resid.shape == like.shape)
    partial = any(bcast) and not all(bcast[i] or nb[i] == 1 for i in (0, 1))
    if (partial and which == 'a' and bcast == [False, True] and st[3] == 1 and like.is_contiguous() and resid is None
            and s.c[1] == s.N and s.c[2] >= nb[1] * s.N and ost[1] == s.N * ost[2] and (ost[2] == 1 or ost[3] == 1)):
        # A is shared by the INNER batch dim (the modes) and both dC and B interleave that dim with the contraction index n -- dC rows are [nb1 * N] long, B's
        # (z1, n) walk is one stride -- so the sum over the modes is part of ONE contraction of depth nb1 * N per outer member:
        #   dA[z0](m, k) = alpha sum_{(z1, n)} dC[z0](m, (z1, n)) B[z0]((z1, n), k)
        # instead of nb1 short-K products written as slabs and summed by a further pass (r06: squeeze-out scores GEMM, 4 x K = 256 -> K = 1024; 0.7 GB of slabs gone)
        out = torch.empty_like(like)
        _run_gemm(L, dC, other, out, rows, cols, nb[1] * s.N, (s.c[0], 0, s.c[2], 1), (ost[0], 0, ost[3], ost[2]), (st[0], 0, st[2]), (nb[0], 1), s.alpha)
        return out
    if partial:
        # shared across ONE batch dim while the other one walks it (attractors shared by the batch, split into modes: Polyformer's
        # in-squeeze): one slab in the operand's own layout per broadcast index, then a deterministic sum over the slabs
        bd = 0 if bcast[0] else 1
        assert like.is_contiguous() and (st[2] == 1 or st[3] == 1)
        k_contig = st[3] == 1
        n = like.numel()
        tmp = torch.zeros(nb[bd], n, dtype=torch.float32, device=dC.device) if n != rows * cols * nb[1 - bd] else _empty(dC, nb[bd], n)
        tgt_b = (n, st[1]) if bd == 0 else (st[0], n)
        row_stride = st[2] if k_contig else st[3]
        dc_as_rows = (s.c[0], s.c[1], s.c[2], 1) if which == 'a' else (s.c[0], s.c[1], 1, s.c[2])
        oth = (ost[0], ost[1], ost[3], ost[2])
        if k_contig:
            _run_gemm(L, dC, other, tmp, rows, cols, inner, dc_as_rows, oth, (tgt_b[0], tgt_b[1], row_stride), nb, s.alpha)
        else:
            _run_gemm(L, other, dC, tmp, cols, rows, inner, oth, dc_as_rows, (tgt_b[0], tgt_b[1], row_stride), nb, s.alpha)
        out = torch.empty_like(like)
        L.colsum(tmp, out, _empty(dC, L.colreduce_ws(nb[bd], n, 1)), nb[bd], n)
        return out
    if any(bcast) and like.is_contiguous() and like.numel() == rows * cols and (st[2] == 1 or st[3] == 1):
        # operand shared by the WHOLE batch (convolution / projection weights): the per-member products are slabs of one deterministic
        # reduction inside the GEMM call (batch_reduce) -- no [batch, rows, cols] temporary, no separate column-sum launches
        k_contig = st[3] == 1
        out = torch.empty_like(like)
        dc_as_rows = (s.c[0], s.c[1], s.c[2], 1) if which == 'a' else (s.c[0], s.c[1], 1, s.c[2])
        oth = (ost[0], ost[1], ost[3], ost[2])
        if k_contig:
            _run_gemm(L, dC, other, out, rows, cols, inner, dc_as_rows, oth, (0, 0, cols), nb, s.alpha, batch_reduce=True)
        else:
            _run_gemm(L, other, dC, out, cols, rows, inner, oth, dc_as_rows, (0, 0, rows), nb, s.alpha, batch_reduce=True)
        return out
    if any(bcast):
        # operand shared across a batch dim: per-batch partial grads, then a deterministic column sum
        assert st[2] == 1 or st[3] == 1
        k_contig = st[3] == 1
        tmp_rows, tmp_cols = (rows, cols) if k_contig else (cols, rows)
        tmp = _empty(dC, nb[0] * nb[1], tmp_rows, tmp_cols)
        tb = (nb[1] * tmp_rows * tmp_cols, tmp_rows * tmp_cols)
        out_rs = tmp_cols
        tgt, tgt_b, row_stride = tmp, tb, out_rs
    else:
        k_contig = st[3] == 1
        tgt = torch.zeros_like(like) if not like.is_contiguous() else torch.empty_like(like)
        tgt_b, row_stride = (st[0], st[1]), (st[2] if k_contig else st[3])
    # dC viewed as an operand: rows m (stride c_m) and cols n (stride 1)
    if which == 'a':
        dc_as_rows = (s.c[0], s.c[1], s.c[2], 1)       # (m, inner=n)
        oth = (ost[0], ost[1], ost[3], ost[2])         # B as (k, inner=n): row stride b_k, inner stride b_n
    else:
        dc_as_rows = (s.c[0], s.c[1], 1, s.c[2])       # (n, inner=m)
        oth = (ost[0], ost[1], ost[3], ost[2])         # A as (k, inner=m): row stride a_k, inner stride a_m
    kw = dict(resid=resid) if resid is not None else {}
    if k_contig:    # out[rows][cols=k]
        _run_gemm(L, dC, other, tgt, rows, cols, inner, dc_as_rows, oth, (tgt_b[0], tgt_b[1], row_stride), nb, s.alpha, **kw)
    else:           # out^T[k][rows]
        _run_gemm(L, other, dC, tgt, cols, rows, inner, oth, dc_as_rows, (tgt_b[0], tgt_b[1], row_stride), nb, s.alpha, **kw)
    if any(bcast):
        assert all(bcast[i] or nb[i] == 1 for i in (0, 1)), 'partial batch broadcast is not supported'
        nbt = nb[0] * nb[1]
        out = torch.empty_like(like)
        assert like.is_contiguous() and like.numel() == tmp_rows * tmp_cols
        ws = _empty(dC, L.colreduce_ws(nbt, tmp_rows * tmp_cols, 1))
        L.colsum(tmp, out, ws, nbt, tmp_rows * tmp_cols)
        return out
    return tgt


class _BGemm(_Fn):
    """pass_b: also return the B operand as a second output (an alias).  A caller that needs B twice -- the input of an MBConv block feeds the
    expansion convolution AND the skip connection -- uses the alias for the second consumer: autograd then hands BOTH gradients to this node,
    and the second one is added inside the dB GEMM (segx_gemm_desc.resid) instead of by a separate accumulation kernel."""
    gelu_bias_fused = True    # GELU epilogue: the bias gradient from the pass that writes dT (segx_gelu_bwd_colsum); False: gelu_bwd + a column-sum pass (tools/ab_switch.py)

    @staticmethod
    def forward(ctx, A, B, bias, spec, gmax, gelu, drop_p, pass_b=False):
        L = segx.lib()
        s = spec
        A, B = _c(A), _c(B)
        C = _empty(A, *s.out_shape)
        kw = dict(bias=bias, bias_mode=s.bias_mode if bias is not None else BIAS_NONE, bias_b1=s.bias_b1, bias_b0=s.bias_b0, gmax=gmax)
        T = None
        seed = off = 0
        if gelu:
            T = torch.empty_like(C)
            if drop_p > 0:
                seed, off = _Rng.reserve(C.numel())
            kw.update(epilogue=EPI_GELU, aux=T, dropout_p=drop_p, seed=seed, offset=off)
        _run_gemm(L, A, B, C, s.M, s.N, s.K, s.a, s.b, s.c, s.nb, s.alpha, **kw)
        ctx.spec, ctx.gelu, ctx.drop = s, gelu, (drop_p, seed, off)
        ctx.has_bias = bias is not None
        ctx.pass_b = pass_b
        ctx.set_materialize_grads(False)                      # an unused output's gradient arrives as None, not as a zero tensor
        ctx.save_for_backward(A, B, T)
        if pass_b:
            return C, B.view_as(B)
        return C

    @staticmethod
    def backward(ctx, dC, dB_alias=None):
        L = segx.lib()
        A, B, T = ctx.saved_tensors
        s = ctx.spec
        if dC is None:                                       # only the alias was used
            return None, dB_alias, None, None, None, None, None, None
        dC = _c(dC)
        dbias = None
        if ctx.gelu:
            p, seed, off = ctx.drop
            dT = torch.empty_like(dC)
            if (ctx.has_bias and ctx.needs_input_grad[2] and s.bias_mode == BIAS_N and s.bias_b0 == 0 and (s.nb[1] == 1 or s.bias_b1 == 0) and s.c[2] == s.N
                    and s.N % 4 == 0 and s.N <= 2048 and _BGemm.gelu_bias_fused and off % 4 == 0 and dC.data_ptr() % 16 == 0 and T.data_ptr() % 16 == 0):
                # the bias gradient (column sums of dT over every row of every batch member) from the pass that writes dT (r06: it was a pass of its own over dT)
                rows = dC.numel() // s.N
                dbias = _empty(dC, s.N)
                L.gelu_bwd_colsum(dC, T, dT, dbias, _empty(dC, L.gelu_bwd_colsum_ws(rows, s.N)), rows, s.N, p, seed, off)
            else:
                L.gelu_bwd(dC, T, dT, dC.numel(), p, seed, off)
            dC = dT
        dA = _grad_operand(L, dC, B, s, 'a', A) if ctx.needs_input_grad[0] else None
        dB = _grad_operand(L, dC, A, s, 'b', B, resid=_c(dB_alias) if dB_alias is not None else None) if ctx.needs_input_grad[1] else None
        if dbias is None and ctx.has_bias and ctx.needs_input_grad[2]:
            dbias = _bias_grad(L, dC, s)
        return dA, dB, dbias, None, None, None, None, None


def _tag_plane_sums(dbase, rsum, B, C, S):
    """_UpGN* hand the lateral convolution's bias gradient (the sums over every (sample, channel) plane of `dbase`) along with `dbase` itself.  The tag is bound
    to the tensor's CONTENTS and LAYOUT -- version counter, storage address, (B, C, S) -- so that a hook / scaling / clipping that touches the gradient in place,
    or a consumer with another plane layout, makes `_take_plane_sums` ignore it (the bare attribute was trusted on numel and device alone)."""
    dbase._segx_plane_sums = (rsum, dbase._version, dbase.data_ptr(), (int(B), int(C), int(S)))


def _take_plane_sums(dC, nbt, M, N):
    tag = getattr(dC, '_segx_plane_sums', None)
    if tag is None:
        return None
    del dC._segx_plane_sums                            # one consumer: a second BIAS_M GEMM reached by the same tensor object computes its own row sums
    rs, version, ptr, bcs = tag
    if version != dC._version or ptr != dC.data_ptr() or bcs != (int(nbt), int(M), int(N)) or not dC.is_contiguous() or rs.device != dC.device:
        return None
    return rs


def _bias_grad(L, dC, s):
    """Only the layouts the model uses: C contiguous [nb0, nb1, M, N] (or [M, N])."""
    nb0, nb1 = s.nb
    assert s.c[2] == s.N or (s.bias_mode == BIAS_N and s.bias_b0 != 0), 'bias grad needs contiguous C rows'
    if s.bias_mode == BIAS_N and s.bias_b0 != 0:
        # one bias vector per (z0, z1), stored [nb0, nb1, N]: column sums of every C slab as ONE GEMM with a row of ones
        assert s.bias_b0 == nb1 * s.N and s.bias_b1 == s.N
        ones = torch.ones(s.M, dtype=torch.float32, device=dC.device)
        out = _empty(dC, nb0, nb1, s.N)
        _run_gemm(L, ones, dC, out, 1, s.N, s.M, (0, 0, s.M, 1), (s.c[0], s.c[1], 1, s.c[2]), (nb1 * s.N, s.N, s.N), s.nb, 1.0)
        return out
    if s.bias_mode == BIAS_N:
        if nb1 == 1 or s.bias_b1 == 0:
            rows = dC.numel() // s.N
            out = _empty(dC, s.N)
            L.colsum(dC, out, _empty(dC, L.colreduce_ws(rows, s.N, 1)), rows, s.N)
            return out
        assert nb0 == 1 and s.bias_b1 == s.N, 'grouped bias grad layout'
        out = _empty(dC, nb1 * s.N)                    # per-mode biases: C is [nb1, M, N]
        for z in range(nb1):
            L.colsum(dC[z] if dC.dim() == 3 else dC.view(nb1, s.M, s.N)[z], out[z * s.N:(z + 1) * s.N],
                     _empty(dC, L.colreduce_ws(s.M, s.N, 1)), s.M, s.N)
        return out
    # BIAS_M (conv-style, one bias per output row m): row sums, batch-summed
    assert s.bias_b1 == 0
    nbt = nb0 * nb1
    rs = _take_plane_sums(dC, nbt, s.M, s.N)           # left by _UpGN*.backward on the gradient they hand to the lateral: the plane sums in closed form
    if rs is None:
        rs = _empty(dC, nbt * s.M)
        L.rowsum(dC, rs, nbt * s.M, s.N)
    if s.bias_b0 == s.M and nb1 == 1:                  # one bias vector per batch member (conv1x1_per_sample with per-sample biases): no sum over the batch
        return rs.view(nb0, s.M)
    if nbt == 1:
        return rs
    out = _empty(dC, s.M)
    L.colsum(rs, out, _empty(dC, L.colreduce_ws(nbt, s.M, 1)), nbt, s.M)
    return out


def bgemm(A, B, spec, bias=None, gmax=None, gelu=False, drop_p=0.0):
    return _BGemm.apply(A, B, bias, spec, gmax, gelu, float(drop_p))


def linear(x, W, b=None, gelu=False, drop_p=0.0):
    """y = x W^T + b over the last axis (nn.Linear).  x [..., K], W [N, K]."""
    K = x.shape[-1]
    N = W.shape[0]
    R = x.numel() // K
    spec = GemmSpec(R, N, K, (0, 0, K, 1), (0, 0, K, 1), (0, 0, N), tuple(x.shape[:-1]) + (N,), bias_mode=BIAS_N)
    return bgemm(x, W, spec, bias=b, gelu=gelu, drop_p=drop_p)


# -------------------------------------------------------------------------------------------------
# Row kernels
# -------------------------------------------------------------------------------------------------
class _Softmax(_Fn):
    """softmax over the last axis, conditional clip (N5) and attention dropout."""

    @staticmethod
    def forward(ctx, S, clip, gmax, drop_p):
        L = segx.lib()
        S = _c(S)
        Lk = S.shape[-1]
        rows = S.numel() // Lk
        P = torch.empty_like(S)
        Pd = torch.empty_like(S) if drop_p > 0 else None
        seed, off = _Rng.reserve(S.numel()) if drop_p > 0 else (0, 0)
        L.softmax_fwd(S, P, Pd, rows, Lk, clip, gmax, drop_p, seed, off)
        ctx.cfg = (rows, Lk, clip, drop_p, seed, off)
        ctx.save_for_backward(P, S if gmax is not None else None, gmax)
        return Pd if drop_p > 0 else P

    @staticmethod
    def backward(ctx, dP):
        L = segx.lib()
        P, S, gmax = ctx.saved_tensors
        rows, Lk, clip, p, seed, off = ctx.cfg
        dS = torch.empty_like(P)
        L.softmax_bwd(P, _c(dP), S, dS, rows, Lk, clip, gmax, p, seed, off)
        return dS, None, None, None


def softmax(S, clip=500.0, gmax=None, drop_p=0.0):
    return _Softmax.apply(S, float(clip), gmax, float(drop_p))


class _PosBias(_Fn):
    """scores [.., N, N] -> clamp_if(global max > clip)(scores) + weight * sliding positional bias (never materialised)."""

    @staticmethod
    def forward(ctx, S, table, grid_shape, weight, clip, gmax):
        L = segx.lib()
        S, table = _c(S), _c(table)
        N = S.shape[-1]
        nmat = S.numel() // (N * N)
        nd = table.dim()
        dims = ((1,) + tuple(grid_shape)) if nd == 2 else tuple(grid_shape)
        geom = tuple(int(v) for v in dims) + ((table.shape[0] - 1) // 2, nd)
        out = torch.empty_like(S)
        L.posbias_fwd(S, out, table, nmat, N, geom, weight, clip, gmax)
        ctx.cfg = (nmat, N, geom, weight, clip)
        ctx.save_for_backward(S, table, gmax)
        return out

    @staticmethod
    def backward(ctx, dOut):
        L = segx.lib()
        S, table, gmax = ctx.saved_tensors
        nmat, N, geom, weight, clip = ctx.cfg
        dOut = _c(dOut)
        dtable = torch.empty_like(table)
        clamped = gmax is not None and bool(gmax.item() > clip)          # rare branch; one scalar read in backward only
        dS = torch.empty_like(dOut) if clamped else None
        L.posbias_bwd(dOut, S if clamped else None, dS, dtable, nmat, N, geom, weight, clip)
        return (dS if clamped else dOut), dtable, None, None, None, None


def pos_bias_add(S, table, grid_shape, weight=1.0, clip=500.0, gmax=None):
    return _PosBias.apply(S, table, tuple(grid_shape), float(weight), float(clip), gmax)


class _LayerNorm(_Fn):
    @staticmethod
    def forward(ctx, X, w, b, eps):
        L = segx.lib()
        X = _c(X)
        C = X.shape[-1]
        rows = X.numel() // C
        Y = torch.empty_like(X)
        mean, rstd = _empty(X, rows), _empty(X, rows)
        L.layernorm_fwd(X, w, b, Y, mean, rstd, rows, C, eps)
        ctx.save_for_backward(X, w, mean, rstd)
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = segx.lib()
        X, w, mean, rstd = ctx.saved_tensors
        dY = _c(dY)
        C = X.shape[-1]
        rows = X.numel() // C
        dX = torch.empty_like(X)
        L.layernorm_bwd(dY, X, w, mean, rstd, dX, rows, C)
        dw = db = None
        if w is not None:
            dw, db = _empty(X, C), _empty(X, C)
            L.ln_param_grad(dY, X, mean, rstd, dw, db, _empty(X, L.colreduce_ws(rows, C, 2)), rows, C)
        return dX, dw, db, None


def layer_norm(X, w=None, b=None, eps=LN_EPS):
    return _LayerNorm.apply(X, w, b, eps)


class _PreNorm(_Fn):
    """mask * dropout(LN_noaffine(LN_affine(x) + pos_weight * pos[:, :C]))  (segtran_shared.py:916-946)."""
    one_pass = True           # backward: segx_prenorm_bwd_all (False: prenorm_bwd + ln_param_grad + colsum over dU, rounds 1-5; tools/ab_switch.py)

    @staticmethod
    def forward(ctx, X, w1, b1, pos, mask, pos_weight, drop_p):
        L = segx.lib()
        X, mask = _c(X), _c(mask)
        pos = _c(pos) if pos is not None else None            # None: 'bias' codes, single norm (:937-940)
        B, N, C = X.shape
        Y = torch.empty_like(X)
        stats = _empty(X, 4 * B * N)
        seed, off = _Rng.reserve(X.numel()) if drop_p > 0 else (0, 0)
        L.prenorm_fwd(X, w1, b1, pos, pos.shape[1] if pos is not None else 0, pos_weight, mask, Y, stats, B, N, C, LN_EPS, drop_p, seed, off)
        ctx.cfg = (pos_weight, drop_p, seed, off)
        ctx.save_for_backward(X, w1, b1, pos, mask, stats)
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = segx.lib()
        X, w1, b1, pos, mask, stats = ctx.saved_tensors
        pw, p, seed, off = ctx.cfg
        B, N, C = X.shape
        if _PreNorm.one_pass and C <= 2048:
            # r06: dX, the LayerNorm-1 parameter gradients and the positional code's batch sum from ONE kernel; dU is never written (it was written once and read three times)
            dX = torch.empty_like(X)
            dw, db = _empty(X, C), _empty(X, C)
            want_pos = pos is not None
            dsum = _empty(X, N, C) if want_pos else None
            L.prenorm_bwd_all(_c(dY), X, w1, b1, pos, pos.shape[1] if want_pos else 0, pw, mask, stats, dX, dsum, dw, db, _empty(X, L.prenorm_bwd_all_ws(N, C)), B, N, C, p, seed, off)
            dpos = None
            if want_pos and ctx.needs_input_grad[3]:
                dpos = torch.zeros_like(pos)
                dpos[:, :C] = dsum * pw
            return dX, dw, db, dpos, None, None, None
        dX, dU = torch.empty_like(X), torch.empty_like(X)
        L.prenorm_bwd(_c(dY), X, w1, b1, pos, pos.shape[1] if pos is not None else 0, pw, mask, stats, dX, dU, B, N, C, p, seed, off)
        rows = B * N
        dw, db = _empty(X, C), _empty(X, C)
        L.ln_param_grad(dU, X, stats[:rows], stats[rows:2 * rows], dw, db, _empty(X, L.colreduce_ws(rows, C, 2)), rows, C)
        dpos = None
        if pos is not None and ctx.needs_input_grad[3]:
            dsum = _empty(X, N * C)
            L.colsum(dU, dsum, _empty(X, L.colreduce_ws(B, N * C, 1)), B, N * C)
            dpos = torch.zeros_like(pos)
            dpos[:, :C] = dsum.view(N, C) * pw
        return dX, dw, db, dpos, None, None, None


def prenorm(X, w1, b1, pos, mask, pos_weight=1.0, drop_p=0.0):
    return _PreNorm.apply(X, w1, b1, pos, mask, float(pos_weight), float(drop_p))


class _PosEmbed(_Fn):
    """LearnedSinuPosEmbedder on batch-invariant normalised coordinates [N, pd] -> [N, C]."""

    @staticmethod
    def forward(ctx, posn, Wp, bp):
        L = segx.lib()
        posn, Wp = _c(posn), _c(Wp)
        N, pd = posn.shape
        C = Wp.shape[0]
        out = _empty(posn, N, C)
        stats = _empty(posn, 2 * N)
        L.posembed_fwd(posn, Wp, bp, out, stats, N, C, pd, LN_EPS)
        ctx.save_for_backward(posn, Wp, bp, stats)
        return out

    @staticmethod
    def backward(ctx, dOut):
        L = segx.lib()
        posn, Wp, bp, stats = ctx.saved_tensors
        N, pd = posn.shape
        C = Wp.shape[0]
        dZ = _empty(posn, N, C)
        L.posembed_bwd(_c(dOut), posn, Wp, bp, stats, dZ, N, C, pd)
        dW = _empty(posn, C, pd)
        # dWp[c][d] = sum_n dZ[n][c] posn[n][d]   (TN GEMM, inner = tokens)
        _run_gemm(L, dZ, posn, dW, C, pd, N, (0, 0, 1, C), (0, 0, 1, pd), (0, 0, pd), (1, 1), 1.0)
        db = _empty(posn, C)
        L.colsum(dZ, db, _empty(posn, L.colreduce_ws(N, C, 1)), N, C)
        return None, dW, db


def pos_embed(posn, Wp, bp):
    return _PosEmbed.apply(posn, Wp, bp)


class _ModesAggr(_Fn):
    """Z [Mo, R, F] -> LN(dropout(Z)) -> learned soft aggregation over modes -> [R, F]."""
    one_pass = True           # backward: segx_modes_aggr_bwd_all (False: the two passes of rounds 1-5; tools/ab_switch.py compares them on one box)

    @staticmethod
    def forward(ctx, Z, lnw, lnb, wa, ba, drop_p):
        L = segx.lib()
        Z = _c(Z)
        Mo, R, Fd = Z.shape
        Y = _empty(Z, R, Fd)
        stats = _empty(Z, 3 * Mo * R)
        seed, off = _Rng.reserve(Z.numel()) if drop_p > 0 else (0, 0)
        wa_f = _c(wa.reshape(-1))
        L.modes_aggr_fwd(Z, lnw, lnb, wa_f, ba, Y, stats, Mo, R, Fd, LN_EPS, drop_p, seed, off)
        ctx.cfg = (drop_p, seed, off, tuple(wa.shape))
        ctx.save_for_backward(Z, lnw, lnb, wa_f, stats)
        return Y

    @staticmethod
    def backward(ctx, dY):
        L = segx.lib()
        Z, lnw, lnb, wa, stats = ctx.saved_tensors
        p, seed, off, wa_shape = ctx.cfg
        Mo, R, Fd = Z.shape
        dY = _c(dY)
        dZ = torch.empty_like(Z)
        dscore = _empty(Z, Mo * R)
        dlnw, dlnb, dwa = _empty(Z, Fd), _empty(Z, Fd), _empty(Z, Fd)             # lnw None (no LayerNorm): dlnw / dlnb are scratch
        if _ModesAggr.one_pass:
            # one pass over Z and dY for dZ, dscore and the three parameter gradients (r06; the separate parameter-gradient pass re-read both and regenerated the mask)
            L.modes_aggr_bwd_all(dY, Z, lnw, lnb, wa, stats, dZ, dscore, dlnw, dlnb, dwa, _empty(Z, L.modes_aggr_bwd_all_ws(Mo, R, Fd)), Mo, R, Fd, p, seed, off)
        else:
            L.modes_aggr_bwd(dY, Z, lnw, lnb, wa, stats, dZ, dscore, Mo, R, Fd, p, seed, off)
            L.modes_aggr_param_grad(dY, Z, lnw, lnb, wa, stats, dscore, dlnw, dlnb, dwa, _empty(Z, L.colreduce_ws(R, Fd, 3)), Mo, R, Fd, p, seed, off)
        dba = _empty(Z, 1)
        L.sum(dscore, Mo * R, dba, _empty(Z, 1024))
        if lnw is None:
            dlnw = dlnb = None
        return dZ, dlnw, dlnb, dwa.view(wa_shape), dba, None


def modes_aggr(Z, lnw, lnb, wa, ba, drop_p=0.0):
    """lnw = lnb = None: soft aggregation of the raw mode features (no LayerNorm)."""
    return _ModesAggr.apply(Z, lnw, lnb, wa, ba, float(drop_p))


class _Dropout(_Fn):
    @staticmethod
    def forward(ctx, x, p):
        L = segx.lib()
        x = _c(x)
        seed, off = _Rng.reserve(x.numel())
        y = torch.empty_like(x)
        L.dropout(x, y, x.numel(), p, seed, off)
        ctx.cfg = (p, seed, off)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        p, seed, off = ctx.cfg
        dy = _c(dy)
        dx = torch.empty_like(dy)
        L.dropout(dy, dx, dy.numel(), p, seed, off)
        return dx, None


def dropout(x, p, training=True):
    """nn.Dropout(p) as its own pass (only the out-FPN output under --outdrop uses it; every other dropout is fused)."""
    if not training or p <= 0:
        return x
    return _Dropout.apply(x, float(p))


class _AvgPool2(_Fn):
    @staticmethod
    def forward(ctx, x):
        L = segx.lib()
        x = _c(x)
        B, C, H, W = x.shape
        y = _empty(x, B, C, H // 2, W // 2)
        L.avgpool2_fwd(x, y, B * C, H, W)
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        B, C, H, W = ctx.shape
        dx = _empty(dy, B, C, H, W)
        L.avgpool2_bwd(_c(dy), dx, B * C, H, W)
        return dx


def avg_pool2(x):
    """nn.AvgPool2d(2) on [B, C, H, W]."""
    return _AvgPool2.apply(x)


class _Transpose(_Fn):
    @staticmethod
    def forward(ctx, x):
        L = segx.lib()
        x = _c(x)
        B, R, C = x.shape
        y = _empty(x, B, C, R)
        L.transpose(x, y, B, R, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        dy = _c(dy)
        B, C, R = dy.shape
        dx = _empty(dy, B, R, C)
        L.transpose(dy, dx, B, C, R)
        return dx


def transpose12(x):
    """[B, R, C] -> [B, C, R] as a contiguous tensor."""
    return _Transpose.apply(x)


# -------------------------------------------------------------------------------------------------
# Pointwise (1x1 / 1x1x1) convolution on NC[D]HW tensors = one batched GEMM, no layout change:
#   Y[b][co][s] = sum_ci W[co][ci] X[b][ci][s] + bias[co]      (s = flattened spatial index, contiguous)
# -------------------------------------------------------------------------------------------------
def _no_grad_operands(what, *ts):
    """the inference-only ops (BatchNorm folded into their operands) have no backward: refuse an operand a gradient would flow through"""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(what + ' is forward-only (inference with BatchNorm folded): call it under torch.no_grad() or on tensors without gradient')


def conv1x1(x, weight, bias=None, pass_input=False, act=0):
    """x [B, Cin, *spatial]; weight [Cout, Cin, 1, 1(, 1)] (nn.Conv2d / nn.Conv3d layout).  pass_input: -> (y, x_alias); route a second use of x
    (a skip connection) through x_alias and its gradient is added inside the dX GEMM (see _BGemm).
    act = ACT_SWISH: y = swish(conv + bias) from the GEMM's epilogue (SEGX_EPI_SWISH) -- forward only: a pointwise convolution whose BatchNorm was folded
    into weight and bias (EfficientNet.fold_batchnorm)."""
    B, Cin = x.shape[0], x.shape[1]
    S = x.numel() // (B * Cin)
    Cout = weight.shape[0]
    if act != ACT_NONE:
        if act != ACT_SWISH or pass_input:
            raise NotImplementedError('conv1x1: the only fused activation is swish (act = ACT_SWISH), without pass_input')
        _no_grad_operands('conv1x1(act=ACT_SWISH)', x, weight, bias)
        L = segx.lib()
        x, W = _c(x), _c(weight.reshape(Cout, Cin))
        y = _empty(x, B, Cout, *x.shape[2:])
        _run_gemm(L, W, x, y, Cout, S, Cin, (0, 0, Cin, 1), (Cin * S, 0, 1, S), (Cout * S, 0, S), (B, 1), 1.0, bias=bias,
                  bias_mode=BIAS_M if bias is not None else BIAS_NONE, epilogue=EPI_SWISH)
        return y
    spec = GemmSpec(Cout, S, Cin, (0, 0, Cin, 1), (Cin * S, 0, 1, S), (Cout * S, 0, S),
                    (B, Cout) + tuple(x.shape[2:]), nb=(B, 1), bias_mode=BIAS_M)
    if pass_input and x.is_contiguous() and _live(x):
        return _BGemm.apply(weight.reshape(Cout, Cin), x, bias, spec, None, False, 0.0, True)
    y = bgemm(weight.reshape(Cout, Cin), x, spec, bias=bias)
    return (y, x) if pass_input else y


def _chan_slice_bs(v):
    """Sample stride (floats) under which a kernel may address v -- [B, C, *spatial], dense or a channel slice of a wider NC... tensor -- in place: 0 = dense, None =
    not addressable (samples not contiguous inside, or the slice does not start on 16 bytes / its sample stride is no float4 multiple)."""
    if v.data_ptr() % 16:
        return None
    if v.is_contiguous():
        return 0
    if v[0].is_contiguous() and v.stride(0) % 4 == 0:
        return int(v.stride(0))
    return None


def conv1x1_relu(x, weight, bias, out=None):
    """relu(conv1x1(x, weight) + bias) from the GEMM's epilogue (SEGX_EPI_RELU) -- forward only: a pointwise convolution of Inception-I3D whose BatchNorm was folded into
    weight and bias (InceptionI3d.fold_batchnorm).  out: where the result goes -- [B, Cout, *spatial], dense or a channel slice of a wider NC... tensor (the branch's
    place in the module's concatenation: no copy), 16-byte aligned with a sample stride in multiples of four floats."""
    _no_grad_operands('conv1x1_relu', x, weight, bias, out)
    B, Cin = x.shape[0], x.shape[1]
    S = x.numel() // (B * Cin)
    Cout = weight.shape[0]
    L = segx.lib()
    x, W = _c(x), _c(weight.reshape(Cout, Cin))
    if out is None:
        out = _empty(x, B, Cout, *x.shape[2:])
    bs = _chan_slice_bs(out)
    if tuple(out.shape) != (B, Cout) + tuple(x.shape[2:]) or bs is None:
        raise ValueError('conv1x1_relu: out must be [B, Cout, *spatial], dense or a 16-byte aligned channel slice with a sample stride in multiples of 4 floats')
    _run_gemm(L, W, x, out, Cout, S, Cin, (0, 0, Cin, 1), (Cin * S, 0, 1, S), (bs or Cout * S, 0, S), (B, 1), 1.0, bias=bias,
              bias_mode=BIAS_M if bias is not None else BIAS_NONE, epilogue=EPI_RELU)
    return out


def conv1x1_tokens(tokens, grid_shape, weight):
    """Pointwise convolution of a channels-last token tensor [B, N, C] straight into the NC[D]HW map [B, Cout, *grid_shape]
    (y[b, o, n] = sum_c W[o, c] tokens[b, n, c]) -- the [B, N, C] -> [B, C, N] transposition never happens."""
    B, N, C = tokens.shape
    Cout = weight.shape[0]
    spec = GemmSpec(Cout, N, C, (0, 0, C, 1), (N * C, 0, C, 1), (Cout * N, 0, N), (B, Cout) + tuple(int(g) for g in grid_shape), nb=(B, 1))
    return bgemm(weight.reshape(Cout, C), tokens, spec)


def compose_conv1x1(w_out, b_out, w_in, b_in):
    """Weights of conv1x1(conv1x1(x, w_in, b_in), w_out, b_out) as ONE pointwise convolution: W = w_out @ w_in,
    b = w_out @ b_in + b_out (both through the differentiable GEMM op, so each factor still receives its exact gradient)."""
    nc, Fd = w_out.shape[0], w_out.shape[1]
    Cin = w_in.shape[1]
    wo = w_out.reshape(nc, Fd)
    W = bgemm(wo, w_in.reshape(Fd, Cin), GemmSpec(nc, Cin, Fd, (0, 0, Fd, 1), (0, 0, 1, Cin), (0, 0, Cin), (nc, Cin)))
    b = b_out
    if b_in is not None:
        b = linear(b_in.view(1, Fd), wo, b_out).view(nc)
    return W.view((nc, Cin) + tuple(w_out.shape[2:])), b


# -------------------------------------------------------------------------------------------------
# Segmentation loss (train2d.py:1233-1242,1314-1318 / train3d.py:738-756), fused fwd + bwd
# -------------------------------------------------------------------------------------------------
class _SegLoss(_Fn):
    @staticmethod
    def forward(ctx, logits, mask, pos_weight, class_w, dice_w):
        L = segx.lib()
        logits, mask = _c(logits), _c(mask)
        B, C = logits.shape[:2]
        S = logits.numel() // (B * C)
        out = _empty(logits, 3 + C)
        ws = _empty(logits, L.loss_ws(B, C))
        L.seg_loss_fwd(logits, mask, pos_weight, class_w, out, ws, B, C, S, dice_w)
        ctx.cfg = (B, C, S, dice_w)
        ctx.save_for_backward(logits, mask, pos_weight, class_w, ws)
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g2):
        L = segx.lib()
        logits, mask, pw, cw, ws = ctx.saved_tensors
        B, C, S, dice_w = ctx.cfg
        d = torch.empty_like(logits)
        L.seg_loss_bwd(logits, mask, pw, cw, ws, _c(g.reshape(1)), d, B, C, S, dice_w)
        return d, None, None, None, None


def seg_loss(logits, mask_nhot, pos_weight, class_w, dice_w=0.5):
    """Returns (loss, stats) with stats = [loss, ce, dice_total, dice_c0, ...] (device tensor, no host sync)."""
    loss, stats = _SegLoss.apply(logits, mask_nhot.to(torch.float32), pos_weight, class_w, float(dice_w))
    return loss, stats


# -------------------------------------------------------------------------------------------------
# Backbone ops (backbone.hip): BatchNorm + activation, depthwise conv, squeeze-excite
# -------------------------------------------------------------------------------------------------
ACT_NONE, ACT_SWISH, ACT_RELU, ACT_LEAKY = 0, 1, 2, 3
_bn_stats_sync = None        # set by segtran_amd.dist for data-parallel runs: merges (mean, var, count) across ranks
_bn_grad_sync = None         # idem: all-reduces the (sum du*xhat, sum du) pair of the BN backward


def _bn_forward(L, x, w, b, run_mean, run_var, training, momentum, eps, act, B, C, S, pool=False, resid=None, dc=(0.0, 0, 0), out=None):
    """BatchNorm (+ activation, + squeeze-excite pooling chunks, + drop_connect scale and skip add) -> (y, mean, var, n, psum, nch).
    Training, one process: ONE call of segx_bn_act_fwd2 -- one launch where a channel fits a workgroup's or a team of workgroups' registers, else a
    statistics-partials launch + the apply pass that merges them.
    Synchronised: local statistics -> ONE all-gather -> merge kernel -> the same apply pass on the merged statistics.  Eval: the apply pass alone.
    out: a channel slice [B, C, ...] of a wider tensor (planes contiguous, see _slice_writable) that receives y in place of a fresh tensor."""
    y = torch.empty_like(x) if out is None else out
    y_bs = 0 if out is None else out.stride(0)
    auto = training and _bn_stats_sync is None              # the library computes the statistics itself (channel-resident: one launch for the layer)
    nch = L.bn_pool_chunks(B, S, auto) if pool else 0
    psum = _empty(x, B * C * nch) if pool else None
    dc_p, seed, off = dc
    if not training:
        L.bn_act_fwd2(x, None, 0, run_mean, run_var, None, None, 0.0, w, b, y, psum, resid, 0.0, 0, 0, B, C, S, eps, act, y_bs=y_bs)
        return y, run_mean, run_var, B * S, psum, nch
    mean, var = _empty(x, C), _empty(x, C)
    if _bn_stats_sync is None:
        parts = _empty(x, L.bn_parts_floats(B, C, S))
        L.bn_act_fwd2(x, parts, 0, mean, var, run_mean, run_var, momentum, w, b, y, psum, resid, dc_p, seed, off, B, C, S, eps, act, y_bs=y_bs)
        return y, mean, var, B * S, psum, nch
    # synchronised BN: ONE local partial (n, mean, M2) per channel (one launch for channel-resident shapes), ONE all-gather of [C] float4, and the
    # apply pass merges the ranks' partials itself (Chan) and updates the running statistics: 2-3 launches + 1 collective (r03: 5 + 1)
    loc = _empty(x, 4 * C)
    L.bn_stats_local(x, loc, _empty(x, L.bn_parts_floats(B, C, S)), B, C, S)
    allv, world = _bn_stats_sync(loc)
    L.bn_act_fwd2(x, allv, -world, mean, var, run_mean, run_var, momentum, w, b, y, psum, resid, dc_p, seed, off, B, C, S, eps, act, y_bs=y_bs)
    return y, mean, var, B * S * world, psum, nch


def _plane_strided(dy, S):
    """(tensor, batch stride) under which the BatchNorm backward kernels read dy: dense -> (dy, 0); a channel slice of a wider tensor whose (sample,
    channel) planes are contiguous -- one operand's share of a channel concatenation's gradient (torch.cat's backward hands out narrow() views) ->
    (dy, its batch stride), read in place; anything else -> a contiguous copy."""
    if dy.is_contiguous():
        return dy, 0
    if dy.dim() >= 3 and dy.stride(1) == S and dy[0].is_contiguous() and dy.stride(0) % 4 == 0 and dy.storage_offset() % 4 == 0 and S % 4 == 0:
        return dy, dy.stride(0)
    return dy.contiguous(), 0


def _bn_act_backward(L, dy, x, mean, var, w, b, cfg, gate=None, dpool=None, inv_S=0.0, dc=(0.0, 0, 0)):
    """dx, dw, db of BatchNorm + activation; gate / dpool: a squeeze-excite gate sits behind it (see segx_bn_act_bwd); dc: the drop_connect scale
    of the forward multiplies dy.  One process: two launches (segx_bn_act_bwd2: the apply pass sums the reduction partials itself)."""
    B, C, S, eps, act, training, n = cfg
    dx = torch.empty_like(x)
    dy, dy_bs = _plane_strided(dy, S)
    if training and _bn_grad_sync is not None:
        dy = _c(dy)
        # synchronised BN: local sums written into one [2C] buffer -> ONE all-reduce -> apply with the global sums / global count.
        # The parameter gradients stay the LOCAL sums (the flat-gradient all-reduce averages them like every other gradient).
        both = _empty(x, 2 * C)
        dw, db = both[:C], both[C:]
        L.bn_act_bwd_reduce(dy, x, mean, var, w, b, dw, db, _empty(x, L.bn_ws(B, C)), B, C, S, eps, act, gate, dpool, inv_S, *dc)
        glob = _bn_grad_sync(both)
        L.bn_act_bwd_apply(dy, x, mean, var, w, b, glob[:C], glob[C:], dx, B, C, S, eps, act, 1.0 / n, gate, dpool, inv_S, *dc)
    else:
        dw, db = _empty(x, C), _empty(x, C)
        L.bn_act_bwd2(dy, x, mean, var, w, b, dx, dw, db, _empty(x, L.bn_ws(B, C, S)), B, C, S, eps, act, 1 if training else 0, gate, dpool, inv_S, *dc, dy_bs=dy_bs)
    return dx, dw, db


class _BNAct(_Fn):
    """y = act(batch_norm(x)) [* drop_connect scale of the sample + resid]: the BatchNorm of every backbone layer; with `resid` also the tail of an
    MBConv block (efficientnet/model.py:116-122) -- the per-sample scale is drawn inside the kernels from the Philox stream, nothing is stored."""

    @staticmethod
    def forward(ctx, x, w, b, run_mean, run_var, training, momentum, eps, act, resid, dc_p):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[0], x.shape[1]
        S = x.numel() // (B * C)
        resid = _c(resid) if resid is not None else None
        dc = (dc_p,) + _Rng.reserve(B) if (dc_p > 0 and training and resid is not None) else (0.0, 0, 0)
        y, mean, var, n, _, _ = _bn_forward(L, x, w, b, run_mean, run_var, training, momentum, eps, act, B, C, S, resid=resid, dc=dc)
        ctx.cfg = (B, C, S, eps, act, training, n)
        ctx.dc, ctx.has_resid = dc, resid is not None
        ctx.save_for_backward(x, mean, var, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        x, mean, var, w, b = ctx.saved_tensors
        dx, dw, db = _bn_act_backward(L, dy, x, mean, var, w, b, ctx.cfg, dc=ctx.dc)      # dy may be a channel slice of a concatenation's gradient: read in place
        return dx, dw, db, None, None, None, None, None, None, (dy if ctx.has_resid else None), None


def _slice_writable(view, S):
    """May a BatchNorm forward kernel write this channel slice of a wider tensor in place (segx_bn_act_fwd2 y_bs)?  Planes contiguous and 16-byte aligned."""
    return (S % 4 == 0 and view.stride(1) == S and view[0].is_contiguous() and view.stride(0) % 4 == 0 and view.storage_offset() % 4 == 0
            and view.data_ptr() % 16 == 0)


class _BNActCat(_Fn):
    """torch.cat([head, act(bn_1(x_1)), ..., act(bn_n(x_n))], dim=1) -- the tail of an Inception module (aj_i3d.py:101-118) -- with every BatchNorm writing its
    channels where they belong in the concatenation (segx_bn_act_fwd2 y_bs) instead of into a tensor of its own that a copy kernel then moves: one pass over each
    branch less, forward.  Backward is what autograd did with the separate nodes: each BatchNorm reads its channel slice of the concatenation's gradient in place
    (_plane_strided), the head's gradient is the narrow view torch.cat's backward hands out."""

    @staticmethod
    def forward(ctx, head, training, act, *flat):
        L = segx.lib()
        n = len(flat) // 7
        xs = [_c(flat[7 * i]) for i in range(n)]
        B, c0 = head.shape[0], head.shape[1]
        sp = tuple(head.shape[2:])
        S = 1
        for v in sp:
            S *= int(v)
        Cs = [int(x.shape[1]) for x in xs]
        out = _empty(head, B, c0 + sum(Cs), *sp)
        out[:, :c0].copy_(head)
        saved, cfgs, off = [], [], c0
        # r06 (reference train2d.py:1109 nn.SyncBatchNorm, one exchange per LAYER): the branch-final BatchNorms of an Inception module are
        # independent of each other, so their synchronised statistics travel in ONE all-gather (and their backward sums in ONE all-reduce): with the fused head
        # (bn_act_multi) a module costs 2 + 2 collectives instead of 4 + 4 (6 + 6 in the reference's layer-by-layer form)
        presync = None
        if training and _bn_stats_sync is not None and n > 1:
            loc = _empty(head, 4 * sum(Cs))
            o4 = 0
            for i in range(n):
                L.bn_stats_local(xs[i], loc[o4:o4 + 4 * Cs[i]], _empty(head, L.bn_parts_floats(B, Cs[i], S)), B, Cs[i], S)
                o4 += 4 * Cs[i]
            allv, world = _bn_stats_sync(loc)
            allv, presync, o4 = allv.view(world, -1), [], 0
            for i in range(n):
                presync.append((allv[:, o4:o4 + 4 * Cs[i]].contiguous().view(-1), world))      # [world][C_i] float4: what segx_bn_act_fwd2 merges (nparts = -world)
                o4 += 4 * Cs[i]
        for i in range(n):
            x, (w, b, rm, rv, mom, eps) = xs[i], flat[7 * i + 1:7 * i + 7]
            assert x.shape[0] == B and tuple(x.shape[2:]) == sp
            dst = out[:, off:off + Cs[i]]
            if presync is not None:
                ok = _slice_writable(dst, S)
                y = dst if ok else torch.empty_like(x)
                mean, var = _empty(x, Cs[i]), _empty(x, Cs[i])
                L.bn_act_fwd2(x, presync[i][0], -presync[i][1], mean, var, rm, rv, mom, w, b, y, None, None, 0.0, 0, 0, B, Cs[i], S, eps, act, y_bs=dst.stride(0) if ok else 0)
                if not ok:
                    dst.copy_(y)
                cnt = B * S * presync[i][1]
            elif _slice_writable(dst, S):
                _, mean, var, cnt, _, _ = _bn_forward(L, x, w, b, rm, rv, training, mom, eps, act, B, Cs[i], S, out=dst)
            else:                                                                          # rows that are not float4 multiples: a tensor of its own + the copy
                y, mean, var, cnt, _, _ = _bn_forward(L, x, w, b, rm, rv, training, mom, eps, act, B, Cs[i], S)
                dst.copy_(y)
            saved += [x, mean, var, w, b]
            cfgs.append((B, Cs[i], S, eps, act, training, cnt))
            off += Cs[i]
        ctx.cfgs, ctx.c0 = cfgs, c0
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = segx.lib()
        sv = ctx.saved_tensors
        grads, off = [], ctx.c0
        if ctx.cfgs and ctx.cfgs[0][5] and _bn_grad_sync is not None and len(ctx.cfgs) > 1:
            # synchronised: the local (sum du * xhat, sum du) pairs of all branches in ONE buffer -> ONE all-reduce -> the apply passes (see forward)
            Ct = sum(cfg[1] for cfg in ctx.cfgs)
            both = _empty(dout, 2 * Ct)
            dys, o2 = [], 0
            for i, cfg in enumerate(ctx.cfgs):
                x, mean, var, w, b = sv[5 * i:5 * i + 5]
                B, C, S, eps, act, training, n = cfg
                dy = _c(dout[:, off:off + C])
                L.bn_act_bwd_reduce(dy, x, mean, var, w, b, both[o2:o2 + C], both[o2 + C:o2 + 2 * C], _empty(x, L.bn_ws(B, C)), B, C, S, eps, act, None, None, 0.0, 0.0, 0, 0)
                dys.append(dy); o2 += 2 * C; off += C
            glob, o2 = _bn_grad_sync(both), 0
            for i, cfg in enumerate(ctx.cfgs):
                x, mean, var, w, b = sv[5 * i:5 * i + 5]
                B, C, S, eps, act, training, n = cfg
                dx = torch.empty_like(x)
                L.bn_act_bwd_apply(dys[i], x, mean, var, w, b, glob[o2:o2 + C], glob[o2 + C:o2 + 2 * C], dx, B, C, S, eps, act, 1.0 / n, None, None, 0.0, 0.0, 0, 0)
                grads += [dx, both[o2:o2 + C], both[o2 + C:o2 + 2 * C], None, None, None, None]
                o2 += 2 * C
            return (dout[:, :ctx.c0], None, None) + tuple(grads)
        for i, cfg in enumerate(ctx.cfgs):
            x, mean, var, w, b = sv[5 * i:5 * i + 5]
            dx, dw, db = _bn_act_backward(L, dout[:, off:off + cfg[1]], x, mean, var, w, b, cfg)
            grads += [dx, dw, db, None, None, None, None]
            off += cfg[1]
        return (dout[:, :ctx.c0], None, None) + tuple(grads)


def bn_act_cat(head, branches, act=ACT_NONE):
    """cat([head] + [act(bn(x)) for x, bn in branches], dim=1); `bn` = nn.BatchNorm2d/3d modules (parameter containers), all in the same mode."""
    flat = []
    for x, bn in branches:
        _bn_tick(bn)
        flat += [x, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps)]
    training = branches[0][1].training
    assert all(bn.training == training for _, bn in branches)
    return _BNActCat.apply(head, training, act, *flat)


_bn_ticks = None          # a list while a model forward defers the `num_batches_tracked += 1` of its BatchNorm layers (defer_bn_ticks)


def defer_bn_ticks():
    """Segtran2d/3d.forward: collect the num_batches_tracked counters of the BatchNorm layers that run in training mode ..."""
    global _bn_ticks
    if _bn_ticks is None:
        _bn_ticks = []


def flush_bn_ticks():
    """... and bump them with ONE multi-tensor launch at the end of the pass (96 layers in EfficientNet-B4: 96 scalar kernels otherwise)."""
    global _bn_ticks
    ticks, _bn_ticks = _bn_ticks, None
    if ticks:
        torch._foreach_add_(ticks, 1)


def _bn_tick(bn):
    if bn.training and bn.num_batches_tracked is not None:
        if _bn_ticks is not None:
            _bn_ticks.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked.add_(1)


def bn_act(x, bn, act=ACT_NONE, resid=None, drop_connect=0.0):
    """nn.BatchNorm2d/3d module `bn` (parameter container) followed by an activation, fused; resid / drop_connect: + the MBConv skip connection
    (y * drop_connect scale of the sample + resid) in the same pass."""
    _bn_tick(bn)
    return _BNAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum), float(bn.eps), act, resid,
                        float(drop_connect or 0.0))


class _AddRelu(_Fn):
    """y = relu(z + resid): the end of a ResNet block (resnet.py:59-64 / :110-115 of the reference) as one streaming pass (resnet.hip).  The backward needs y
    only, and z and resid receive the same gradient tensor."""

    @staticmethod
    def forward(ctx, z, resid):
        L = segx.lib()
        z = _c(z)
        resid = _c(resid) if resid is not None else None
        B, C = z.shape[0], z.shape[1]
        S = z.numel() // (B * C)
        y = torch.empty_like(z)
        L.add_relu_fwd(z, resid, None, y, B * C, C, S)
        ctx.cfg = (B * C, S)
        ctx.has_resid = resid is not None
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        (y,) = ctx.saved_tensors
        dz = torch.empty_like(y)
        L.add_relu_bwd(_c(dy), y, dz, *ctx.cfg)
        return dz, (dz if ctx.has_resid else None)


def add_relu(z, resid=None, bias=None, out=None):
    """relu((z + bias[channel]) + resid) on [B, C, *spatial] maps, the additions in that order; a NaN operand gives NaN (torch.relu).  The end of a ResNet block:
    training / unfolded    add_relu(bn_act(conv_out, bn_last, ACT_NONE, resid=shortcut))   -- the skip add stays in the BatchNorm apply pass;
    BatchNorm folded       add_relu(z, shortcut, bias=b_last + b_down, out=z)             -- forward only (_no_grad_operands), in place.
    resid: same shape as z.  bias: [C].  out: a dense tensor of z's shape that receives the result (z itself allowed); forward only as well."""
    if z.dim() < 2 or z.numel() == 0:
        raise ValueError('add_relu: z must be a non-empty [B, C, *spatial] map, got %s' % (tuple(z.shape),))
    if resid is not None and resid.shape != z.shape:
        raise ValueError('add_relu: resid %s does not match z %s' % (tuple(resid.shape), tuple(z.shape)))
    if bias is None and out is None:
        return _AddRelu.apply(z, resid)
    if bias is not None and bias.requires_grad and torch.is_grad_enabled():
        raise RuntimeError('add_relu: the bias gradient is not built (a bias exists only with BatchNorm folded, in inference): call it under torch.no_grad() '
                           'or with a bias that does not require grad')
    _no_grad_operands('add_relu(bias= / out=)', z, resid, bias, out)
    B, C = z.shape[0], z.shape[1]
    if bias is not None and bias.numel() != C:
        raise ValueError('add_relu: bias has %d elements for %d channels' % (bias.numel(), C))
    if out is None:
        out = torch.empty_like(z, memory_format=torch.contiguous_format)
    elif out.shape != z.shape or not out.is_contiguous():
        raise ValueError('add_relu: out must be a dense tensor of the shape of z')
    zc = _c(z)
    segx.lib().add_relu_fwd(zc, _c(resid) if resid is not None else None, _c(bias) if bias is not None else None, out, B * C, C, z.numel() // (B * C))
    return out


def bn_act_multi(x, bns, act=ACT_NONE):
    """BatchNorm (+ activation) of SEVERAL BatchNorm modules in one pass: x's channels are the concatenation of the modules' channels (the outputs
    of convolutions that were run as one convolution with concatenated filters).  BatchNorm is per channel, so this is exactly the separate
    layers -- with one statistics pass, one apply pass and, when synchronised, ONE exchange for all of them.  Same momentum / eps required."""
    mom, eps, training = float(bns[0].momentum), float(bns[0].eps), bns[0].training
    assert all(float(b.momentum) == mom and float(b.eps) == eps and b.training == training for b in bns)
    w, b = torch.cat([m.weight for m in bns]), torch.cat([m.bias for m in bns])
    rm, rv = torch.cat([m.running_mean for m in bns]), torch.cat([m.running_var for m in bns])
    y = _BNAct.apply(x, w, b, rm, rv, training, mom, eps, act, None, 0.0)
    if training:
        sizes = [m.num_features for m in bns]
        with torch.no_grad():
            torch._foreach_copy_([m.running_mean for m in bns] + [m.running_var for m in bns], list(rm.split(sizes)) + list(rv.split(sizes)))
        for m in bns:
            if m.num_batches_tracked is not None:
                if _bn_ticks is not None:
                    _bn_ticks.append(m.num_batches_tracked)
                else:
                    m.num_batches_tracked.add_(1)
    return y


class _DWConv(_Fn):
    fused_backward = True     # stride-1 'same' layers: segx_dwconv2d_bwd_fused (False: data and weight gradient as two kernels, rounds 1-5; tools/ab_switch.py)

    @staticmethod
    def forward(ctx, x, w, stride, pad):
        L = segx.lib()
        x, w = _c(x), _c(w)
        B, C, H, W = x.shape
        k = w.shape[-1]
        pl, pr, pt, pb = pad
        OH, OW = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
        y = _empty(x, B, C, OH, OW)
        L.dwconv2d_fwd(x, w, y, B, C, H, W, OH, OW, k, stride, pt, pl)
        ctx.cfg = (B, C, H, W, OH, OW, k, stride, pt, pl)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        x, w = ctx.saved_tensors
        B, C, H, W, OH, OW, k, stride, pt, pl = ctx.cfg
        dy = _c(dy)
        dx = dw = None
        fr = 0
        if _DWConv.fused_backward and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0:
            fr = L.dwconv2d_bwd_fused_rows(H, W, OH, OW, k, stride, pt, pl)
        if fr:
            # r06: stride-1 'same' layers -- dx and the weight-gradient partials from ONE pass over dy (the separate kernels read it twice)
            dx = torch.empty_like(x)
            part = _empty(x, B * fr, C * k * k)
            L.dwconv2d_bwd_fused(dy, x, w, dx, part, B, C, H, W, OH, OW, k, stride, pt, pl)
            dw = _empty(x, C * k * k)
            L.colsum(part, dw, _empty(x, L.colreduce_ws(B * fr, C * k * k, 1)), B * fr, C * k * k)
            return dx, dw.view_as(w), None, None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.dwconv2d_bwd_data(dy, w, dx, B, C, H, W, OH, OW, k, stride, pt, pl)
        if ctx.needs_input_grad[1]:
            dw = _empty(x, C * k * k)
            if not L.dwconv2d_bwd_weight_direct(dy, x, dw, B, C, H, W, OH, OW, k, stride, pt, pl):      # one launch where a channel is one workgroup's work
                rows = B * L.dwconv2d_wgrad_rows(OH, OW)
                part = _empty(x, rows, C * k * k)
                L.dwconv2d_bwd_weight(dy, x, part, B, C, H, W, OH, OW, k, stride, pt, pl)
                L.colsum(part, dw, _empty(x, L.colreduce_ws(rows, C * k * k, 1)), rows, C * k * k)
            dw = dw.view_as(w)
        return dx, dw, None, None


def dwconv2d(x, w, stride, pad):
    """Depthwise conv; w [C,1,k,k]; pad = (left, right, top, bottom) zero padding (F.pad order)."""
    return _DWConv.apply(x, w, int(stride), tuple(int(p) for p in pad))


def _se_excite(L, x, psum, nch, S, w1, b1, w2, b2, Wproj=None):
    """The excitation MLP on the pooling chunks of the BatchNorm pass (segx_se_fwd2, two launches): -> (p, hpre, gate, W1, W2, Wb or None)."""
    B, C = x.shape[0], x.shape[1]
    Cs = w1.shape[0]
    W1, W2 = _c(w1.reshape(Cs, C)), _c(w2.reshape(C, Cs))
    p, hpre, gate = _empty(x, B, C), _empty(x, B, Cs), _empty(x, B, C)
    M = Wproj.shape[0] if Wproj is not None else 0
    Wb = _empty(x, B, M, C) if Wproj is not None else None
    L.se_fwd2(psum, nch, 1.0 / S, W1, b1, W2, b2, Wproj, p, hpre, gate, Wb, B, C, Cs, M)
    return p, hpre, gate, W1, W2, Wb


def _se_excite_backward(L, x, dWb, Wproj, dgate, gate, hpre, p, W1, W2, S):
    """-> (dpool, dW1, db1, dW2, db2, dWproj) from the per-sample projection weight gradient dWb (or from dgate): segx_se_bwd2, three launches."""
    B, C = gate.shape
    Cs = hpre.shape[1]
    dpool = _empty(x, B * C)
    dW1, db1, dW2, db2 = _empty(x, Cs, C), _empty(x, Cs), _empty(x, C, Cs), _empty(x, C)
    dWproj = torch.empty_like(Wproj) if Wproj is not None else None
    M = Wproj.shape[0] if Wproj is not None else 0
    L.se_bwd2(dWb, Wproj, dgate, gate, hpre, p, W1, W2, 1.0 / S, dpool, dW1, db1, dW2, db2, dWproj, _empty(x, L.se_ws2(B, C, Cs)), B, C, Cs, M)
    return dpool, dW1, db1, dW2, db2, dWproj


class _BNActSE(_Fn):
    """squeeze_excite(bn_act(x)) as ONE op (MBConvBlock.forward, efficientnet/model.py:101-110): the squeeze-excite pooling comes out of the
    BatchNorm + swish pass (no separate plane-sum pass over y), and in backward the gate's product rule -- dy = dz * gate + dpool / S -- is
    applied on the fly by the BatchNorm backward kernels instead of being written out by a pass of its own."""

    @staticmethod
    def forward(ctx, x, w, b, run_mean, run_var, training, momentum, eps, act, w1, b1, w2, b2):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[0], x.shape[1]
        S = x.numel() // (B * C)
        y, mean, var, n, psum, nch = _bn_forward(L, x, w, b, run_mean, run_var, training, momentum, eps, act, B, C, S, pool=True)
        p, hpre, gate, W1, W2, _ = _se_excite(L, x, psum, nch, S, w1, b1, w2, b2)
        z = torch.empty_like(x)
        L.plane_scale(y, gate, z, B * C, S)
        ctx.cfg = (B, C, S, eps, act, training, n)
        ctx.shapes = (tuple(w1.shape), tuple(w2.shape))
        ctx.save_for_backward(x, mean, var, w, b, y, p, hpre, gate, W1, W2)
        return z

    @staticmethod
    def backward(ctx, dz):
        L = segx.lib()
        x, mean, var, w, b, y, p, hpre, gate, W1, W2 = ctx.saved_tensors
        B, C, S = ctx.cfg[:3]
        w1s, w2s = ctx.shapes
        dz = _c(dz)
        dgate = _empty(x, B * C)
        L.plane_dot(dz, y, dgate, B * C, S)
        dpool, dW1, db1, dW2, db2, _ = _se_excite_backward(L, x, None, None, dgate, gate, hpre, p, W1, W2, S)
        dx, dw, db = _bn_act_backward(L, dz, x, mean, var, w, b, ctx.cfg, gate.reshape(-1), dpool, 1.0)
        return dx, dw, db, None, None, None, None, None, None, dW1.view(w1s), db1, dW2.view(w2s), db2


class _BNActGateW(_Fn):
    """The middle of an MBConv block (efficientnet/model.py:100-113) up to the operands of its projection GEMM: BatchNorm + swish of the depthwise
    output, the squeeze-excite gate from the same pass, and the gate folded straight into per-sample projection weights
    Wb[b] = W_project * gate[b] (exact re-association).  Returns (y, Wb): project_conv(y * gate) == conv1x1_per_sample(y, Wb).
    Forward: 4 launches (statistics partials, apply + pooling chunks, hidden layer, gate + weights); backward from (dy, dWb): 3 + 2."""

    @staticmethod
    def forward(ctx, x, w, b, run_mean, run_var, training, momentum, eps, act, w1, b1, w2, b2, Wproj):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[0], x.shape[1]
        S = x.numel() // (B * C)
        Wp = _c(Wproj.reshape(Wproj.shape[0], C))
        y, mean, var, n, psum, nch = _bn_forward(L, x, w, b, run_mean, run_var, training, momentum, eps, act, B, C, S, pool=True)
        p, hpre, gate, W1, W2, Wb = _se_excite(L, x, psum, nch, S, w1, b1, w2, b2, Wp)
        ctx.cfg = (B, C, S, eps, act, training, n)
        ctx.shapes = (tuple(w1.shape), tuple(w2.shape), tuple(Wproj.shape))
        ctx.save_for_backward(x, mean, var, w, b, p, hpre, gate, W1, W2, Wp)
        return y, Wb

    @staticmethod
    def backward(ctx, dy, dWb):
        L = segx.lib()
        x, mean, var, w, b, p, hpre, gate, W1, W2, Wp = ctx.saved_tensors
        S = ctx.cfg[2]
        w1s, w2s, wps = ctx.shapes
        dWb = _c(dWb) if dWb is not None else torch.zeros(gate.shape[0], Wp.shape[0], Wp.shape[1], dtype=torch.float32, device=x.device)
        dpool, dW1, db1, dW2, db2, dWp = _se_excite_backward(L, x, dWb, Wp, None, gate, hpre, p, W1, W2, S)
        dx, dw, db = _bn_act_backward(L, _c(dy), x, mean, var, w, b, ctx.cfg, None, dpool, 1.0)
        return dx, dw, db, None, None, None, None, None, None, dW1.view(w1s), db1, dW2.view(w2s), db2, dWp.view(wps)


def bn_act_gate_weights(x, bn, act, w1, b1, w2, b2, proj_weight):
    """(bn_act(x, bn, act), per-sample projection weights [B, Cout, C] carrying the squeeze-excite gate) -- see _BNActGateW; pair with conv1x1_per_sample."""
    _bn_tick(bn)
    return _BNActGateW.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum), float(bn.eps), act, w1, b1, w2, b2,
                             proj_weight)


class _MBConvMid(_Fn):
    """The middle of a stride-1 MBConv block in training mode as ONE op: (y, Wb) = _BNActGateW(dwconv2d(_BNAct(e, bn0, swish)), bn1, swish, squeeze-excite, W_project)
    with the three tensor ops in one launch per direction (segx_mbconv_mid_fwd / _bwd: one workgroup owns a channel; 3 + 4 passes over the expanded tensor instead
    of 6 + 10).  Saved for backward: e, the convolution's output d and the four statistics; swish(bn0(e)) is recomputed.  Only for shapes segx_mbconv_mid_ok
    accepts and one process (synchronised BatchNorm exchanges statistics between the launches' halves): MBConvBlock.forward routes."""

    @staticmethod
    def forward(ctx, e, w0, b0, rm0, rv0, mom0, eps0, wdw, w1, b1, rm1, rv1, mom1, eps1, sw1, sb1, sw2, sb2, Wproj):
        L = segx.lib()
        e, wdw = _c(e), _c(wdw)
        if e.data_ptr() % 16:
            e = e.clone()
        B, C, H, W = e.shape
        k, S = wdw.shape[-1], H * W
        Wp = _c(Wproj.reshape(Wproj.shape[0], C))
        d, y = torch.empty_like(e), torch.empty_like(e)
        psum, stats = _empty(e, B * C), _empty(e, 4, C)                # stats: mean0, var0, mean1, var1
        L.mbconv_mid_fwd(e, w0, b0, rm0, rv0, wdw, w1, b1, rm1, rv1, d, y, psum, stats[0], stats[1], stats[2], stats[3], mom0, eps0, mom1, eps1, B, C, H, W, k)
        p, hpre, gate, W1, W2, Wb = _se_excite(L, y, psum, 1, S, sw1, sb1, sw2, sb2, Wp)
        ctx.cfg = (B, C, H, W, k, eps0, eps1)
        ctx.shapes = (tuple(sw1.shape), tuple(sw2.shape), tuple(Wproj.shape), tuple(wdw.shape))
        ctx.save_for_backward(e, d, stats, w0, b0, wdw, w1, b1, p, hpre, gate, W1, W2, Wp)
        return y, Wb

    @staticmethod
    def backward(ctx, dy, dWb):
        L = segx.lib()
        e, d, stats, w0, b0, wdw, w1, b1, p, hpre, gate, W1, W2, Wp = ctx.saved_tensors
        B, C, H, W, k, eps0, eps1 = ctx.cfg
        w1s, w2s, wps, wds = ctx.shapes
        dWb = _c(dWb) if dWb is not None else torch.zeros(B, Wp.shape[0], C, dtype=torch.float32, device=e.device)
        dy = _c(dy) if dy is not None else torch.zeros_like(e)
        if dy.data_ptr() % 16:
            dy = dy.clone()
        dpool, dW1, db1, dW2, db2, dWp = _se_excite_backward(L, e, dWb, Wp, None, gate, hpre, p, W1, W2, H * W)
        de, g, dwd = torch.empty_like(e), _empty(e, 4, C), _empty(e, C * k * k)       # g: dw0, db0, dw1, db1
        L.mbconv_mid_bwd(dy, dpool, d, e, stats[0], stats[1], stats[2], stats[3], w0, b0, w1, b1, wdw, de, g[0], g[1], g[2], g[3], dwd, 1.0, eps0, eps1, B, C, H, W, k)
        return (de, g[0], g[1], None, None, None, None, dwd.view(wds), g[2], g[3], None, None, None, None,
                dW1.view(w1s), db1, dW2.view(w2s), db2, dWp.view(wps))


def mbconv_mid_ok(e_shape, k):
    """does the channel-resident op below serve an expanded tensor of this shape and a k x k stride-1 'same' depthwise convolution?"""
    return len(e_shape) == 4 and segx.lib().mbconv_mid_ok(e_shape[0], e_shape[1], e_shape[2], e_shape[3], int(k))


def mbconv_mid(e, bn0, dw_weight, bn1, w1, b1, w2, b2, proj_weight):
    """(swish(bn1(dwconv(swish(bn0(e))))), per-sample projection weights carrying the squeeze-excite gate) -- see _MBConvMid; pair with conv1x1_per_sample.
    Both BatchNorm modules are in training mode and mbconv_mid_ok(e.shape, k) holds (the caller checks)."""
    _bn_tick(bn0)
    _bn_tick(bn1)
    return _MBConvMid.apply(e, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var, float(bn0.momentum), float(bn0.eps), dw_weight,
                            bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, float(bn1.momentum), float(bn1.eps), w1, b1, w2, b2, proj_weight)


class _BNActDWConv(_Fn):
    """BatchNorm0 + swish + the depthwise convolution behind it in training mode as ONE op: d = dwconv2d(_BNAct(e, bn0, swish), stride), one team launch per direction.
    stride 2 (segx_bn_dw_s2_fwd / _bwd: the entry of a stride-2 MBConv block, 1 1/4 + 2 1/4 passes over the expanded tensor instead of 3 1/4 + 5 1/2) or stride 1 with 'same'
    padding (segx_bn_dw_s1_fwd / _bwd: 2 + 3 passes instead of 4 + 6).  Saved for backward: e and the two statistics; swish(bn0(e)) is neither written nor kept.
    Only for shapes bn_dw_s2_ok / bn_dw_s1_ok accept and one process: MBConvBlock.forward and EfficientNet.extract_endpoints route."""

    @staticmethod
    def forward(ctx, e, w0, b0, rm0, rv0, mom0, eps0, wdw, pt, pl, stride):
        L = segx.lib()
        e, wdw = _c(e), _c(wdw)
        if e.data_ptr() % 16:
            e = e.clone()
        B, C, H, W = e.shape
        k = wdw.shape[-1]
        d, stats = _empty(e, B, C, H // stride, W // stride), _empty(e, 2, C)     # stats: mean0, var0
        if stride == 2:
            L.bn_dw_s2_fwd(e, w0, b0, rm0, rv0, wdw, d, stats[0], stats[1], _empty(e, L.bn_dw_s2_ws(B, C, H, W, False)), mom0, eps0, B, C, H, W, k, pt, pl)
        else:
            L.bn_dw_s1_fwd(e, w0, b0, rm0, rv0, wdw, d, stats[0], stats[1], _empty(e, L.bn_dw_s1_ws(B, C, H, W, False)), mom0, eps0, B, C, H, W, k, pt, pl)
        ctx.cfg = (B, C, H, W, k, pt, pl, eps0, tuple(wdw.shape), stride)
        ctx.save_for_backward(e, stats, w0, b0, wdw)
        return d

    @staticmethod
    def backward(ctx, dd):
        L = segx.lib()
        e, stats, w0, b0, wdw = ctx.saved_tensors
        B, C, H, W, k, pt, pl, eps0, wds, stride = ctx.cfg
        dd = _c(dd)
        if dd.data_ptr() % 16:
            dd = dd.clone()
        rows = L.bn_dw_s2_rows(B, H, W) if stride == 2 else L.bn_dw_s1_rows(B, H, W)
        de, g, part = torch.empty_like(e), _empty(e, 2, C), _empty(e, rows, C * k * k)      # g: dw0, db0
        if stride == 2:
            L.bn_dw_s2_bwd(dd, e, stats[0], stats[1], w0, b0, wdw, de, g[0], g[1], part, _empty(e, L.bn_dw_s2_ws(B, C, H, W, True)), eps0, B, C, H, W, k, pt, pl)
        else:
            L.bn_dw_s1_bwd(dd, e, stats[0], stats[1], w0, b0, wdw, de, g[0], g[1], part, _empty(e, L.bn_dw_s1_ws(B, C, H, W, True)), eps0, B, C, H, W, k, pt, pl)
        dwd = _empty(e, C * k * k)
        L.colsum(part, dwd, _empty(e, L.colreduce_ws(rows, C * k * k, 1)), rows, C * k * k)
        return de, g[0], g[1], None, None, None, None, dwd.view(wds), None, None, None


def bn_dw_s2_ok(e_shape, k, stride, pad):
    """does the op above serve an expanded tensor of this shape and a k x k depthwise convolution of this stride and padding (left, right, top, bottom)?"""
    if len(e_shape) != 4:
        return False
    B, C, H, W = (int(v) for v in e_shape)
    pl, pr, pt, pb = (int(p) for p in pad)
    if int(stride) != 2 or H % 2 or W % 2 or (H + pt + pb - k) // 2 + 1 != H // 2 or (W + pl + pr - k) // 2 + 1 != W // 2:
        return False
    return segx.lib().bn_dw_s2_ok(B, C, H, W, int(k), int(stride), pt, pl)


def bn_act_dwconv_s2(e, bn0, dw_weight, stride, static_pad):
    """dwconv2d(bn_act(e, bn0, swish), dw_weight, stride, static_pad) -- see _BNActDWConv.  bn0 is in training mode and bn_dw_s2_ok(e.shape, k, stride, static_pad)
    holds (the caller checks)."""
    assert int(stride) == 2
    _bn_tick(bn0)
    return _BNActDWConv.apply(e, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var, float(bn0.momentum), float(bn0.eps), dw_weight,
                              int(static_pad[2]), int(static_pad[0]), 2)


def bn_dw_s1_ok(e_shape, k, stride, pad):
    """the same for stride 1: symmetric 'same' padding (k - 1) / 2 on all four sides (left, right, top, bottom)"""
    if len(e_shape) != 4:
        return False
    B, C, H, W = (int(v) for v in e_shape)
    k = int(k)
    if int(stride) != 1 or k % 2 != 1 or tuple(int(p) for p in pad) != ((k - 1) // 2,) * 4:
        return False
    return segx.lib().bn_dw_s1_ok(B, C, H, W, k, 1, (k - 1) // 2, (k - 1) // 2)


def bn_act_dwconv_s1(e, bn0, dw_weight, stride, static_pad):
    """dwconv2d(bn_act(e, bn0, swish), dw_weight, 1, static_pad) -- see _BNActDWConv.  bn0 is in training mode and bn_dw_s1_ok(e.shape, k, stride, static_pad) holds (the
    caller checks)."""
    assert int(stride) == 1
    _bn_tick(bn0)
    return _BNActDWConv.apply(e, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var, float(bn0.momentum), float(bn0.eps), dw_weight,
                              int(static_pad[2]), int(static_pad[0]), 1)


def conv1x1_per_sample(x, Wb, bias=None):
    """Pointwise convolution with one weight matrix per sample: y[b] = Wb[b] x[b] (+ bias[b])  (Wb [B, Cout, Cin], bias [B, Cout]); one batched GEMM, A strided
    over the batch."""
    B, Cin = x.shape[0], x.shape[1]
    S = x.numel() // (B * Cin)
    Cout = Wb.shape[1]
    if bias is None:
        spec = GemmSpec(Cout, S, Cin, (Cout * Cin, 0, Cin, 1), (Cin * S, 0, 1, S), (Cout * S, 0, S), (B, Cout) + tuple(x.shape[2:]), nb=(B, 1))
        return bgemm(Wb, x, spec)
    spec = GemmSpec(Cout, S, Cin, (Cout * Cin, 0, Cin, 1), (Cin * S, 0, 1, S), (Cout * S, 0, S), (B, Cout) + tuple(x.shape[2:]), nb=(B, 1), bias_mode=BIAS_M, bias_b0=Cout)
    return bgemm(Wb, x, spec, bias=_c(bias))


def dwconv2d_bias_act_pool(x, w, bias, stride, pad, act=ACT_SWISH, pool=True):
    """Inference form of depthwise conv -> BatchNorm -> activation -> squeeze-excite pooling with the BatchNorm folded into w [C, 1, k, k] and bias [C]:
    y = act(dwconv2d(x, w) + bias) and the pooling partials of y from ONE pass (segx_dwconv2d_bias_act_pool).  -> (y, psum [B * C * nch] or None, nch);
    psum / nch are what segx_se_fwd2 takes (se_gate_weights).  Forward only.  pad = (left, right, top, bottom)."""
    if act not in (ACT_NONE, ACT_SWISH):
        raise NotImplementedError('dwconv2d_bias_act_pool: act is ACT_NONE or ACT_SWISH')
    _no_grad_operands('dwconv2d_bias_act_pool', x, w, bias)
    L = segx.lib()
    x, w = _c(x), _c(w)
    B, C, H, W = x.shape
    k, stride = w.shape[-1], int(stride)
    pl, pr, pt, pb = (int(v) for v in pad)
    OH, OW = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    y = _empty(x, B, C, OH, OW)
    nch = L.dwconv2d_pool_chunks(OH, OW) if pool else 0
    psum = _empty(x, B * C * nch) if pool else None
    L.dwconv2d_bias_act_pool(x, w, _c(bias), y, psum, B, C, H, W, OH, OW, k, stride, pt, pl, act)
    return y, psum, nch


def se_gate_weights(y, psum, nch, w1, b1, w2, b2, proj_weight):
    """Per-sample projection weights [B, Cout, C] = proj_weight * squeeze-excite gate, from the pooling partials of y (dwconv2d_bias_act_pool); forward only."""
    _no_grad_operands('se_gate_weights', psum, w1, b1, w2, b2, proj_weight)
    B, C = y.shape[0], y.shape[1]
    S = y.numel() // (B * C)
    return _se_excite(segx.lib(), y, psum, nch, S, w1, b1, w2, b2, _c(proj_weight.reshape(proj_weight.shape[0], C)))[5]


def conv1x1_per_sample_bias(x, Wb, bias, resid=None):
    """conv1x1_per_sample with ONE bias vector [Cout] for every sample and an optional skip input added in the GEMM's epilogue: y[b] = Wb[b] x[b] + bias (+ resid[b]).
    Forward only: the projection of an MBConv block with its BatchNorm folded (scale in Wb, shift = bias, efficientnet/model.py:113-122 in eval mode)."""
    _no_grad_operands('conv1x1_per_sample_bias', x, Wb, bias, resid)
    B, Cin = x.shape[0], x.shape[1]
    S = x.numel() // (B * Cin)
    Cout = Wb.shape[1]
    x, Wb = _c(x), _c(Wb)
    y = _empty(x, B, Cout, *x.shape[2:])
    kw = dict(resid=_c(resid)) if resid is not None else {}
    assert resid is None or resid.shape == y.shape
    _run_gemm(segx.lib(), Wb, x, y, Cout, S, Cin, (Cout * Cin, 0, Cin, 1), (Cin * S, 0, 1, S), (Cout * S, 0, S), (B, 1), 1.0, bias=_c(bias), bias_mode=BIAS_M, **kw)
    return y


def bn_act_se(x, bn, act, w1, b1, w2, b2):
    """squeeze_excite(bn_act(x, bn, act), w1, b1, w2, b2), fused (see _BNActSE)."""
    _bn_tick(bn)
    return _BNActSE.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum), float(bn.eps), act, w1, b1, w2, b2)


# -------------------------------------------------------------------------------------------------
# Feature-pyramid ops (fpn.hip): GroupNorm, linear resampling (+ fused lateral add)
# -------------------------------------------------------------------------------------------------
class _GroupNorm(_Fn):
    @staticmethod
    def forward(ctx, x, w, b, G, eps):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[:2]
        S = x.numel() // (B * C)
        y = torch.empty_like(x)
        mean, rstd = _empty(x, B * G), _empty(x, B * G)
        L.groupnorm_fwd(x, w, b, y, mean, rstd, _empty(x, L.gn_ws(B, C, G)), B, C, G, S, eps)
        ctx.cfg = (B, C, G, S)
        ctx.save_for_backward(x, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        x, w, mean, rstd = ctx.saved_tensors
        B, C, G, S = ctx.cfg
        dx = torch.empty_like(x)
        dw, db = _empty(x, C), _empty(x, C)
        L.groupnorm_bwd(_c(dy), x, w, mean, rstd, dx, dw, db, _empty(x, L.gn_ws(B, C, G)), B, C, G, S)
        return dx, dw, db, None, None


def group_norm(x, gn):
    """nn.GroupNorm module `gn` as parameter container."""
    return _GroupNorm.apply(x, gn.weight, gn.bias, int(gn.num_groups), float(gn.eps))


def _dhw(shape):
    sp = tuple(int(v) for v in shape)
    return (1,) + sp if len(sp) == 2 else sp


def _corner_scale(n_in, n_out):
    """src_scale argument of the one-axis resampling kernels for align_corners=True (negative = aligned corners, see segx.h)."""
    return -((n_in - 1) / (n_out - 1)) if n_out > 1 and n_in > 1 else -1e-6


class _InterpAdd(_Fn):
    @staticmethod
    def forward(ctx, x, base, size, align_corners=False):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[:2]
        d, h, w = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        base = _c(base) if base is not None else None
        axes = [(ax, n_in, n_out) for ax, (n_in, n_out) in enumerate(((d, D), (h, H), (w, W))) if n_in != n_out]
        ctx.align = bool(align_corners)
        if d != D and h != H and not align_corners and W % 4 == 0:
            # r04: the x pass (if any), then y AND z in ONE streaming pass with the lateral added (segx_interp_linear_fwd_axis2): 21 instead of 29
            # coarse-tensor sizes of traffic for a 2 x 2 x 2 up-sampling, the same blends in the same order
            cur = x
            if w != W:
                cur = _empty(x, B * C * d * h * W)
                L.interp_fwd_axis(x, None, cur, B * C * d * h, w, W, 1, 0.0)
            out = _empty(x, B, C, *size)
            L.interp_fwd_axis2(cur, base, out, B * C, d, D, h, H, W)
        elif (D > 1 or align_corners) and axes:
            # 3-D: one streaming pass per resized axis, innermost (smallest tensor) first, the lateral added in the last pass --
            # the same blends in the same order as the fused formula (bit-identical), at HBM rate instead of 1-2 TB/s
            cur, dims = x, [d, h, w]
            for k, (ax, n_in, n_out) in enumerate(sorted(axes, reverse=True)):
                outer = B * C
                for a in range(ax):
                    outer *= dims[a]
                inner = 1
                for a in range(ax + 1, 3):
                    inner *= dims[a]
                last = k == len(axes) - 1
                nxt = _empty(x, B, C, *size) if last else _empty(x, outer * n_out * inner)
                L.interp_fwd_axis(cur, base if last else None, nxt, outer, n_in, n_out, inner, _corner_scale(n_in, n_out) if align_corners else 0.0)
                cur, dims[ax] = nxt, n_out
            out = cur
        elif align_corners:                                    # nothing to resample: identity (+ base)
            out = x.clone() if base is None else x + base
        else:
            out = _empty(x, B, C, *size)
            L.interp_fwd(x, base, out, B * C, d, h, w, D, H, W)
        ctx.cfg = (B * C, d, h, w, D, H, W, tuple(x.shape))
        return out

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        planes, d, h, w, D, H, W, xshape = ctx.cfg
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0] and d != D and h != H and not ctx.align and W % 4 == 0:
            dx = _interp_bwd_yz_x(L, dy, planes, d, h, w, D, H, W).view(xshape)      # z and y adjoints in one pass, then x
        if ctx.needs_input_grad[0] and dx is None:
            # separable adjoint, one pass per resized axis, OUTERMOST axis first: the passes over the big tensors then have a long
            # contiguous inner extent (float4 kernel); the scalar innermost-axis pass runs last, on the smallest tensor
            cur, dims = dy, [D, H, W]
            for ax, n_in in ((0, d), (1, h), (2, w)):
                if dims[ax] == n_in:
                    continue
                outer = planes
                for a in range(ax):
                    outer *= dims[a]
                inner = 1
                for a in range(ax + 1, 3):
                    inner *= dims[a]
                nxt = _empty(dy, outer * n_in * inner)
                L.interp_bwd_axis(cur, nxt, outer, dims[ax], n_in, inner, _corner_scale(n_in, dims[ax]) if ctx.align else 0.0)
                cur, dims[ax] = nxt, n_in
            dx = cur.view(xshape) if cur is not dy else dy.clone().view(xshape)
        return dx, (dy if ctx.needs_input_grad[1] else None), None, None


class _UpGN(_Fn):
    """group_norm(interp_linear(x, size, base)) of a pyramid level (segtran3d.py:336-360: `out_gnNb(out_fpnMN_conv3d(cur) + up(feat))`) as ONE node:
    the y/z resampling pass that writes the level also leaves GroupNorm partials of it (segx_interp_linear_fwd_axis2_gn), so the statistics pass
    over the 2 - 3.5 GB tensor is gone; the backward's plane sums give the per-plane sums of the gradient it returns for `base` in closed form
    (segx_groupnorm_bwd plane_dx_sums), which the lateral convolution's bias gradient picks up (_bias_grad) instead of a row-sum pass.  Same blends in
    the same order as the unfused ops; the statistics differ by fp32 summation order only (Chan merge of per-workgroup partials)."""

    @staticmethod
    def forward(ctx, x, base, w, b, size, G, eps, nparts):
        L = segx.lib()
        x, base = _c(x), _c(base)
        B, C = x.shape[:2]
        d, h, wd = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        cur = x
        if wd != W:
            cur = _empty(x, B * C * d * h * W)
            L.interp_fwd_axis(x, None, cur, B * C * d * h, wd, W, 1, 0.0)
        pre = _empty(x, B, C, *size)
        parts = _empty(x, B * G * nparts * 4)
        L.interp_fwd_axis2_gn(cur, base, pre, B * C, d, D, h, H, W, C // G, parts, nparts)
        S = D * H * W
        y = torch.empty_like(pre)
        mean, rstd = _empty(x, B * G), _empty(x, B * G)
        L.groupnorm_fwd_parts(pre, parts, nparts, w, b, y, mean, rstd, B, C, G, S, eps)
        ctx.cfg = (B, C, G, S, d, h, wd, D, H, W, tuple(x.shape))
        ctx.save_for_backward(pre, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        pre, w, mean, rstd = ctx.saved_tensors
        B, C, G, S, d, h, wd, D, H, W, xshape = ctx.cfg
        dpre = torch.empty_like(pre)
        dw, db = _empty(pre, C), _empty(pre, C)
        rsum = _empty(pre, B * C)
        L.groupnorm_bwd(_c(dy), pre, w, mean, rstd, dpre, dw, db, _empty(pre, L.gn_ws(B, C, G)), B, C, G, S, rsum)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _interp_bwd_yz_x(L, dpre, B * C, d, h, wd, D, H, W).view(xshape)
        dbase = None
        if ctx.needs_input_grad[1]:
            dbase = dpre
            _tag_plane_sums(dbase, rsum, B, C, S)            # sum over every (sample, channel) plane of dbase: the lateral convolution's bias gradient (_bias_grad)
        return dx, dbase, dw, db, None, None, None, None


def _gn_fold_stat_grads(dsc, dsh, w, mean, rstd, B, C, G, S):
    """From the gradients of sc = rstd w and sh = b - mean sc ([B, C] each): GroupNorm's parameter gradients and the two per-(sample, group) coefficients of the
    statistics' share of the input gradient, dx += A + Bc * xhat  (d mean / d x = 1 / n;  d rstd / d x = -rstd^3 (x - mean) / n = -(rstd^2 / n) xhat)."""
    cpg = C // G
    n = float(cpg) * float(S)
    mn, rs, wg = mean.view(B, G, 1), rstd.view(B, G, 1), w.view(1, G, cpg)
    dscg, dshg = dsc.reshape(B, G, cpg), dsh.reshape(B, G, cpg)
    t = dscg - dshg * mn
    dw = (t * rs).sum(0).reshape(C)
    db = dsh.reshape(B, C).sum(0)
    dmean = -(dshg * (rs * wg)).sum(2)                        # [B, G]
    drstd = (t * wg).sum(2)
    A = (dmean / n).reshape(-1).contiguous()
    Bc = (-drstd * rstd.view(B, G) * rstd.view(B, G) / n).reshape(-1).contiguous()
    return dw, db, A, Bc


class _UpGNFold(_Fn):
    """The pyramid level `up(x) + base` with its GroupNorm statistics, for a GroupNorm that is FOLDED into its pointwise-convolution consumer (fpn.hip: r05
    "GroupNorm folded into its consumer"): returns (pre, sc, sh) with gn(pre) == pre * sc[b, c] + sh[b, c]; the normalised tensor is never written.  Backward
    takes the consumer's data gradient (which already carries sc) plus the gradients of sc and sh -- they come out of the consumer's per-sample weight / bias
    gradients, i.e. out of GEMMs that read `pre` anyway -- and needs ONE pass over the level (segx_gn_fold_bwd) instead of plane sums + apply."""

    @staticmethod
    def forward(ctx, x, base, w, b, size, G, eps, nparts):
        L = segx.lib()
        x, base = _c(x), _c(base)
        B, C = x.shape[:2]
        d, h, wd = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        cur = x
        if wd != W:
            cur = _empty(x, B * C * d * h * W)
            L.interp_fwd_axis(x, None, cur, B * C * d * h, wd, W, 1, 0.0)
        pre = _empty(x, B, C, *size)
        parts = _empty(x, B * G * nparts * 4)
        L.interp_fwd_axis2_gn(cur, base, pre, B * C, d, D, h, H, W, C // G, parts, nparts)
        mean, rstd = _empty(x, B * G), _empty(x, B * G)
        L.groupnorm_stats_parts(parts, nparts, mean, rstd, B * G, eps)
        cpg = C // G
        rs = rstd.view(B, G, 1).expand(B, G, cpg).reshape(B, C)
        mn = mean.view(B, G, 1).expand(B, G, cpg).reshape(B, C)
        sc = rs * w.view(1, C)
        sh = b.view(1, C) - mn * sc
        ctx.cfg = (B, C, G, D * H * W, d, h, wd, D, H, W, tuple(x.shape))
        ctx.save_for_backward(pre, w, mean, rstd)
        return pre, sc, sh

    @staticmethod
    def backward(ctx, dpre, dsc, dsh):
        L = segx.lib()
        pre, w, mean, rstd = ctx.saved_tensors
        B, C, G, S, d, h, wd, D, H, W, xshape = ctx.cfg
        dw, db, A, Bc = _gn_fold_stat_grads(dsc, dsh, w, mean, rstd, B, C, G, S)
        dtot = torch.empty_like(pre)
        rsum = _empty(pre, B * C)
        L.gn_fold_bwd(_c(dpre), pre, mean, rstd, A, Bc, dtot, rsum, _empty(pre, B * C * 64), B, C, G, S)
        dx = _interp_bwd_yz_x(L, dtot, B * C, d, h, wd, D, H, W).view(xshape) if ctx.needs_input_grad[0] else None
        dbase = None
        if ctx.needs_input_grad[1]:
            dbase = dtot
            _tag_plane_sums(dbase, rsum, B, C, S)             # plane sums of dbase: the lateral convolution's bias gradient (_bias_grad)
        return dx, dbase, dw, db, None, None, None, None


class _UpGNFoldProj(_Fn):
    """_UpGNFold + its consumer in ONE node, for a consumer that projects onto NC <= 8 channels (the class projection): out = (W * sc_b) pre + (W sh_b + bias).
    Backward never writes the consumer's full-size data gradient: segx_gn_fold_bwd_proj forms sum_o Wb[b, o, c] dOut[b, o, s] while it makes its one pass
    over the level (at cfg5 a 3.5-GB tensor the K = 4 GEMM took 0.86 ms to write and the pass 0.6 ms to read back)."""

    @staticmethod
    def forward(ctx, x, base, w, b, weight, bias, size, G, eps, nparts):
        L = segx.lib()
        x, base = _c(x), _c(base)
        B, C = x.shape[:2]
        d, h, wd = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        S = D * H * W
        cur = x
        if wd != W:
            cur = _empty(x, B * C * d * h * W)
            L.interp_fwd_axis(x, None, cur, B * C * d * h, wd, W, 1, 0.0)
        pre = _empty(x, B, C, *size)
        parts = _empty(x, B * G * nparts * 4)
        L.interp_fwd_axis2_gn(cur, base, pre, B * C, d, D, h, H, W, C // G, parts, nparts)
        mean, rstd = _empty(x, B * G), _empty(x, B * G)
        L.groupnorm_stats_parts(parts, nparts, mean, rstd, B * G, eps)
        cpg = C // G
        NC = weight.shape[0]
        W2 = _c(weight.reshape(NC, C))
        sc = rstd.view(B, G, 1).expand(B, G, cpg).reshape(B, C) * w.view(1, C)
        sh = b.view(1, C) - mean.view(B, G, 1).expand(B, G, cpg).reshape(B, C) * sc
        Wb = (W2.unsqueeze(0) * sc.unsqueeze(1)).contiguous()                        # [B, NC, C]
        bb = (sh.unsqueeze(1) * W2.unsqueeze(0)).sum(2)                              # [B, NC]
        if bias is not None:
            bb = bb + bias.view(1, NC)
        bb = bb.contiguous()
        out = _empty(x, B, NC, *size)
        _run_gemm(L, Wb, pre, out, NC, S, C, (NC * C, 0, C, 1), (C * S, 0, 1, S), (NC * S, 0, S), (B, 1), 1.0, bias=bb, bias_mode=BIAS_M, bias_b0=NC)
        ctx.cfg = (B, C, G, S, NC, d, h, wd, D, H, W, tuple(x.shape), tuple(weight.shape), bias is not None)
        ctx.save_for_backward(pre, w, mean, rstd, W2, Wb, sc, sh)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = segx.lib()
        pre, w, mean, rstd, W2, Wb, sc, sh = ctx.saved_tensors
        B, C, G, S, NC, d, h, wd, D, H, W, xshape, wshape, has_bias = ctx.cfg
        dout = _c(dout)
        dbb = _empty(pre, B * NC)
        L.rowsum(dout, dbb, B * NC, S)
        dbb = dbb.view(B, NC)
        dWb = _empty(pre, B, NC, C)                                                  # per-sample weight gradient: dOut[b] pre[b]^T (contraction over the voxels)
        _run_gemm(L, dout, pre, dWb, NC, C, S, (NC * S, 0, S, 1), (C * S, 0, S, 1), (NC * C, 0, C), (B, 1), 1.0)
        dsc = (dWb * W2.unsqueeze(0)).sum(1)                                         # [B, C]
        dsh = (dbb.unsqueeze(2) * W2.unsqueeze(0)).sum(1)
        dW2 = (dWb * sc.unsqueeze(1)).sum(0) + (dbb.unsqueeze(2) * sh.unsqueeze(1)).sum(0)
        dbias = dbb.sum(0) if has_bias else None
        dw, db, A, Bc = _gn_fold_stat_grads(dsc, dsh, w, mean, rstd, B, C, G, S)
        dtot = torch.empty_like(pre)
        rsum = _empty(pre, B * C)
        L.gn_fold_bwd_proj(dout, Wb, NC, pre, mean, rstd, A, Bc, dtot, rsum, _empty(pre, B * C * 64), B, C, G, S)
        dx = _interp_bwd_yz_x(L, dtot, B * C, d, h, wd, D, H, W).view(xshape) if ctx.needs_input_grad[0] else None
        dbase = None
        if ctx.needs_input_grad[1]:
            dbase = dtot
            _tag_plane_sums(dbase, rsum, B, C, S)
        return dx, dbase, dw, db, dW2.view(wshape), dbias, None, None, None, None


def up_group_norm_conv(x, size, base, gn, weight, bias=None):
    """conv1x1(gn(F.interpolate(x, size, mode='trilinear') + base), weight, bias) with the GroupNorm folded into per-sample weights and biases (_UpGNFold):
    the level is written once (by the resampling pass, which also leaves the statistics) and read once (by the convolution); backward adds one pass.
    Shapes the fused resampling pass does not serve take up_group_norm + conv1x1."""
    size = tuple(int(s) for s in size)
    G = int(gn.num_groups)
    if base is not None and x.dim() in (4, 5) and fold_group_norm:      # 2-D maps: depth 1, the y pass alone carries the statistics
        d, h, _ = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        B, C = x.shape[0], x.shape[1]
        if h != H and W % 4 == 0 and C % G == 0 and tuple(base.shape) == (B, C) + size:
            nparts = segx.lib().interp_gn_nparts(D * H * (W // 4), C // G)
            if nparts > 0:
                Cout = weight.shape[0]
                if Cout <= 8:                                      # a projection onto a few channels: the whole level + consumer as one node (no full-size data gradient)
                    return _UpGNFoldProj.apply(x, base, gn.weight, gn.bias, weight, bias, size, G, float(gn.eps), nparts)
                pre, sc, sh = _UpGNFold.apply(x, base, gn.weight, gn.bias, size, G, float(gn.eps), nparts)
                W2 = weight.reshape(Cout, C)
                Wb = W2.unsqueeze(0) * sc.unsqueeze(1)            # [B, Cout, C]
                bb = linear(sh, W2, bias)                          # [B, Cout] = sh W^T + bias (libsegx GEMM: no vendor BLAS on the step)
                return conv1x1_per_sample(pre, Wb, bias=bb)
    return conv1x1(up_group_norm(x, size, base, gn), weight, bias)


fold_group_norm = True          # False: GroupNorm applied by its own pass (up_group_norm) -- A/B switch of tests and tools


def _interp_bwd_yz_x(L, dy, planes, d, h, w, D, H, W):
    """adjoint of the x pass + fused y/z pass: z and y in one pass, then x (13 instead of 21 coarse-tensor sizes); d == D: the y adjoint alone"""
    cur = _empty(dy, planes * d * h * W)
    if d == D:
        L.interp_bwd_axis(dy, cur, planes * D, H, h, W, 0.0)
    else:
        L.interp_bwd_axis2(dy, cur, planes, D, d, H, h, W)
    if w != W:
        nxt = _empty(dy, planes * d * h * w)
        L.interp_bwd_axis(cur, nxt, planes * d * h, W, w, 1, 0.0)
        cur = nxt
    return cur


def up_group_norm(x, size, base, gn):
    """gn(F.interpolate(x, size, mode='trilinear') + base): the fused node where the level is up-sampled along both outer axes, W % 4 == 0 and the plane
    splits into whole 1024-float chunks; the two plain ops otherwise (2-D maps, odd sizes)."""
    size = tuple(int(s) for s in size)
    G = int(gn.num_groups)
    if base is not None and x.dim() == 5:
        d, h, _ = _dhw(x.shape[2:])
        D, H, W = _dhw(size)
        C = x.shape[1]
        if h != H and W % 4 == 0 and C % G == 0 and tuple(base.shape) == (x.shape[0], C) + size:        # y resized (z too, or not: the 64 x 32 x 32 -> 64^3 level)
            nparts = segx.lib().interp_gn_nparts(D * H * (W // 4), C // G)
            if nparts > 0:
                return _UpGN.apply(x, base, gn.weight, gn.bias, size, G, float(gn.eps), nparts)
    return group_norm(interp_linear(x, size, base), gn)


def interp_linear(x, size, base=None, align_corners=False):
    """F.interpolate(x, size, mode='bilinear'/'trilinear', align_corners=...) (+ base): NC[D]HW in, NC[D']H'W' out."""
    return _InterpAdd.apply(x, base, tuple(int(s) for s in size), align_corners)


class _InterpTokens(_Fn):
    """Linear resampling of a token grid kept channels-last, [B, prod(in_shape), C] -> [B, prod(out_shape), C]: one streaming pass
    per resized axis (innermost first = ATen's blend order), the channels riding along as the contiguous inner extent."""

    @staticmethod
    def forward(ctx, x, in_shape, out_shape, src_scale):
        L = segx.lib()
        x = _c(x)
        B, U, C = x.shape
        assert U == math.prod(in_shape) and len(in_shape) == len(out_shape)
        cur, dims = x, list(in_shape)
        for ax in reversed(range(len(dims))):
            if dims[ax] == out_shape[ax]:
                continue
            outer = B * math.prod(dims[:ax])
            inner = C * math.prod(dims[ax + 1:])
            nxt = _empty(x, outer * out_shape[ax] * inner)
            L.interp_fwd_axis(cur, None, nxt, outer, dims[ax], out_shape[ax], inner, src_scale)
            cur, dims[ax] = nxt, out_shape[ax]
        ctx.cfg = (B, C, tuple(in_shape), tuple(out_shape), src_scale)
        return cur.view(B, -1, C) if cur is not x else x.clone()

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        B, C, in_shape, out_shape, src_scale = ctx.cfg
        cur, dims = _c(dy), list(out_shape)
        for ax in range(len(dims)):                       # adjoint passes in the reverse order of the forward ones
            if dims[ax] == in_shape[ax]:
                continue
            outer = B * math.prod(dims[:ax])
            inner = C * math.prod(dims[ax + 1:])
            nxt = _empty(dy, outer * in_shape[ax] * inner)
            L.interp_bwd_axis(cur, nxt, outer, dims[ax], in_shape[ax], inner, src_scale)
            cur, dims[ax] = nxt, in_shape[ax]
        return cur.view(B, -1, C), None, None, None


def interp_tokens(x, in_shape, out_shape=None, scale_factor=None):
    """reference resize_flat_features (segtran_shared.py:47-66) on channels-last tokens [B, N, C].  Either `out_shape` (the
    size= form: source step n_in/n_out) or `scale_factor` (output floor(n*sf), source step float(1/sf) -- ATen keeps the given
    factor for the coordinates)."""
    in_shape = tuple(int(v) for v in in_shape)
    if scale_factor is not None:
        out_shape = tuple(int(math.floor(v * scale_factor)) for v in in_shape)
        src_scale = 1.0 / scale_factor          # rounded to fp32 at the C boundary, as ATen's static_cast<float>(1.0 / scale)
    else:
        out_shape, src_scale = tuple(int(v) for v in out_shape), 0.0
    if out_shape == in_shape:
        return x
    return _InterpTokens.apply(x, in_shape, out_shape, src_scale)


# -------------------------------------------------------------------------------------------------
# I3D spatial convolutions (implicit GEMM on the MFMA engine) and TF-'same' max-pool (conv3d.hip)
# -------------------------------------------------------------------------------------------------
def _same_pads(size, k, s):
    """aj_i3d.py:68-90 -- dynamic TF-'same' padding: (front, back) per axis."""
    out = []
    for n, kk, ss in zip(size, k, s):
        tot = max(kk - ss, 0) if n % ss == 0 else max(kk - (n % ss), 0)
        out.append((tot // 2, tot - tot // 2))
    return out


def _conv3d_fwd_shaped(L, x, w, y, B, Cout, geom, mode, x_bs=0, y_bs=0, halo=True):
    """y = the convolution of geometry `geom` over x with the layer's filters w as they are (mode 0: the forward pass) or transposed and flipped (mode 1: the stride-1
    data gradient, Cout = the layer's Cin).  The LDS-resident-halo kernel where it serves (3 x 3 x 3 stride-1 'same', conv3d_halo.hip; filters pre-split once per call),
    else the implicit GEMM: split-K workspace, filters packed where the contracted channels come in eights (one tap decode per eight gathers, conv3d.hip).
    x_bs / y_bs: sample strides of channel slices (0 = dense)."""
    C, KV = geom[0], geom[7] * geom[8] * geom[9]
    if halo and L.conv3d_halo_ok(B, Cout, geom):
        L.conv3d_halo_fwd(x, L.conv3d_halo_pack(w, Cout, C, mode), y, B, Cout, geom, x_bs=x_bs, y_bs=y_bs)
        return
    sk = L.conv3d_splitk(B, Cout, geom, False)
    ws = _empty(x, sk * B * Cout * geom[4] * geom[5] * geom[6]) if sk > 1 else None
    packed = C % 8 == 0
    if packed or mode:
        wp = torch.empty_like(w)
        if packed:
            L.conv3d_pack_weights(w, wp, Cout, C, KV, mode)
        else:
            L.conv3d_flip_weights(w, wp, C, Cout, KV)
        w = wp
    L.conv3d_fwd(x, w, y, B, Cout, geom, sk, ws, packed=packed, x_bs=x_bs, y_bs=y_bs)


def _conv3d_dgrad_strided(L, dy, w, dx, B, geom):
    """dx of a strided convolution of geometry `geom`."""
    Cin, ID, IH, IW, OD, OH, OW, KD, KH, KW, sd, sh, sw, pd, ph, pw = geom
    Cout = w.shape[0]
    if Cin <= 4:
        # strided transposed convolution onto <= 4 channels (the 7x7x7 stride-2 I3D stem): direct gather kernel
        L.conv3d_bwd_data_direct(dy, w, dx, B, Cout, geom)
        return
    # general strided case (the 4x4 stride-2 convolutions of the domain discriminator): dY with stride-1 zeros inserted, then the stride-1 transposed
    # convolution on the tile engine (positions beyond the dilated extent read the zero padding); always the implicit GEMM
    DD, DH, DW = (OD - 1) * sd + 1, (OH - 1) * sh + 1, (OW - 1) * sw + 1
    dyd = dy.new_zeros(B, Cout, DD, DH, DW)
    dyd[:, :, ::sd, ::sh, ::sw] = dy
    g2 = (Cout, DD, DH, DW, ID, IH, IW, KD, KH, KW, 1, 1, 1, KD - 1 - pd, KH - 1 - ph, KW - 1 - pw)
    _conv3d_fwd_shaped(L, dyd, w, dx, B, Cin, g2, 1, halo=False)


def _conv3d_wgrad(L, dy, x, w, B, geom, x_bs=0):
    """dw of the convolution of geometry `geom` (x: possibly a channel slice with sample stride x_bs): the halo kernel where it serves, else per-sample rows on the
    implicit GEMM (packed row order where Cin comes in eights), their sum over the batch, and the layer's [Cout][Cin][KV] order restored."""
    Cout, Cin = w.shape[:2]
    KV = geom[7] * geom[8] * geom[9]
    N = Cin * KV
    if L.conv3d_halo_wgrad_ok(B, Cout, geom):
        dw = torch.empty_like(w)
        L.conv3d_halo_wgrad(dy, x, dw, B, Cout, geom, x_bs=x_bs)
        return dw
    sk = L.conv3d_splitk(B, Cout, geom, True)
    ws = _empty(dy, sk * B * Cout * N) if sk > 1 else None
    dwb = _empty(dy, B, Cout * N)
    packed = Cin % 8 == 0
    L.conv3d_bwd_weight(dy, x, dwb, B, Cout, geom, sk, ws, packed=packed, x_bs=x_bs)
    dw = dwb
    if B > 1:
        dw = _empty(dy, Cout * N)
        L.colsum(dwb, dw, _empty(dy, L.colreduce_ws(B, Cout * N, 1)), B, Cout * N)
    if packed:
        dwp, dw = dw, _empty(dy, Cout * N)
        L.conv3d_unpack_wgrad(dwp, dw, Cout, Cin, KV)
    return dw.view_as(w)


class _Conv3d(_Fn):
    @staticmethod
    def forward(ctx, x, w, stride, pads):
        L = segx.lib()
        x, w = _c(x), _c(w)
        B, Cin, ID, IH, IW = x.shape
        Cout, _, KD, KH, KW = w.shape
        (pd, pdb), (ph, phb), (pw, pwb) = pads
        OD = (ID + pd + pdb - KD) // stride[0] + 1
        OH = (IH + ph + phb - KH) // stride[1] + 1
        OW = (IW + pw + pwb - KW) // stride[2] + 1
        y = _empty(x, B, Cout, OD, OH, OW)
        ctx.geom = (Cin, ID, IH, IW, OD, OH, OW, KD, KH, KW) + tuple(stride) + (pd, ph, pw)
        _conv3d_fwd_shaped(L, x, w, y, B, Cout, ctx.geom, 0)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        x, w = ctx.saved_tensors
        dy = _c(dy)
        Cin, ID, IH, IW, OD, OH, OW, KD, KH, KW, sd, sh, sw, pd, ph, pw = geom = ctx.geom
        B, Cout = x.shape[0], w.shape[0]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if (sd, sh, sw) == (1, 1, 1):
                g2 = (Cout, OD, OH, OW, ID, IH, IW, KD, KH, KW, 1, 1, 1, KD - 1 - pd, KH - 1 - ph, KW - 1 - pw)
                _conv3d_fwd_shaped(L, dy, w, dx, B, Cin, g2, 1)
            else:
                _conv3d_dgrad_strided(L, dy, w, dx, B, geom)
        if ctx.needs_input_grad[1]:
            dw = _conv3d_wgrad(L, dy, x, w, B, geom)
        return dx, dw, None, None


class _Conv3dSlices(_Fn):
    """Stride-1 'same' convolutions over DISJOINT channel slices of one NCDHW tensor t (slice i = the next w_i.shape[1] channels), without copying
    the slices out: the implicit-GEMM kernels take the slice pointer and t's sample stride (segx_conv3d_*_bs), and in backward each transposed
    convolution writes its slice of ONE gradient tensor (every element written exactly once: no zero fill, no gradient adds).  Used by the
    Inception module whose two 1x1x1 reductions run as one convolution + one BatchNorm (aj_i3d.py:112-141)."""

    @staticmethod
    def forward(ctx, t, with_tail, *ws):
        L = segx.lib()
        t = _c(t)
        ctx.with_tail = bool(with_tail)
        B, Ct, D, H, W = t.shape
        ys, geoms, c0 = [], [], 0
        for w in ws:
            w = _c(w)
            Cout, Cin, KD, KH, KW = w.shape
            assert Cin % 8 == 0 and Cout % 8 == 0 and KD % 2 == KH % 2 == KW % 2 == 1, 'slice convolutions: channel counts in multiples of 8, odd windows'
            geom = (Cin, D, H, W, D, H, W, KD, KH, KW, 1, 1, 1, KD // 2, KH // 2, KW // 2)
            y = _empty(t, B, Cout, D, H, W)
            _conv3d_fwd_shaped(L, t[:, c0:], w, y, B, Cout, geom, 0, x_bs=Ct * D * H * W)
            ys.append(y); geoms.append(geom); c0 += Cin
        assert c0 <= Ct, 'the slices exceed the tensor'      # channels beyond the last slice (another consumer's, e.g. Inception branch 0)
        ctx.geoms = geoms
        ctx.save_for_backward(t, *ws)
        ctx.set_materialize_grads(False)
        if ctx.with_tail:
            # the channels no convolution reads leave as one more output (a view): their consumer's gradient comes back to THIS node and is written into
            # the tail of dt -- instead of a zero fill here plus autograd's slice-backward (zeros + copy) and a full-size accumulation add
            return tuple(ys) + (t[:, c0:],)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        L = segx.lib()
        t, ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        B, Ct, D, H, W = t.shape
        t_bs = Ct * D * H * W
        dt = torch.empty_like(t) if ctx.needs_input_grad[0] else None
        covered = sum(int(w.shape[1]) for w in ws)
        d_tail = dys[len(ws)] if ctx.with_tail else None
        if dt is not None and covered < Ct:
            if d_tail is not None:
                dt[:, covered:].copy_(d_tail)
            else:
                dt[:, covered:].zero_()
        dws, c0 = [], 0
        for i, (w, dy, geom) in enumerate(zip(ws, dys, ctx.geoms)):
            Cout, Cin = w.shape[:2]
            dy = _c(dy) if dy is not None else torch.zeros(B, Cout, D, H, W, dtype=torch.float32, device=t.device)
            if dt is not None:
                _conv3d_fwd_shaped(L, dy, w, dt[:, c0:], B, Cin, (Cout,) + geom[1:], 1, y_bs=t_bs)
            dws.append(_conv3d_wgrad(L, dy, t[:, c0:], w, B, geom, x_bs=t_bs) if ctx.needs_input_grad[2 + i] else None)
            c0 += Cin
        return (dt, None) + tuple(dws)


def conv3d_slices(t, *weights, with_tail=False):
    """(conv3d_same(t[:, :c1], w1), conv3d_same(t[:, c1:c1+c2], w2), ...) for stride-1 odd-window convolutions, reading the slices in place.
    with_tail: one more output, the channels behind the last slice (a view of t) -- route their consumer through it and its gradient is written
    into t's gradient by this node (no zero fill, no slice-backward copy, no accumulation add)."""
    return _Conv3dSlices.apply(t, with_tail, *weights)


def conv3d_same(x, w, stride=(1, 1, 1)):
    """nn.Conv3d(bias=False) with the dynamic TF-'same' zero padding of Unit3D (aj_i3d.py:75-92)."""
    stride = tuple(int(s) for s in stride)
    return _Conv3d.apply(x, w, stride, _same_pads(x.shape[2:], w.shape[2:], stride))


def conv3d_bias_relu(x, w, bias, stride=(1, 1, 1), pads=None, out=None, ops=None):
    """relu(conv3d(x, w) + bias) with the dynamic 'same' padding of conv3d_same (or the given (front, back) pads per axis) -- forward only: a convolution whose BatchNorm
    was folded into w and bias.  The LDS-resident-halo kernel where it serves (bias and ReLU in its store loop), else the implicit GEMM (epilogue; split-K: the slab
    reduction).  x / out: dense, or channel slices of wider NCDHW tensors read / written in place (_chan_slice_bs; otherwise through a copy).
    ops: a dict the caller keeps per layer -- the derived filter banks ('halo': segx_conv3d_halo_pack, 'packed': segx_conv3d_pack_weights) are built on first use and
    reused while the caller keeps it (the fold's per-layer operand cache): no pack launch after the first call.
    bias = None: the plain convolution on the cached bank (the folded space-to-depth stem, whose bias is a map: stem_bridge_conv_s2d_folded)."""
    _no_grad_operands('conv3d_bias_relu', x, w, bias, out)
    L = segx.lib()
    stride = tuple(int(v) for v in stride)
    B, Cin, ID, IH, IW = x.shape
    Cout, Cw, KD, KH, KW = w.shape
    assert Cw == Cin and (bias is None or bias.numel() == Cout)
    (pd, pdb), (ph, phb), (pw, pwb) = pads if pads is not None else _same_pads(x.shape[2:], w.shape[2:], stride)
    OD, OH, OW = (ID + pd + pdb - KD) // stride[0] + 1, (IH + ph + phb - KH) // stride[1] + 1, (IW + pw + pwb - KW) // stride[2] + 1
    geom = (Cin, ID, IH, IW, OD, OH, OW, KD, KH, KW) + stride + (pd, ph, pw)
    x_bs = _chan_slice_bs(x)
    if x_bs is None:
        x, x_bs = x.contiguous() if not x.is_contiguous() else x.clone(), 0
    if out is None:
        out = _empty(x, B, Cout, OD, OH, OW)
    assert tuple(out.shape) == (B, Cout, OD, OH, OW)
    y_bs = _chan_slice_bs(out)
    y = out if y_bs is not None else _empty(x, B, Cout, OD, OH, OW)
    y_bs = y_bs or 0
    ops = ops if ops is not None else {}
    w = _c(w)
    if Cin % 8 and (x_bs or y_bs):                              # unpacked filters (no layer of I3D behind its stem): the kernels take dense operands only
        if x_bs:
            x, x_bs = x.contiguous(), 0
        if y_bs:
            y, y_bs = _empty(x, B, Cout, OD, OH, OW), 0
    if bias is not None and L.conv3d_halo_ok(B, Cout, geom):
        wq = ops.get('halo')
        if wq is None:
            wq = ops['halo'] = L.conv3d_halo_pack(w, Cout, Cin, 0)
        L.conv3d_halo_bias_act_fwd(x, wq, bias, y, B, Cout, geom, x_bs=x_bs, y_bs=y_bs, act=ACT_RELU)
    else:
        sk = L.conv3d_splitk(B, Cout, geom, False)
        ws = _empty(x, sk * B * Cout * OD * OH * OW) if sk > 1 else None
        packed = Cin % 8 == 0
        if packed:
            wp = ops.get('packed')
            if wp is None:
                wp = torch.empty_like(w)
                L.conv3d_pack_weights(w, wp, Cout, Cin, KD * KH * KW, 0)
                ops['packed'] = wp
            w = wp
        if bias is None:
            assert packed or not (x_bs or y_bs)
            L.conv3d_fwd(x, w, y, B, Cout, geom, sk, ws, packed=packed, x_bs=x_bs, y_bs=y_bs)
        else:
            L.conv3d_fwd_bias_act(x, w, bias, y, B, Cout, geom, sk, ws, packed=packed, x_bs=x_bs, y_bs=y_bs, act=ACT_RELU)
    if y is not out:
        out.copy_(y)
    return out


def stem_s2d_folded_operands(stem_weight, bridge_weight, bridge_bias, bias):
    """The constants of stem_bridge_conv_s2d for a stem whose BatchNorm was folded in (stem_weight = w', bias = b'): the space-to-depth filters w2 [O, 8, 7, 7, 4] and
    the bias seen through each tap v [O, 7, 7, 7] -- the same contractions, over tensors of <= 64 x 343 x 3 x 4 numbers, in fp64 (as the fold itself), rounded once."""
    O, C3, KD, KH, KW = stem_weight.shape
    Cb = bridge_weight.shape[1]
    with torch.no_grad():
        taps = stem_weight.double().permute(0, 2, 3, 4, 1)                                            # [O, kd, kh, kw, c3]
        wc = (taps.unsqueeze(-1) * bridge_weight.double().reshape(C3, Cb)).sum(4).permute(0, 4, 1, 2, 3)   # [O, Cb, 7, 7, 7]
        w2 = F.pad(wc, (0, 1)).view(O, Cb, KD, KH, 4, 2).permute(0, 1, 5, 2, 3, 4).reshape(O, 2 * Cb, KD, KH, 4).float().contiguous()
        v = (taps * bridge_bias.double()).sum(4)                                                      # [O, 7, 7, 7]
    return w2, v, bias


def stem_s2d_bias_map(v, bias, D, H, W):
    """[O, OD, OH, OW] (fp32): the bridge's bias through the taps the zero padding leaves on (stem_bridge_conv_s2d's bias map) + bias[o]; depends on the input extent only"""
    with torch.no_grad():
        md, mh, mw = (_stem_axis_mask(n, 7, 2, 2, v.device).double() for n in (D, H, W))
        m = sum(v[:, t, None] * md[:, t].view(1, -1, 1, 1) for t in range(7))                        # [O, OD, kh, kw]
        m = sum(m[:, :, u, None] * mh[:, u].view(1, 1, -1, 1) for u in range(7))                     # [O, OD, OH, kw]
        m = sum(m[:, :, :, w, None] * mw[:, w].view(1, 1, 1, -1) for w in range(7))                  # [O, OD, OH, OW]
        return (m + bias.double().view(-1, 1, 1, 1)).float().contiguous()


def stem_bridge_conv_s2d_folded(batch, w2, bias_map, ops=None):
    """relu(stem_bridge_conv_s2d(...) folded with the stem's BatchNorm): the space-to-depth input, the stride-(2, 2, 1) convolution with the folded filters, and ONE pass
    y = relu(y + bias_map) (segx_bias_map_relu) -- no linear chain, no ATen add, no BatchNorm launch.  Forward only."""
    _no_grad_operands('stem_bridge_conv_s2d_folded', batch, w2, bias_map)
    L = segx.lib()
    B, Cb, H, W, D = batch.shape
    U = W // 2 + 3
    x2 = _empty(batch, B, 2 * Cb, D, H, U)
    L.stem_s2d_input(_c(batch), x2, B, Cb, H, W, D, U)
    y = conv3d_bias_relu(x2, w2, None, (2, 2, 1), ((2, 3), (2, 3), (0, 0)), ops=ops)        # (bias = None: the plain convolution on the cached packed bank)
    assert tuple(y.shape[1:]) == tuple(bias_map.shape)
    L.bias_map_relu(y, bias_map, B, bias_map.numel())
    return y


class _StemCompose(_Fn):
    """Wc [O, Cc, *k] = stem filters [O, C3, *k] composed with the input bridge (weight [C3, Cb, 1, 1, 1], bias [C3]); see segx_stem_compose_fwd."""

    @staticmethod
    def forward(ctx, ws, wb, bb, Cc):
        L = segx.lib()
        ws, wb = _c(ws), _c(wb)
        O, C3 = ws.shape[:2]
        T = ws[0, 0].numel()
        Cb = wb.shape[1]
        wc = _empty(ws, O, Cc, *ws.shape[2:])
        L.stem_compose_fwd(ws, wb, bb, wc, O, C3, Cb, Cc, T)
        ctx.dims = (O, C3, Cb, Cc, T)
        ctx.save_for_backward(ws, wb, bb)
        return wc

    @staticmethod
    def backward(ctx, dwc):
        L = segx.lib()
        ws, wb, bb = ctx.saved_tensors
        O, C3, Cb, Cc, T = ctx.dims
        dws, dwb = torch.empty_like(ws), torch.empty_like(wb)
        dbb = torch.empty_like(bb) if bb is not None else None
        L.stem_compose_bwd(_c(dwc), ws, wb, bb, dws, dwb, dbb, O, C3, Cb, Cc, T)
        return dws, dwb, dbb, None


def stem_compose(stem_weight, bridge_weight, bridge_bias, Cc=8):
    return _StemCompose.apply(stem_weight, bridge_weight, bridge_bias, int(Cc))


_stem_masks = {}


def _stem_axis_mask(n_in, k, stride, pad_front, device):
    """[n_out, k] 0/1: tap k of output o reads input stride * o + k - pad_front inside [0, n_in) -- the taps the zero padding does NOT switch off"""
    key = (n_in, k, stride, pad_front, str(device))
    m = _stem_masks.get(key)
    if m is None:
        n_out = (n_in + stride - 1) // stride
        i = torch.arange(n_out).view(-1, 1) * stride + torch.arange(k).view(1, -1) - pad_front
        m = ((i >= 0) & (i < n_in)).float().to(device)
        _stem_masks[key] = m
    return m


def stem_bridge_conv_s2d(batch, stem_weight, bridge_weight, bridge_bias, stride=(2, 2, 2)):
    """Conv3d_1a_7x7(in_bridge_to3(batch)) (segtran3d.py:420-423 + aj_i3d.py:75-97: a 1x1x1 convolution with bias onto 3 channels, then the 7 x 7 x 7 stride-2
    'same' stem) for the raw batch [B, Cb, H, W, D] (2 Cb = 8) as ONE stride-(2, 2, 1) convolution with a 7 x 7 x 4 window over a SPACE-TO-DEPTH image along W:
        x2[b][2 c + j][d][h][u] = x[b][c][d][h][2 u + j - 2]          (u = ow + kw', tap kw = 2 kw' + j; zero outside the volume)
        w2[o][2 c + j][kd][kh][kw'] = sum_c3 Ws[o][c3][kd][kh][2 kw' + j] Wb[c3][c]      (kw = 7 does not exist: zero)
    plus the bridge's bias as a bias MAP: sum over the taps the zero padding leaves on of V[o][tap] = sum_c3 Ws[o][c3][tap] bb[c3] -- 4 x 4 x 4 border classes of
    output positions, contracted axis by axis with 0/1 masks.  Exactly the products of the composed 8-channel form of r02 (SF.stem_compose: [x, 1, 0, 0, 0] -> 64)
    in another order, without its three all-zero channels and its constant channel: K = 8 * 196 = 1568 instead of 8 * 343 = 2744 (-43 % of the stem's FLOPs),
    unit stride along W -- 16-byte row loads in the weight-gradient loader, which therefore runs on the bf16x6 engine (the stride-2 form stayed on the fp32
    engine at 81 TFLOP/s) -- and every parameter gradient through autograd's chain rule over the small tensors (SF.linear / pad / permute of <= 64 x 8 x 343 floats)."""
    B, Cb, H, W, D = batch.shape
    O, C3, KD, KH, KW = stem_weight.shape
    assert tuple(stride) == (2, 2, 2) and (KD, KH, KW) == (7, 7, 7) and 2 * Cb == 8 and W % 2 == 0 and H % 2 == 0 and D % 2 == 0
    # the small contractions run on the tile engine too (SF.linear: differentiable, no vendor GEMM on the step -- torch.einsum would hand them to hipBLASLt)
    taps = stem_weight.permute(0, 2, 3, 4, 1).reshape(O * KD * KH * KW, C3)                # [(o, kd, kh, kw), c3]
    wc = linear(taps, bridge_weight.reshape(C3, Cb).t()).view(O, KD, KH, KW, Cb).permute(0, 4, 1, 2, 3)   # [O, Cb, 7, 7, 7] = sum_c3 Ws[o][c3][tap] Wb[c3][c]
    w2 = F.pad(wc, (0, 1)).view(O, Cb, KD, KH, 4, 2).permute(0, 1, 5, 2, 3, 4).reshape(O, 2 * Cb, KD, KH, 4).contiguous()
    # conv axes (D, H, W) = (batch's last axis, H, W): [B, Cb, D, H, W] padded along W by 2 in front (the 'same' front pad) and 4 behind (window end), then W -> (U, 2)
    U = W // 2 + 3
    x2 = _empty(batch, B, 2 * Cb, D, H, U)
    segx.lib().stem_s2d_input(_c(batch.detach()), x2, B, Cb, H, W, D, U)      # one pass (pad + permute + reshape: three ATen copies of the batch)
    y = _Conv3d.apply(x2, w2, (2, 2, 1), ((2, 3), (2, 3), (0, 0)))
    v = linear(taps, bridge_bias.view(1, C3)).view(O, KD, KH, KW)                           # the bias seen through each tap
    md, mh, mw = (_stem_axis_mask(n, 7, 2, 2, batch.device) for n in (D, H, W))
    # bias_map[o][d][h][w] = sum_{t,u,v} v[o][t][u][v] md[d][t] mh[h][u] mw[w][v], one axis at a time (the contracted axis moved last, the W axis contracted last so
    # that the result lands in [O, OD, OH, OW] order): only a shell of three voxels differs from the interior value
    s = linear(v.permute(0, 2, 3, 1), md)                                                   # [O, kh, kw, OD]
    s = linear(s.permute(0, 3, 2, 1), mh)                                                   # [O, OD, kw, OH]
    bias_map = linear(s.permute(0, 1, 3, 2), mw)                                            # [O, OD, OH, OW]
    return y + bias_map.unsqueeze(0)


def bridge_input(x, Cc=8):
    """[B, Cb, H, W, D] -> [B, Cc, D, H, W] with a constant-one channel at index Cb and zeros above it (no gradient: network input)."""
    L = segx.lib()
    x = _c(x.detach())
    B, Cb, H, W, D = x.shape
    y = _empty(x, B, Cc, D, H, W)
    L.bridge_input(x, y, B, Cb, Cc, H, W, D)
    return y


class _MaxPool3d(_Fn):
    """pass_input: also return the input as a second output (an alias).  Where the pooled tensor has other consumers -- the I3D endpoints feats[1..3] feed the next
    backbone stage through a strided pool AND the feature pyramid (segtran3d.py:436-441) -- they read the alias: autograd then hands their summed gradient to THIS
    node, and the pool's backward kernel adds it while it writes dX (segx_maxpool3d_bwd addend) instead of autograd running an accumulation kernel over two
    full-size tensors (0.68 ms of the cfg5 step)."""

    @staticmethod
    def forward(ctx, x, kernel, stride, pads, pass_input=False):
        L = segx.lib()
        x = _c(x)
        B, C, ID, IH, IW = x.shape
        (pd, pdb), (ph, phb), (pw, pwb) = pads
        OD = (ID + pd + pdb - kernel[0]) // stride[0] + 1
        OH = (IH + ph + phb - kernel[1]) // stride[1] + 1
        OW = (IW + pw + pwb - kernel[2]) // stride[2] + 1
        y = _empty(x, B, C, OD, OH, OW)
        arg = torch.empty(B, C, OD, OH, OW, dtype=torch.int32, device=x.device)
        geom = (ID, IH, IW, OD, OH, OW) + tuple(kernel) + tuple(stride) + (pd, ph, pw)
        L.maxpool3d_fwd(x, y, arg, B * C, geom)
        ctx.geom, ctx.xshape = geom, tuple(x.shape)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(arg)
        if pass_input:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dalias=None):
        L = segx.lib()
        (arg,) = ctx.saved_tensors
        if dy is None:                                           # only the alias was used
            return dalias, None, None, None, None
        dx = _empty(dy, *ctx.xshape)
        addend = None
        if dalias is not None:
            addend = _c(dalias)
            if tuple(ctx.geom[9:12]) == (1, 1, 1) or addend.data_ptr() % 16:      # the stride-1 kernels take no addend
                addend = None
        L.maxpool3d_bwd(_c(dy), arg, dx, ctx.xshape[0] * ctx.xshape[1], ctx.geom, addend)
        if dalias is not None and addend is None:
            dx = dx + dalias
        return dx, None, None, None, None


def maxpool3d_same(x, kernel, stride, pass_input=False):
    """MaxPool3dSamePadding (aj_i3d.py:6-30).  pass_input: -> (y, x_alias), see _MaxPool3d."""
    kernel, stride = tuple(int(k) for k in kernel), tuple(int(s) for s in stride)
    if pass_input and _live(x):
        return _MaxPool3d.apply(x, kernel, stride, _same_pads(x.shape[2:], kernel, stride), True)
    y = _MaxPool3d.apply(x, kernel, stride, _same_pads(x.shape[2:], kernel, stride))
    return (y, x) if pass_input else y


class _ConvStem2d(_Fn):
    """The 3 -> c0 channel 3 x 3 stem on an input that needs no gradient (stem2d.hip): direct forward; dW = sum_b dY_b Xcol_b^T with the window matrix Xcol written
    once in backward (28 rows: 27 taps + a zero row) and contracted by the streaming skinny weight-gradient kernel."""
    ROWS = 28
    enabled = True            # False: the implicit-GEMM path of rounds 1-5 (tools/ab_switch.py compares them on one box)

    @staticmethod
    def forward(ctx, x, w, stride, pad):
        L = segx.lib()
        x, w = _c(x), _c(w)
        B, Cin, H, W = x.shape
        Cout, _, K, _ = w.shape
        pl, pr, pt, pb = pad
        OH, OW = (H + pt + pb - K) // stride + 1, (W + pl + pr - K) // stride + 1
        y = _empty(x, B, Cout, OH, OW)
        L.conv2d_stem_fwd(x, w, y, B, Cin, Cout, H, W, OH, OW, K, stride, pt, pl)
        ctx.cfg = (B, Cin, Cout, H, W, OH, OW, K, stride, pt, pl)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        (x,) = ctx.saved_tensors
        B, Cin, Cout, H, W, OH, OW, K, stride, pt, pl = ctx.cfg
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        dy = _c(dy)
        P, R = OH * OW, _ConvStem2d.ROWS
        xcol = _empty(x, B, R, P)
        L.conv2d_stem_im2col(x, xcol, B, Cin, H, W, OH, OW, K, stride, pt, pl, R)
        dwr = _empty(x, Cout, R)
        _run_gemm(L, dy, xcol, dwr, Cout, R, P, (Cout * P, 0, P, 1), (R * P, 0, P, 1), (0, 0, R), (B, 1), 1.0, batch_reduce=True)
        return None, dwr[:, :Cin * K * K].reshape(Cout, Cin, K, K), None, None


def conv2d_dense(x, w, stride, pad):
    """Dense k x k 2-D convolution (only the EfficientNet stem).  pad = (left, right, top, bottom) zero padding.  The stem proper -- 3 input channels, 3 x 3, an input
    without gradient -- runs as a direct convolution (_ConvStem2d); anything else on the implicit-GEMM engine as a 3-D convolution with depth 1."""
    s = int(stride)
    if _ConvStem2d.enabled and x.dim() == 4 and x.shape[1] == 3 and tuple(w.shape[1:]) == (3, 3, 3) and s in (1, 2) and not x.requires_grad and x.shape[0] <= 65535:
        return _ConvStem2d.apply(x, w, s, tuple(int(v) for v in pad))
    return _Conv3d.apply(x.unsqueeze(2), w.unsqueeze(2), (1, s, s), ((0, 0), (int(pad[2]), int(pad[3])), (int(pad[0]), int(pad[1])))).squeeze(2)


def conv2d_stem_bias_act(x, w, bias, stride, pad, act=ACT_SWISH):
    """The EfficientNet stem with its BatchNorm folded into w [Cout, 3, 3, 3] and bias [Cout]: y = act(conv2d_dense(x, w) + bias) in the direct stem kernel's store
    (segx_conv2d_stem_bias_act_fwd).  Forward only; 3 input channels, 3 x 3, stride 1 or 2 -- anything else is an error (no other kernel carries the epilogue)."""
    if act not in (ACT_NONE, ACT_SWISH):
        raise NotImplementedError('conv2d_stem_bias_act: act is ACT_NONE or ACT_SWISH')
    _no_grad_operands('conv2d_stem_bias_act', x, w, bias)
    s = int(stride)
    if not (x.dim() == 4 and x.shape[1] == 3 and tuple(w.shape[1:]) == (3, 3, 3) and s in (1, 2) and x.shape[0] <= 65535):
        raise NotImplementedError('conv2d_stem_bias_act: only the 3-channel 3 x 3 stem at stride 1 or 2 is built')
    L = segx.lib()
    x, w = _c(x), _c(w)
    B, Cin, H, W = x.shape
    Cout, K = w.shape[0], 3
    pl, pr, pt, pb = (int(v) for v in pad)
    OH, OW = (H + pt + pb - K) // s + 1, (W + pl + pr - K) // s + 1
    y = _empty(x, B, Cout, OH, OW)
    L.conv2d_stem_bias_act_fwd(x, w, _c(bias), y, B, Cin, Cout, H, W, OH, OW, K, s, pt, pl, act)
    return y


class _PlaneBias(_Fn):
    """y[b, c] = x[b, c] + bias[c] on NC* maps (the bias of a dense convolution that ran on the implicit-GEMM engine)."""

    @staticmethod
    def forward(ctx, x, bias):
        L = segx.lib()
        x = _c(x)
        B, C = x.shape[:2]
        S = x.numel() // (B * C)
        y = torch.empty_like(x)
        L.plane_bias_add(x, _c(bias), y, B * C, C, S)
        ctx.cfg = (B, C, S)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        B, C, S = ctx.cfg
        dy = _c(dy)
        db = None
        if ctx.needs_input_grad[1]:
            rs = _empty(dy, B * C)
            L.rowsum(dy, rs, B * C, S)
            db = _empty(dy, C)
            L.colsum(rs, db, _empty(dy, L.colreduce_ws(B, C, 1)), B, C)
        return dy, db


def conv2d_bias(x, w, bias, pad=1, stride=1):
    """nn.Conv2d(Cin, Cout, k, padding=pad) with bias (unet2d/unet_parts.py:16-20): implicit-GEMM convolution + per-channel bias pass."""
    y = conv2d_dense(x, w, stride, (pad, pad, pad, pad))
    return y if bias is None else _PlaneBias.apply(y, bias)


class _PixelShuffle2(_Fn):
    """[B, 4 C, h, w] -> [B, C, 2h, 2w] (F.pixel_shuffle, r = 2); backward = the inverse re-arrangement"""
    @staticmethod
    def forward(ctx, x):
        L = segx.lib()
        x = _c(x)
        B, C4, h, w = x.shape
        y = _empty(x, B, C4 // 4, 2 * h, 2 * w)
        L.pixel_shuffle2(x, y, B * (C4 // 4), h, w, 0)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = segx.lib()
        dy = _c(dy)
        B, C, H, W = dy.shape
        dx = _empty(dy, B, 4 * C, H // 2, W // 2)
        L.pixel_shuffle2(dy, dx, B * C, H // 2, W // 2, 1)
        return dx


def conv_transpose2x2(x, weight, bias=None):
    """nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) (unet_parts.py:53): non-overlapping, so it is a pointwise convolution onto the
    4 Cout channels (co, a, c) -- on the tile engine -- followed by the 2 x 2 re-arrangement.  weight [Cin, Cout, 2, 2], bias [Cout]."""
    cin, cout = weight.shape[0], weight.shape[1]
    wr = weight.permute(1, 2, 3, 0).reshape(4 * cout, cin)                   # rows (co, a, c): the pixel-shuffle channel order
    br = None if bias is None else bias.repeat_interleave(4)
    return _PixelShuffle2.apply(conv1x1(x, wr.reshape(4 * cout, cin, 1, 1), br))


def maxpool2d(x, k=2):
    """nn.MaxPool2d(k) (stride k, no padding, floor): the 3-D max-pool kernels on a depth-1 volume."""
    return _MaxPool3d.apply(x.unsqueeze(2), (1, k, k), (1, k, k), ((0, 0), (0, 0), (0, 0))).squeeze(2)


# -------------------------------------------------------------------------------------------------
# Foreground mask and label maps (no gradients)
# -------------------------------------------------------------------------------------------------
def nonzero_mask(x, pool):
    """get_mask (segtran2d.py:229-233 / segtran3d.py:266-270): [B,C,*spatial] -> 0/1 float [B, *spatial // pool]."""
    L = segx.lib()
    x = _c(x.detach())
    B, C = x.shape[:2]
    D, H, W = _dhw(x.shape[2:])
    kd, kh, kw = _dhw(pool)
    out = _empty(x, B, D // kd, H // kh, W // kw)
    L.nonzero_mask(x, out, B, C, D, H, W, kd, kh, kw)
    return out if x.dim() == 5 else out[:, 0]


def bridge_mask(batch, weight, bias, pool):
    """nonzero_mask(conv1x1(batch, weight, bias).permute(0, 1, 4, 2, 3), pool) for the raw 3-D batch [B, Cb, H, W, D] without the bridged image: see segx_bridge_mask."""
    L = segx.lib()
    x = _c(batch.detach())
    B, Cb, H, W, D = x.shape
    C3 = weight.shape[0]
    kd, kh, kw = (int(v) for v in pool)
    out = _empty(x, B, D // kd, H // kh, W // kw)
    L.bridge_mask(x, _c(weight.detach().reshape(C3, Cb)), None if bias is None else bias.detach(), out, B, Cb, C3, H, W, D, kd, kh, kw)
    return out


def label_nhot(labels, mode, exclusive=False, num_classes=None):
    """mode 'fundus' | 'polyp' (uint8 [B,Cin,*S]) | 'brats' (integer [B,*S]) -> float n-hot [B,C,*S].
    exclusive (fundus only, train2d.py --exclusive): the disc channel excludes the cup (datasets2d.py:110-111).
    mode 'oct': index masks [B,1,H,W] / [B,H,W] -> one-hot [B,num_classes,H,W] (index_onehot; num_classes defaults to the task's 10)."""
    if mode == 'oct':
        lab = labels[:, 0] if labels.dim() == 4 else labels
        return index_onehot(lab, 10 if num_classes is None else num_classes)
    L = segx.lib()
    m = {'fundus': 0, 'polyp': 1, 'brats': 2}[mode]
    if m == 0 and exclusive:
        m = 3
    if m == 2:
        lab = _c(labels.to(torch.int32))
        B, S = lab.shape[0], lab[0].numel()
        out = torch.empty((B, 4) + tuple(lab.shape[1:]), dtype=torch.float32, device=lab.device)
        L.label_nhot(lab, out, B, 1, S, 2)
    else:
        lab = _c(labels.to(torch.uint8))
        B, Cin, S = lab.shape[0], lab.shape[1], lab[0, 0].numel()
        out = torch.empty((B, 2 if m == 1 else 3) + tuple(lab.shape[2:]), dtype=torch.float32, device=lab.device)
        L.label_nhot(lab, out, B, Cin, S, m)
    return out


def resized_crop3d(x, resized, out_size, offset):
    """[B, C, d, h, w] --(trilinear resample to `resized`, zero pad, crop `out_size` at `offset` = crop start - front pad)--> [B, C, *out_size].
    Data augmentation (no gradient): the fused form of F.interpolate + F.pad + slicing in reference datasets3d.py:611-665."""
    L = segx.lib()
    x = _c(x.detach().float())
    B, C = x.shape[:2]
    y = _empty(x, B, C, *out_size)
    L.resized_crop3d(x, y, B * C, tuple(x.shape[2:]) + tuple(resized) + tuple(out_size) + tuple(offset))
    return y


# -------------------------------------------------------------------------------------------------
# Data augmentation on the device (augment.hip): no autograd; random parameters are drawn by the callers (dataloaders/)
# -------------------------------------------------------------------------------------------------
class AxisMap:
    """A composition of flips / rot90s / crops / zero pads of the three trailing axes of a tensor, applied by ONE gather (segx_axis_gather).
    State: for each INPUT axis b the output axis p[b] that feeds it, a sign and an offset (i_b = s[b] * o_{p[b]} + t[b]), plus the current
    output extents.  Every method returns self (chainable); out-of-range reads are zeros (that is what padding is)."""

    def __init__(self, shape):
        self.I = [int(v) for v in shape]
        self.O = list(self.I)
        self.p, self.s, self.t = [0, 1, 2], [1, 1, 1], [0, 0, 0]

    def flip(self, axis):
        for b in range(3):
            if self.p[b] == axis:
                self.t[b] += self.s[b] * (self.O[axis] - 1); self.s[b] = -self.s[b]
        return self

    def rot90(self, k=1, axes=(0, 1)):
        """numpy.rot90(m, k, axes): one step is new[i][j] = cur[j][n1 - 1 - i] on the two axes"""
        a0, a1 = axes
        for _ in range(k % 4):
            n1 = self.O[a1]
            for b in range(3):
                if self.p[b] == a0:
                    self.p[b] = a1
                elif self.p[b] == a1:
                    self.p[b] = a0; self.t[b] += self.s[b] * (n1 - 1); self.s[b] = -self.s[b]
            self.O[a0], self.O[a1] = self.O[a1], self.O[a0]
        return self

    def window(self, start, size):
        """crop (start >= 0) and / or zero-pad (start < 0, or size beyond the extent): new[o] = cur[o + start]"""
        for a in range(3):
            for b in range(3):
                if self.p[b] == a:
                    self.t[b] += self.s[b] * int(start[a])
            self.O[a] = int(size[a])
        return self

    def geom(self):
        src, sgn, off = [0] * 3, [1] * 3, [0] * 3
        for b in range(3):
            src[self.p[b]], sgn[self.p[b]], off[self.p[b]] = b, self.s[b], self.t[b]
        return tuple(self.I) + tuple(self.O) + tuple(src) + tuple(sgn) + tuple(off)

    def apply(self, x):
        """x [..., I0, I1, I2] -> [..., O0, O1, O2]"""
        L = segx.lib()
        xs = _c(x.detach().float())
        assert list(xs.shape[-3:]) == self.I, (tuple(xs.shape), self.I)
        y = torch.empty(tuple(xs.shape[:-3]) + tuple(self.O), dtype=torch.float32, device=xs.device)
        L.axis_gather(xs, y, max(1, xs.numel() // (self.I[0] * self.I[1] * self.I[2])), self.geom())
        return y


def add_noise(x, mu=0.0, sigma=0.1, nonzero_only=True, noise=None):
    """RandomNoise (datasets3d.py:581-597) on the device; `noise`: a standard-normal field to use instead of the Philox stream (parity tests)."""
    L = segx.lib()
    xs = _c(x.detach().float())
    y = torch.empty_like(xs)
    seed, off = _Rng.reserve(xs.numel())
    L.add_noise(xs, None if noise is None else _c(noise.float()), y, mu, sigma, nonzero_only, seed, off)
    return y


def resize2d(x, size, mode='cubic', quantize=False):
    """[..., h, w] -> [..., H, W] with cv2.resize conventions (imgaug's Resize / keep_size): mode 'nearest' | 'linear' | 'cubic'"""
    L = segx.lib()
    xs = _c(x.detach().float())
    h, w = xs.shape[-2:]
    y = torch.empty(tuple(xs.shape[:-2]) + (int(size[0]), int(size[1])), dtype=torch.float32, device=xs.device)
    L.resize2d(xs, y, max(1, xs.numel() // (h * w)), h, w, int(size[0]), int(size[1]), {'nearest': 0, 'linear': 1, 'cubic': 2}[mode], quantize)
    return y


def color_blend(x, mode, factor, quantize=True):
    """x [B, 3, H, W] (0..255 scale); mode 'brightness' | 'contrast' | 'saturation' | 'grayscale' (factor = 1 - alpha); factor [B] tensor"""
    L = segx.lib()
    xs = _c(x.detach().float())
    B, HW = xs.shape[0], xs.shape[2] * xs.shape[3]
    m = {'brightness': 0, 'contrast': 1, 'saturation': 2, 'grayscale': 3}[mode]
    f = _c(factor.to(xs.device, torch.float32))
    pivot = None
    if m == 1:
        pivot = torch.empty(B, dtype=torch.float32, device=xs.device)
        L.gray_mean(xs, pivot, B, HW, quantize)
    y = torch.empty_like(xs)
    L.color_blend(xs, y, B, HW, m, f, pivot, quantize)
    return y


def normalize(x, mean, std, scale=1.0 / 255.0):
    """transforms.ToTensor + Normalize: (x * scale - mean[c]) / std[c]; x [B, C, H, W]"""
    L = segx.lib()
    xs = _c(x.detach().float())
    B, C = xs.shape[:2]
    y = torch.empty_like(xs)
    L.normalize(xs, y, B, C, xs.numel() // (B * C), scale, torch.as_tensor(mean, dtype=torch.float32, device=xs.device),
                torch.as_tensor(std, dtype=torch.float32, device=xs.device))
    return y


# -------------------------------------------------------------------------------------------------
# Evaluation path (infer.hip): no autograd, everything under torch.no_grad()
# -------------------------------------------------------------------------------------------------
def window_accum(scores, acc, cnt, origin):
    """acc[:, :, window] += sigmoid(resample(scores -> window)); cnt[:, window] += 1.  scores [B,C,*s], acc [B,C,*canvas], cnt [B,*canvas];
    the window has the size given by `origin = (start..., size...)`: 2-D (y0, x0, H, W), 3-D (z0, y0, x0, D, H, W)."""
    L = segx.lib()
    scores = _c(scores.detach())
    nd = scores.dim() - 2
    B, C = scores.shape[:2]
    s3 = (1,) * (3 - nd) + tuple(scores.shape[2:])
    o3 = (0,) * (3 - nd) + tuple(origin[:nd]); w3 = (1,) * (3 - nd) + tuple(origin[nd:])
    c3 = (1,) * (3 - nd) + tuple(acc.shape[2:])
    assert acc.is_contiguous() and cnt.is_contiguous() and acc.shape[:2] == (B, C) and tuple(cnt.shape) == (B,) + tuple(acc.shape[2:])
    L.window_accum(scores, acc, cnt, B, C, s3 + w3 + c3 + o3)


def harden_segmap(acc, cnt=None, mode=0, T=0.5, want_soft=True):
    """(soft, hard): soft = acc / cnt (or acc), hard = n-hot 0/1 floats with the background consistency rule; mode 1 = BraTS."""
    L = segx.lib()
    acc = _c(acc.detach())
    B, C = acc.shape[:2]
    S = acc.numel() // (B * C)
    hard = torch.empty_like(acc)
    soft = torch.empty_like(acc) if want_soft else None
    L.harden_segmap(acc, _c(cnt) if cnt is not None else None, soft, hard, B, C, S, mode, T)
    return soft, hard


class WindowTable:
    """The window origins of one sliding-window evaluation: `origins` = one (start...) tuple per window (2-D (y0, x0), 3-D (z0, y0, x0)) in padded-canvas
    coordinates, in the order the eager loops visit the windows.  Holds the device table the kernels read (int32 [nwin, 3]) and the host copy their refusals
    are decided on; build it once and pass it to window_gather / window_merge (building one copies to the device, which a graph capture refuses)."""

    def __init__(self, origins, device):
        o = [tuple(int(v) for v in w) for w in origins]
        if not o or any(len(w) != len(o[0]) or len(w) not in (2, 3) for w in o):
            raise ValueError('WindowTable: one (y0, x0) or (z0, y0, x0) per window, at least one window')
        self.nd, self.nwin = len(o[0]), len(o)
        self.origins = tuple(o)
        flat = [v for w in o for v in (0,) * (3 - self.nd) + w]
        self.host = (segx.c_i * len(flat))(*flat)
        self.dev = torch.tensor(flat, dtype=torch.int32, device=device).view(self.nwin, 3)


MAX_VIEWS = 8                                    # SEGX_MAX_VIEWS of include/segx.h


def check_views(views, nd, what='tta'):
    """The views of a flip test-time augmentation as a tuple of sorted axis tuples, in the given order.  A view is a tuple of distinct spatial axes to flip
    (0 = the first spatial axis of the image; () is the identity and has to be listed to be used).  ValueError for an empty sequence, more than MAX_VIEWS views, an
    axis outside 0..nd-1, an axis twice in a view, or the same set of axes twice."""
    try:
        vs = [tuple(int(a) for a in v) for v in views]
    except TypeError:
        raise ValueError('%s: a sequence of views, each a tuple of axis indices, not %r' % (what, views))
    if not 1 <= len(vs) <= MAX_VIEWS:
        raise ValueError('%s: between 1 and %d views, not %d' % (what, MAX_VIEWS, len(vs)))
    for v in vs:
        if any(a < 0 or a >= nd for a in v):
            raise ValueError('%s: view %r names an axis outside 0..%d' % (what, v, nd - 1))
        if len(set(v)) != len(v):
            raise ValueError('%s: view %r names an axis twice' % (what, v))
    if len({frozenset(v) for v in vs}) != len(vs):
        raise ValueError('%s: the same view twice in %r' % (what, tuple(vs)))
    return tuple(tuple(sorted(v)) for v in vs)


class ViewTable:
    """The views of one flip test-time augmentation for images of `nd` spatial axes (check_views), as the flip masks the kernels read: bit (3 - nd + a) for spatial
    axis a, i.e. bit 0 = the depth axis of the kernels' [B, C, ID, IH, IW] frame.  Holds the device table (int32 [V]) and the host copy the refusals are decided on;
    like WindowTable it is built once, before a capture."""

    def __init__(self, views, nd, device):
        if nd not in (2, 3):
            raise ValueError('ViewTable: 2 or 3 spatial axes, not %r' % (nd,))
        self.nd, self.views = nd, check_views(views, nd, 'ViewTable')
        self.V = len(self.views)
        self.masks = tuple(sum(1 << (3 - nd + a) for a in v) for v in self.views)
        self.host = (segx.c_i * self.V)(*self.masks)
        self.dev = torch.tensor(self.masks, dtype=torch.int32, device=device)


def _view_table(what, views, nd, device):
    if isinstance(views, ViewTable):
        if views.nd != nd:
            raise TypeError('%s: `views` is a ViewTable of %d-D views' % (what, nd))
        return views
    return ViewTable(views, nd, device)


def _window_geometry(what, table, nd, image_size, window, pads, canvas):
    if not isinstance(table, WindowTable) or table.nd != nd:
        raise TypeError('%s: `table` is a WindowTable of %d-D origins' % (what, nd))
    image_size, window = tuple(int(v) for v in image_size), tuple(int(v) for v in window)
    pads = tuple(int(v) for v in pads) if pads is not None else (0,) * nd
    canvas = tuple(int(v) for v in canvas) if canvas is not None else tuple(max(i + p, w) for i, p, w in zip(image_size, pads, window))
    if not len(image_size) == len(window) == len(pads) == len(canvas) == nd:
        raise ValueError('%s: image size, window, pads and canvas must all have %d entries' % (what, nd))
    one, zero = (1,) * (3 - nd), (0,) * (3 - nd)
    return one + image_size, one + window, zero + pads, one + canvas


def window_gather(image, table, window, patch_size=None, pads=None, canvas=None, views=None):
    """The network's input for every window: image [B, C, *spatial] -> [nwin * B, C, *patch_size], window-major then image; entry k * B + b is
    interp_linear(padded[b, :, window k], patch_size) bit for bit (the plain crop when patch_size == window), where `padded` is the image zero-padded to `canvas`
    with the left pads `pads` -- it never exists in memory.  One launch (segx_window_gather) for the crops of all windows; when the patch size differs, ONE
    interp_linear over the stacked crops follows (per-plane arithmetic: the bits of the per-window calls).  table: WindowTable; canvas defaults to
    max(image + pads, window).  Forward only.
    views (a ViewTable, or a sequence of views -- inside a capture only the former): the crops of every view of a flip test-time augmentation in the same one launch
    (segx_window_gather_views): [V * nwin * B, C, *patch_size], view-major, then window, then image; view v's rows are window_gather(image.flip(axes of view v))
    bit for bit.  The flip is index arithmetic: no flipped image exists."""
    _no_grad_operands('window_gather', image)
    L = segx.lib()
    image = _c(image.detach())
    nd = image.dim() - 2
    B, C = image.shape[:2]
    i3, w3, p3, c3 = _window_geometry('window_gather', table, nd, image.shape[2:], window, pads, canvas)
    if views is None:
        out = _empty(image, table.nwin * B, C, *w3[3 - nd:])
        L.window_gather(image, table.dev, table.host, out, table.nwin, B, C, i3 + p3 + w3 + c3)
    else:
        vt = _view_table('window_gather', views, nd, image.device)
        out = _empty(image, vt.V * table.nwin * B, C, *w3[3 - nd:])
        L.window_gather_views(image, table.dev, table.host, vt.dev, vt.host, out, table.nwin, vt.V, B, C, i3 + p3 + w3 + c3)
    if patch_size is not None and tuple(int(v) for v in patch_size) != w3[3 - nd:]:
        out = interp_linear(out, patch_size)
    return out


def window_merge(scores, table, window, image_size, pads=None, canvas=None, mode=0, T=0.5, views=None):
    """(soft, hard) [B, C, *image_size] of the whole sliding-window evaluation in one launch (segx_window_merge): scores [nwin * B, C, *s] (laid out as
    window_gather's output).  Bit for bit what window_accum per window (in the table's order, on zeroed acc / cnt) followed by harden_segmap(mode, T) leaves in
    the un-padded region of the canvas; acc and cnt never exist.  A cell that no window of a hand-built table covers is 0 / 0 = NaN, as on the eager path
    (infer2d.sliding_windows never leaves one).  Forward only.
    views (as window_gather): scores [V * nwin * B, C, *s] hold the views of a flip test-time augmentation; one launch (segx_window_merge_views) forms
    soft = (((soft_0 + soft_1) + soft_2) + ...) / float(V) -- soft_v = the soft map of view v's rows flipped back along its axes, fp32 adds in the views' order, one
    division -- and hardens it (mode, T): bit for bit the composition of window_merge per view, torch.flip, the adds, the division and harden_segmap."""
    _no_grad_operands('window_merge', scores)
    L = segx.lib()
    scores = _c(scores.detach())
    nd = scores.dim() - 2
    C = scores.shape[1]
    vt = None if views is None else _view_table('window_merge', views, nd, scores.device)
    rows = table.nwin * (1 if vt is None else vt.V)
    if scores.shape[0] % rows:
        raise ValueError('window_merge: scores holds %d samples, no multiple of the %d windows%s' %
                         (scores.shape[0], table.nwin, '' if vt is None else ' x %d views' % vt.V))
    B = scores.shape[0] // rows
    i3, w3, p3, c3 = _window_geometry('window_merge', table, nd, image_size, window, pads, canvas)
    soft = _empty(scores, B, C, *i3[3 - nd:])
    hard = torch.empty_like(soft)
    geom = (1,) * (3 - nd) + tuple(scores.shape[2:]) + w3 + c3 + p3 + i3
    if vt is None:
        L.window_merge(scores, table.dev, table.host, soft, hard, table.nwin, B, C, geom, mode, T)
    else:
        L.window_merge_views(scores, table.dev, table.host, vt.dev, vt.host, soft, hard, table.nwin, vt.V, B, C, geom, mode, T)
    return soft, hard


def dice_scores(pred, gt, smooth=1e-5):
    """calc_dice (test_util2d.py:233-240) for every leading plane of pred/gt [..., *spatial] given as [P, S]-viewable tensors:
    (2 sum(p g) + s) / (sum p^2 + sum g^2 + s).  Returns a [P] tensor."""
    L = segx.lib()
    pred, gt = _c(pred.detach().float()), _c(gt.detach().float())
    P = pred.shape[0]
    S = pred.numel() // P
    sums = L.dice_sums(pred, gt, P, S)
    return (2 * sums[:, 0] + smooth) / (sums[:, 1] + sums[:, 2] + smooth)


# -------------------------------------------------------------------------------------------------
# Surface-distance metrics (metrics.hip): border map, exact squared distance field, histogram of squared surface distances.  Planes-first tensors:
# [P, H, W] is a stack of images (nd = 2), [P, D, H, W] a stack of volumes (nd = 3).  Forward only.
# -------------------------------------------------------------------------------------------------
def _surface_operand(what, t, dtype=None):
    if torch.is_grad_enabled() and t.requires_grad:
        raise RuntimeError(what + ' is forward-only: call it under torch.no_grad() or on tensors without gradient')
    if t.dim() not in (3, 4):
        raise ValueError('%s: [P, H, W] or [P, D, H, W] tensors, not rank %d' % (what, t.dim()))
    if dtype is not None and t.dtype != dtype:
        raise TypeError('%s: a %s tensor, not %s' % (what, dtype, t.dtype))
    P = t.shape[0]
    D, H, W = (1,) * (4 - t.dim()) + tuple(t.shape[1:])
    return _c(t.detach()), P, D, H, W


def surface_border(masks):
    """border = mask XOR erode(mask) with the face neighbourhood (4 neighbours for [P, H, W], 6 for [P, D, H, W]); a voxel is set iff it is not 0, neighbours
    outside the array are unset.  What medpy's surface distances call the surface (connectivity 1).  Returns uint8 0 / 1 of the same shape."""
    m, P, D, H, W = _surface_operand('surface_border', masks)
    m = m.float()
    border = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    segx.lib().surface_border(m, border, P, D, H, W, m.dim() - 1)
    return border


def edt_sq(border):
    """int32 squared Euclidean distance (unit spacing) of EVERY voxel to the nearest set voxel of its plane of `border` (uint8), exact; a plane without a set voxel
    is segx.SegxLib.EDT_INF throughout.  Extents above segx.SegxLib.EDT_MAX_EXTENT are refused."""
    b, P, D, H, W = _surface_operand('edt_sq', border, torch.uint8)
    d2 = torch.empty(b.shape, dtype=torch.int32, device=b.device)
    segx.lib().edt_sq(b, d2, P, D, H, W)
    return d2


def surface_hist(border_from, d2_to):
    """int32 [P, nbins], nbins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1: hist[p, k] = number of set voxels of border_from[p] (uint8) whose d2_to[p] (int32, from edt_sq) is
    k -- the squared surface distances from one mask's border to the other's as counts.  Voxels at the sentinel (an empty other mask) are not counted."""
    b, P, D, H, W = _surface_operand('surface_hist', border_from, torch.uint8)
    d, *_ = _surface_operand('surface_hist', d2_to, torch.int32)
    if b.shape != d.shape:
        raise ValueError('surface_hist: border_from %s and d2_to %s differ in shape' % (tuple(b.shape), tuple(d.shape)))
    nbins = (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1
    hist = torch.zeros(P, nbins, dtype=torch.int32, device=b.device)
    segx.lib().surface_hist(b, d, hist, P, D, H, W, nbins)
    return hist


def brats_case_tail(soft, hard, gt=None, want_labels=True, counts=None, labels=None):
    """The tail of one BraTS case in one launch (segx_brats_case_tail): soft, hard float32 [4, *spatial] (or [4, S]) as window_merge / harden_segmap leave them in mode 1;
    gt: the raw label volume [*spatial] (converted to int32 when it is not), or None.  Returns (counts, labels):
      counts int32 [3, 3] -- per foreground class {sum pred * gt, sum pred, sum gt} against brats_map_label(gt) (a raw 4 counts as 3), which never exists as a
        tensor; None without gt;
      labels uint8 [*spatial] -- argmax(brats_inv_map_label(soft)) with 3 written as 4, the volume the reference saves; None with want_labels=False.
    counts / labels: tensors to write into (a captured graph passes its static ones); passing `labels` asks for them.  No copy to the host, no synchronisation.
    Forward only."""
    _no_grad_operands('brats_case_tail', soft, hard)
    if soft.dim() < 2 or soft.shape[0] != 4 or soft.shape != hard.shape or soft.dtype != torch.float32 or hard.dtype != torch.float32:
        raise ValueError('brats_case_tail: soft %s and hard %s must be float32 [4, *spatial] tensors of one shape' % (tuple(soft.shape), tuple(hard.shape)))
    spatial = tuple(soft.shape[1:])
    S = soft[0].numel()
    if S < 1:
        raise ValueError('brats_case_tail: empty tensor %s' % (tuple(soft.shape),))
    soft, hard = _c(soft.detach()), _c(hard.detach())
    if gt is None:
        if counts is not None:
            raise ValueError('brats_case_tail: counts need gt')
    else:
        if tuple(gt.shape) != spatial:
            raise ValueError('brats_case_tail: gt %s is not the volume %s' % (tuple(gt.shape), spatial))
        gt = _c(gt.detach().to(torch.int32))
        if counts is None:
            counts = torch.empty(3, 3, dtype=torch.int32, device=soft.device)
        elif counts.dtype != torch.int32 or tuple(counts.shape) != (3, 3) or not counts.is_contiguous():
            raise ValueError('brats_case_tail: counts is a contiguous int32 [3, 3] tensor')
    if labels is not None:
        if labels.dtype != torch.uint8 or tuple(labels.shape) != spatial or not labels.is_contiguous():
            raise ValueError('brats_case_tail: labels is a contiguous uint8 %s tensor' % (spatial,))
    elif want_labels:
        labels = torch.empty(spatial, dtype=torch.uint8, device=soft.device)
    if counts is None and labels is None:
        raise ValueError('brats_case_tail: nothing to compute (no gt and want_labels=False)')
    segx.lib().brats_case_tail(soft, hard, gt if counts is not None else None, counts, labels, S)
    return counts, labels


# -------------------------------------------------------------------------------------------------
# One-hot tasks (metrics.hip; the OCT task): index masks -> one-hot floats, n-hot maps -> colours, and the evaluation tail in one pass.  Forward only, no copy to the
# host and no synchronisation.
# -------------------------------------------------------------------------------------------------
def _class_count(what, C, low=1):
    if int(C) != C or not low <= int(C) <= segx.SegxLib.MAX_CLASSES:
        raise ValueError('%s: %r classes, not %d .. %d' % (what, C, low, segx.SegxLib.MAX_CLASSES))
    return int(C)


def index_onehot(labels, num_classes):
    """float32 [B, num_classes, *spatial] from an integer index mask [B, *spatial] (segx_index_onehot): out[b, c] = (labels[b] == c).  uint8 and int32 masks are read
    as they are, other integer types are converted to int32 first.  A label outside 0 .. num_classes - 1 sets no class (the reference's scatter_ raises there)."""
    _no_grad_operands('index_onehot', labels)
    C = _class_count('index_onehot', num_classes)
    if labels.dim() < 2:
        raise ValueError('index_onehot: an index mask [B, *spatial], not rank %d' % labels.dim())
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise TypeError('index_onehot: an integer index mask, not %s' % labels.dtype)
    lab = _c(labels.detach() if labels.dtype in (torch.uint8, torch.int32) else labels.detach().to(torch.int32))
    B = lab.shape[0]
    if lab.numel() == 0:
        raise ValueError('index_onehot: empty tensor %s' % (tuple(labels.shape),))
    out = torch.empty((B, C) + tuple(lab.shape[1:]), dtype=torch.float32, device=lab.device)
    segx.lib().index_onehot(lab, lab.element_size(), out, B, C, lab.numel() // B)
    return out


_COLOR_TABLES = {}


def _color_table(what, colormap, C, device):
    """the uint8 [C, 3] device table of a colormap given as a tensor (used as it is when it already is one) or as C (r, g, b) triples (built once per device and kept)"""
    if isinstance(colormap, torch.Tensor):
        if colormap.dim() != 2 or colormap.shape[1] != 3 or colormap.shape[0] < C:
            raise ValueError('%s: colormap %s is no [C, 3] table with C >= %d' % (what, tuple(colormap.shape), C))
        if colormap.dtype == torch.uint8 and colormap.device == device and colormap.is_contiguous():
            return colormap
        if colormap.is_floating_point():
            raise TypeError('%s: colormap holds integer colours 0 .. 255, not %s' % (what, colormap.dtype))
        return _c(colormap.to(device=device, dtype=torch.uint8))
    rows = tuple(tuple(_uint8_value(what + ': colormap', v) for v in row) for row in colormap)
    if len(rows) < C or any(len(r) != 3 for r in rows):
        raise ValueError('%s: colormap needs %d (r, g, b) rows' % (what, C))
    key = (rows, device)
    table = _COLOR_TABLES.get(key)
    if table is None:
        table = _COLOR_TABLES[key] = torch.tensor(rows, dtype=torch.uint8, device=device)
    return table


def onehot_colormap(nhot, colormap=None):
    """uint8 [B, *spatial, 3] from n-hot floats [B, C, *spatial] (segx_onehot_colormap): colormap[argmax over the classes], the lowest index winning a tie as in
    torch.argmax; colormap None: the index itself in all three bytes.  colormap: a [C, 3] tensor of colours 0 .. 255 (a uint8 tensor on the device is read in place)
    or C (r, g, b) triples."""
    _no_grad_operands('onehot_colormap', nhot)
    if nhot.dim() < 3:
        raise ValueError('onehot_colormap: [B, C, *spatial] maps, not rank %d' % nhot.dim())
    B, C = nhot.shape[:2]
    C = _class_count('onehot_colormap', C)
    x = _c(nhot.detach().float())
    if x.numel() == 0:
        raise ValueError('onehot_colormap: empty tensor %s' % (tuple(nhot.shape),))
    table = None if colormap is None else _color_table('onehot_colormap', colormap, C, x.device)
    out = torch.empty((B,) + tuple(x.shape[2:]) + (3,), dtype=torch.uint8, device=x.device)
    segx.lib().onehot_colormap(x, table, out, B, C, x[0, 0].numel())
    return out


def onehot_case_tail(soft, gt=None, colormap=None, T=0.5, want_labels=True, counts=None, labels=None, rgb=None):
    """The evaluation tail of a one-hot task in one launch (segx_onehot_case_tail): soft float32 [B, C, *spatial] as window_merge leaves it; gt: the index mask
    [B, *spatial] (converted to uint8 when it is not), or None.  Returns (counts, labels, rgb):
      counts int32 [B, C - 1, 3] -- per image and foreground class {sum pred * gt, sum pred, sum gt} with pred = soft[:, c] >= T and gt = (mask == c); None without gt;
      labels uint8 [B, *spatial] -- the lowest class >= 1 that is on, 0 where none is: onehot_inv_map(harden_segmap2d(soft)) as indices; None with want_labels=False;
      rgb uint8 [B, *spatial, 3] -- colormap[labels]; None without a colormap (a [C, 3] tensor or C triples, as onehot_colormap takes it).
    counts / labels / rgb: tensors to write into (a captured graph passes its static ones); passing `labels` asks for them.  Forward only."""
    _no_grad_operands('onehot_case_tail', soft)
    if soft.dim() < 3 or soft.dtype != torch.float32:
        raise ValueError('onehot_case_tail: soft %s %s must be a float32 [B, C, *spatial] tensor' % (soft.dtype, tuple(soft.shape)))
    B, C = soft.shape[:2]
    C = _class_count('onehot_case_tail', C, low=2)
    spatial = tuple(soft.shape[2:])
    S = soft[0, 0].numel() if B else 0
    if B < 1 or S < 1:
        raise ValueError('onehot_case_tail: empty tensor %s' % (tuple(soft.shape),))
    soft = _c(soft.detach())
    dev = soft.device
    if gt is None:
        if counts is not None:
            raise ValueError('onehot_case_tail: counts need gt')
    else:
        if tuple(gt.shape) != (B,) + spatial:
            raise ValueError('onehot_case_tail: gt %s is not the index mask %s' % (tuple(gt.shape), (B,) + spatial))
        if gt.is_floating_point() or gt.dtype == torch.bool:
            raise TypeError('onehot_case_tail: gt is an integer index mask, not %s' % gt.dtype)
        if gt.dtype != torch.uint8:
            gt = gt.detach().clamp(-1, 255).to(torch.uint8)           # -1 -> 255: outside every class, as any label >= C
        gt = _c(gt.detach())
        if counts is None:
            counts = torch.empty(B, C - 1, 3, dtype=torch.int32, device=dev)
        elif counts.dtype != torch.int32 or tuple(counts.shape) != (B, C - 1, 3) or not counts.is_contiguous():
            raise ValueError('onehot_case_tail: counts is a contiguous int32 [%d, %d, 3] tensor' % (B, C - 1))
    if labels is not None:
        if labels.dtype != torch.uint8 or tuple(labels.shape) != (B,) + spatial or not labels.is_contiguous():
            raise ValueError('onehot_case_tail: labels is a contiguous uint8 %s tensor' % ((B,) + spatial,))
    elif want_labels:
        labels = torch.empty((B,) + spatial, dtype=torch.uint8, device=dev)
    table = None
    if colormap is None:
        if rgb is not None:
            raise ValueError('onehot_case_tail: rgb needs a colormap')
    else:
        table = _color_table('onehot_case_tail', colormap, C, dev)
        if rgb is None:
            rgb = torch.empty((B,) + spatial + (3,), dtype=torch.uint8, device=dev)
        elif rgb.dtype != torch.uint8 or tuple(rgb.shape) != (B,) + spatial + (3,) or not rgb.is_contiguous():
            raise ValueError('onehot_case_tail: rgb is a contiguous uint8 %s tensor' % ((B,) + spatial + (3,),))
    if counts is None and labels is None and rgb is None:
        raise ValueError('onehot_case_tail: nothing to compute (no gt, no colormap and want_labels=False)')
    segx.lib().onehot_case_tail(soft, gt if counts is not None else None, table, counts, labels, rgb, B, C, S, T)
    return counts, labels, rgb


# -------------------------------------------------------------------------------------------------
# Tail of the 2-D evaluation (components.hip): connected components, fragment removal, row extents, n-hot -> pixel values.  Stacks of planes [P, H, W] (or one
# [H, W] plane); integer kernels with exact results; no copy to the host and no synchronisation, so the calls can be captured into a graph.  Forward only.
# -------------------------------------------------------------------------------------------------
def _planes_operand(what, t, dtypes):
    if torch.is_grad_enabled() and t.requires_grad:
        raise RuntimeError(what + ' is forward-only: call it under torch.no_grad() or on tensors without gradient')
    if t.dim() not in (2, 3):
        raise ValueError('%s: an [H, W] or [P, H, W] tensor, not rank %d' % (what, t.dim()))
    if t.dtype not in dtypes:
        raise TypeError('%s: a %s tensor, not %s' % (what, ' / '.join(str(d) for d in dtypes), t.dtype))
    P, H, W = (1,) * (3 - t.dim()) + tuple(t.shape)
    if P < 1 or H < 1 or W < 1:
        raise ValueError('%s: empty tensor %s' % (what, tuple(t.shape)))
    if H * W >= segx.SegxLib.CCL_MAX_PLANE:
        raise ValueError('%s: H * W = %d is not below the limit of 2^30 pixels per plane' % (what, H * W))
    t = _c(t.detach())
    return (t.view(torch.uint8) if t.dtype == torch.bool else t), P, H, W


def _uint8_value(what, v):
    if int(v) != v or not 0 <= int(v) <= 255:
        raise ValueError('%s: %r is no uint8 value' % (what, v))
    return int(v)


def label_components(mask, bg_value=0):
    """8-connected components (cv2.connectedComponents' default connectivity) of every plane of a uint8 / bool mask [P, H, W] or [H, W]; a pixel is background
    iff it equals bg_value.  Returns (labels, sizes), int32 of the mask's shape: labels = 0 on the background, else 1 + the raster index inside the plane of the
    component's first pixel; sizes = the component's pixel count at that first pixel, 0 everywhere else."""
    m, P, H, W = _planes_operand('label_components', mask, (torch.uint8, torch.bool))
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    sizes = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    segx.lib().ccl2d(m, _uint8_value('label_components: bg_value', bg_value), labels, sizes, P, H, W)
    return labels, sizes


def remove_fragments(seg_u8, bg_value):
    """Per plane of the uint8 label image(s) [P, H, W] / [H, W]: label the 8-connected components of seg != bg_value, keep the two most frequent of {background,
    components} (ties: the background, then the component that starts first) and paint the rest bg_value.  Returns a new tensor; three kernels' worth of launches
    (segx_ccl2d, segx_frag_keep2, segx_frag_apply), nothing on the host."""
    s, P, H, W = _planes_operand('remove_fragments', seg_u8, (torch.uint8,))
    bg = _uint8_value('remove_fragments: bg_value', bg_value)
    L = segx.lib()
    labels = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    sizes = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    keep = torch.empty(P, 2, dtype=torch.int32, device=s.device)
    out = torch.empty_like(s)
    L.ccl2d(s, bg, labels, sizes, P, H, W)
    L.frag_keep2(sizes, keep, P, H, W)
    L.frag_apply(s, labels, keep, out, P, H, W, bg)
    return out


# -------------------------------------------------------------------------------------------------
# Connected-component post-processing of 3-D predictions (components.hip): 6- / 26-connected labelling of volumes [X, Y, Z] or stacks [V, X, Y, Z],
# the keep rule and the BraTS rule.  Integer-exact; no copy to the host and no synchronisation, so the calls can be captured into a graph.  Forward only.
# -------------------------------------------------------------------------------------------------
CONNECTIVITIES3D = (6, 26)


def check_connectivity3d(what, connectivity):
    if connectivity not in CONNECTIVITIES3D or isinstance(connectivity, bool):
        raise ValueError('%s: connectivity %r is neither 6 nor 26' % (what, connectivity))
    return int(connectivity)


def check_voxel_count(what, name, v):
    """a threshold in voxels: a non-negative integer below 2^31"""
    try:
        ok = not isinstance(v, bool) and int(v) == v and 0 <= int(v) < 1 << 31
    except (TypeError, ValueError, OverflowError):             # None, a string, inf, nan
        ok = False
    if not ok:
        raise ValueError('%s: %s = %r is not a non-negative voxel count' % (what, name, v))
    return int(v)


def _volumes_operand(what, t):
    """(tensor the labelling reads: uint8 or float32, contiguous -- bool viewed as uint8, uint8 and float32 as they are, any other float type as the uint8 map
    (t != 0), one extra pass, taken in the type itself so that no non-zero value rounds to 0; V, X, Y, Z) of a bool / uint8 / float mask [X, Y, Z] or [V, X, Y, Z]"""
    if torch.is_grad_enabled() and t.requires_grad:
        raise RuntimeError(what + ' is forward-only: call it under torch.no_grad() or on tensors without gradient')
    if t.dim() not in (3, 4):
        raise ValueError('%s: an [X, Y, Z] or [V, X, Y, Z] tensor, not rank %d' % (what, t.dim()))
    if not (t.dtype in (torch.bool, torch.uint8) or t.is_floating_point()):
        raise TypeError('%s: a bool, uint8 or float tensor, not %s' % (what, t.dtype))
    V, X, Y, Z = (1,) * (4 - t.dim()) + tuple(t.shape)
    if V < 1 or X < 1 or Y < 1 or Z < 1:
        raise ValueError('%s: empty tensor %s' % (what, tuple(t.shape)))
    if X * Y * Z >= segx.SegxLib.CCL_MAX_PLANE:
        raise ValueError('%s: X * Y * Z = %d is not below the limit of 2^30 voxels per volume' % (what, X * Y * Z))
    t = _c(t.detach())
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.is_floating_point() and t.dtype != torch.float32:
        t = (t != 0).view(torch.uint8)
    return t, V, X, Y, Z


def label_components3d(mask, connectivity=26):
    """6- or 26-connected components of every volume of a bool / uint8 / float mask [V, X, Y, Z] or [X, Y, Z] (segx_ccl3d; a bool, uint8 or float32 mask is read as
    it is, no conversion pass; another float type through one (mask != 0) pass); a voxel is set iff it is not 0.  Returns (labels, sizes), int32 of the mask's shape, with label_components' definitions: labels = 0 on the
    background, else 1 + the raster index inside the volume of the component's first voxel; sizes = the component's voxel count at that first voxel, 0 elsewhere."""
    conn = check_connectivity3d('label_components3d', connectivity)
    m, V, X, Y, Z = _volumes_operand('label_components3d', mask)
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    sizes = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    segx.lib().ccl3d(m, 0, labels, sizes, V, X, Y, Z, conn)
    return labels, sizes


def keep_components3d(labels, sizes, min_voxels=0, largest_only=False):
    """uint8 keep mask of label_components3d's (labels, sizes) (segx_cc3d_keep): 1 on the voxels of every component with size >= min_voxels that, with largest_only,
    is also the largest of its volume (ties: the one whose first voxel comes first in raster order); 0 elsewhere.  A volume without foreground keeps nothing."""
    nmin = check_voxel_count('keep_components3d', 'min_voxels', min_voxels)
    if labels.dim() not in (3, 4) or labels.shape != sizes.shape or labels.dtype != torch.int32 or sizes.dtype != torch.int32:
        raise ValueError('keep_components3d: labels %s and sizes %s must be int32 [X, Y, Z] or [V, X, Y, Z] tensors of one shape' % (tuple(labels.shape), tuple(sizes.shape)))
    labels, sizes = _c(labels), _c(sizes)
    V = labels.shape[0] if labels.dim() == 4 else 1
    S = labels.numel() // max(V, 1)
    if V < 1 or S < 1:
        raise ValueError('keep_components3d: empty tensor %s' % (tuple(labels.shape),))
    keep = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    stats = torch.empty(V, 2, dtype=torch.int32, device=labels.device)
    segx.lib().cc3d_keep(labels, sizes, stats, keep, V, S, nmin, largest_only)
    return keep


def remove_small_components3d(mask, min_voxels=0, largest_only=False, connectivity=26):
    """A NEW tensor of mask's shape and dtype: mask where keep_components3d(label_components3d(mask, connectivity), min_voxels, largest_only) is set, 0 elsewhere
    (segx_ccl3d, segx_cc3d_keep, segx_mask_apply)."""
    conn = check_connectivity3d('remove_small_components3d', connectivity)
    check_voxel_count('remove_small_components3d', 'min_voxels', min_voxels)
    m, V, X, Y, Z = _volumes_operand('remove_small_components3d', mask)
    labels, sizes = label_components3d(m, conn)
    keep = keep_components3d(labels, sizes, min_voxels, largest_only)
    src = _c(mask.detach())
    out = torch.empty_like(src)                                 # the mask's own dtype: the elements move bit for bit at their width
    segx.lib().mask_apply(src, keep, out, src.numel())
    return out


def brats_postprocess(hard, wt_min_voxels=0, wt_largest_only=False, et_min_voxels=0, connectivity=26, out=None, flag=None):
    """The BraTS post-processing rule on hard float32 [4, X, Y, Z] (background, ET, WT, TC -- brats_map_label's order -- as 0 / 1 floats):
      1. WT' = WT . keep_components3d(label_components3d(WT, connectivity), wt_min_voxels, wt_largest_only);  2. ET' = ET . WT', TC' = TC . WT';
      3. ET' = 0 if it has fewer than et_min_voxels voxels (TC stays);  4. background' = 1 exactly where ET' + WT' + TC' == 0.
    Returns (hard', flag): a new tensor (or `out`), hard itself is not modified; flag int32 [2] on the device = (voxel count of ET . WT', 1 iff ET was dropped),
    which brats_relabel reads.  With wt_min_voxels <= 1 and no wt_largest_only every WT component stays and no labelling runs."""
    what = 'brats_postprocess'
    conn = check_connectivity3d(what, connectivity)
    wt_min, et_min = check_voxel_count(what, 'wt_min_voxels', wt_min_voxels), check_voxel_count(what, 'et_min_voxels', et_min_voxels)
    _no_grad_operands(what, hard)
    if hard.dim() != 4 or hard.shape[0] != 4 or hard.dtype != torch.float32:
        raise ValueError('%s: hard %s %s must be a float32 [4, X, Y, Z] tensor (the 4-class BraTS task)' % (what, hard.dtype, tuple(hard.shape)))
    hard = _c(hard.detach())
    S = hard[0].numel()
    if S < 1:
        raise ValueError('%s: empty tensor %s' % (what, tuple(hard.shape)))
    if out is None:
        out = torch.empty_like(hard)
    elif out.dtype != torch.float32 or out.shape != hard.shape or not out.is_contiguous() or out.data_ptr() == hard.data_ptr():
        raise ValueError('%s: out is another contiguous float32 %s tensor' % (what, tuple(hard.shape)))
    if flag is None:
        flag = torch.empty(2, dtype=torch.int32, device=hard.device)
    elif flag.dtype != torch.int32 or tuple(flag.shape) != (2,):
        raise ValueError('%s: flag is an int32 [2] tensor' % what)
    keep = None
    if wt_min > 1 or wt_largest_only:
        labels, sizes = label_components3d(hard[2], conn)
        keep = keep_components3d(labels, sizes, wt_min, wt_largest_only)
    segx.lib().brats_postprocess(hard, keep, out, flag, S, et_min)
    return out, flag


def brats_relabel(labels, hard_pp, flag, out=None):
    """The export label volume (brats_case_tail's uint8 labels) after brats_postprocess: 0 where WT' (hard_pp[2]) is 0, a 4 becomes 1 where flag says ET was dropped.
    Returns a new tensor, or `out` (which may be labels itself)."""
    if labels.dtype != torch.uint8 or hard_pp.dim() < 2 or hard_pp.shape[0] != 4 or tuple(labels.shape) != tuple(hard_pp.shape[1:]) or hard_pp.dtype != torch.float32:
        raise ValueError('brats_relabel: labels uint8 %s do not match hard_pp float32 %s' % (tuple(labels.shape), tuple(hard_pp.shape)))
    labels, hard_pp = _c(labels), _c(hard_pp)
    if out is None:
        out = torch.empty_like(labels)
    elif out.dtype != torch.uint8 or out.shape != labels.shape or not out.is_contiguous():
        raise ValueError('brats_relabel: out is a contiguous uint8 %s tensor' % (tuple(labels.shape),))
    segx.lib().brats_relabel(labels, hard_pp[2], flag, out, labels.numel())
    return out


# -------------------------------------------------------------------------------------------------
# Lesion-wise evaluation (components.hip): dilation of the ground truth, the matching of predicted components to lesions and the per-lesion integer
# rows.  No copy to the host and no synchronisation, so the calls can be captured into a graph.  Forward only.
# -------------------------------------------------------------------------------------------------
DILATION_CONNECTIVITIES = (6, 18, 26)


def check_dilation(what, iters, connectivity):
    """(iters, connectivity) of a dilation: a non-negative iteration count and a structuring element of 6, 18 or 26 neighbours"""
    if connectivity not in DILATION_CONNECTIVITIES or isinstance(connectivity, bool):
        raise ValueError('%s: dilation connectivity %r is not 6, 18 or 26' % (what, connectivity))
    try:
        ok = not isinstance(iters, bool) and int(iters) == iters and 0 <= int(iters) < 1 << 15
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError('%s: dilation_iters = %r is not a non-negative iteration count' % (what, iters))
    return int(iters), int(connectivity)


def _gt_operand(what, gt, gt_map):
    """(tensor the kernels read, map code, V, X, Y, Z) of a ground truth: a mask stack as _volumes_operand takes it, or with gt_map='brats' ONE raw label volume
    [X, Y, Z] (any integer or float type, read as int32) that stands for the three regions ET, WT, TC"""
    if gt_map not in segx.SegxLib.LESION_MAPS:
        raise ValueError('%s: gt_map %r is not one of %s' % (what, gt_map, sorted(segx.SegxLib.LESION_MAPS, key=str)))
    if gt_map is None:
        m, V, X, Y, Z = _volumes_operand(what, gt)
        return m, 0, V, X, Y, Z
    if gt.dim() != 3 or gt.numel() < 1 or gt.dtype == torch.bool:
        raise ValueError("%s: gt_map='brats' takes one raw label volume [X, Y, Z], not %s %s" % (what, gt.dtype, tuple(gt.shape)))
    if gt.numel() >= segx.SegxLib.CCL_MAX_PLANE:
        raise ValueError('%s: X * Y * Z = %d is not below the limit of 2^30 voxels per volume' % (what, gt.numel()))
    g = _c(gt.detach())
    return (g if g.dtype == torch.int32 else g.to(torch.int32), segx.SegxLib.LESION_MAPS[gt_map], 3) + tuple(gt.shape)


def _dilate(what, g, gmap, V, X, Y, Z, iters, conn):
    out = torch.empty((V, X, Y, Z), dtype=torch.uint8, device=g.device)
    tmp = torch.empty_like(out) if iters >= 2 else None
    segx.lib().dilate3d(g, gmap, out, tmp, V, X, Y, Z, conn, iters)
    return out


def dilate3d(mask, iters=1, connectivity=18, gt_map=None):
    """uint8 0 / 1 of the mask's shape: a bool / uint8 / float mask [X, Y, Z] or [V, X, Y, Z] (set = not 0) dilated `iters` times by the 3 x 3 x 3 structuring element
    of the centre and its 6, 18 or 26 nearest neighbours (segx_dilate3d) -- scipy.ndimage.binary_dilation(mask, generate_binary_structure(3, 1 | 2 | 3), iters);
    outside the volume is unset.  iters = 0 gives the mask itself as bytes.  gt_map='brats': mask is one raw BraTS label volume, the result the [3, X, Y, Z] stack of
    its dilated ET, WT and TC regions."""
    iters, conn = check_dilation('dilate3d', iters, connectivity)
    g, gmap, V, X, Y, Z = _gt_operand('dilate3d', mask, gt_map)
    out = _dilate('dilate3d', g, gmap, V, X, Y, Z, iters, conn)
    return out[0] if mask.dim() == 3 and gt_map is None else out


def lesion_rows(pred, gt, *, gt_map=None, dilation_iters=3, dilation_connectivity=18, connectivity=26, out=None):
    """The device tables of the lesion-wise evaluation of a stack of binary regions, without reading them: (rows, header) with rows int32
    [V, LESION_MAX_GT, 4] = (root label, tp, gvol, pvol) per lesion in arbitrary order, zeros behind the last, and header int32 [V, LESION_HEADER] =
    (n_lesions, n_pred_components, n_fp, fp_voxels, overflow, 0, 0, 0).  pred, gt: bool / uint8 / float [V, X, Y, Z] or [X, Y, Z] (set = not 0); with
    gt_map='brats' gt is the raw label volume [X, Y, Z] and pred the [3, X, Y, Z] stack of ET, WT, TC (channels 1..3 of preds_hard).  The ground truth is dilated
    (segx_dilate3d), both maps are labelled (segx_ccl3d at `connectivity`), then segx_lesion_match and segx_lesion_reduce.  out = (rows, header): contiguous
    int32 tensors of those shapes to write into.  The inputs are not modified; infer3d.lesionwise_from_tables turns the tables into the metrics."""
    what = 'lesion_rows'
    iters, dconn = check_dilation(what, dilation_iters, dilation_connectivity)
    conn = check_connectivity3d(what, connectivity)
    p, V, X, Y, Z = _volumes_operand(what, pred)
    g, gmap, Vg, Xg, Yg, Zg = _gt_operand(what, gt, gt_map)
    if (V, X, Y, Z) != (Vg, Xg, Yg, Zg):
        raise ValueError('%s: pred %s and gt %s (gt_map %r) are not the same stack of regions' % (what, tuple(pred.shape), tuple(gt.shape), gt_map))
    L = segx.lib()
    shape = ((V, L.LESION_MAX_GT, 4), (V, L.LESION_HEADER))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32, device=p.device) for s in shape)
    elif len(out) != 2 or any(t.dtype != torch.int32 or tuple(t.shape) != s or not t.is_contiguous() for t, s in zip(out, shape)):
        raise ValueError('%s: out is a pair of contiguous int32 tensors %s and %s' % ((what,) + shape))
    rows, header = out
    gd = g if iters == 0 and gmap == 0 else _dilate(what, g, gmap, V, X, Y, Z, iters, dconn)         # no dilation of a plain mask: it is labelled as it is
    gl = torch.empty((V, X, Y, Z), dtype=torch.int32, device=p.device)
    gsizes, pl, psizes = torch.empty_like(gl), torch.empty_like(gl), torch.empty_like(gl)
    L.ccl3d(gd, 0, gl, gsizes, V, X, Y, Z, conn)
    L.ccl3d(p, 0, pl, psizes, V, X, Y, Z, conn)
    ws = torch.empty(L.lesion_ws_bytes(V), dtype=torch.uint8, device=p.device)
    L.lesion_match(g, gmap, gl, gsizes, pl, psizes, ws, V, X * Y * Z)
    L.lesion_reduce(ws, rows, header, V)
    return rows, header


def row_extent(mask, thres):
    """int32 [P, 2] (or [2] for one [H, W] plane): the lowest and the highest row index of each plane of the float mask that holds a value >= thres; (H, -1) where
    none does."""
    m, P, H, W = _planes_operand('row_extent', mask, (torch.float32,))
    ext = torch.empty(P, 2, dtype=torch.int32, device=m.device)
    segx.lib().row_extent(m, ext, P, H, W, thres)
    return ext if mask.dim() == 3 else ext[0]


_VALUE_TABLES = {}


def nhot_to_values(nhot, values):
    """uint8 [B, *spatial] from n-hot floats [B, C, *spatial]: 0, then for c ascending values[c] where nhot[:, c] == 1 -- a later class wins, as in the reference's
    inverse maps.  values: C ints in 0..255 (their device table is built once per device and kept: no host copy on later calls)."""
    if torch.is_grad_enabled() and nhot.requires_grad:
        raise RuntimeError('nhot_to_values is forward-only: call it under torch.no_grad() or on tensors without gradient')
    if nhot.dim() < 3:
        raise ValueError('nhot_to_values: [B, C, *spatial] floats, not rank %d' % nhot.dim())
    values = tuple(_uint8_value('nhot_to_values: values', v) for v in values)
    B, C = nhot.shape[:2]
    if len(values) != C:
        raise ValueError('nhot_to_values: %d values for %d classes' % (len(values), C))
    x = _c(nhot.detach().float())
    out = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device)
    if out.numel() == 0:
        raise ValueError('nhot_to_values: empty tensor %s' % (tuple(nhot.shape),))
    segx.lib().nhot_to_values(x, _value_table('nhot_to_values', values, C, x.device), out, B, C, out.numel() // B)
    return out


def _value_table(what, values, C, device):
    """the int32 [C] device table of C pixel values 0..255, built once per device and kept (the cache nhot_to_values fills)"""
    values = tuple(_uint8_value(what + ': values', v) for v in values)
    if len(values) != C:
        raise ValueError('%s: %d values for %d classes' % (what, len(values), C))
    key = (values, device)
    table = _VALUE_TABLES.get(key)
    if table is None:
        table = _VALUE_TABLES[key] = torch.tensor(values, dtype=torch.int32, device=device)
    return table


def _tail_output(what, name, given, want, shape, dtype, device):
    """an output of a tail launch: the caller's tensor (checked), a new one when wanted, else None"""
    if given is not None:
        if given.dtype != dtype or tuple(given.shape) != tuple(shape) or not given.is_contiguous() or given.device != device:
            raise ValueError('%s: %s is a contiguous %s %s tensor on %s' % (what, name, str(dtype).replace('torch.', ''), list(shape), device))
        return given
    return torch.empty(shape, dtype=dtype, device=device) if want else None


def nhot_case_tail(soft, gt=None, size=None, gt_map='nhot', values=None, T=0.5, want_extents=False, want_hard=False, counts=None, ext=None, labels=None,
                   hard=None):
    """The evaluation tail of an n-hot 2-D task (fundus, polyp) in one launch (segx_nhot_case_tail), one pass over the destination grid `size` = (H, W) (default: the
    ground truth's): soft float32 [B, C, h, w] as window_merge leaves it is resampled to it (interp_linear's values bit for bit; read as it is when the sizes agree)
    and hardened (harden_segmap mode 0, threshold T).  gt, in the form gt_map names, or None:
      'nhot': float32 [B, C, H, W] n-hot maps, class c on where the value >= 0.5 (what fundus_map_mask / polyp_map_mask return);
      'fundus' / 'fundus_exclusive': the raw uint8 mask [B, >= 2, H, W], mapped in registers as fundus_map_mask(mask, exclusive=False / True) (C == 3);
      'polyp': the raw uint8 mask [B, >= 1, H, W], mapped as polyp_map_mask (C == 2).
    Returns (counts, ext, labels, hard), None for what was not asked for:
      counts int32 [B, C - 1, 3] -- per image and foreground class {sum pred * gt, sum pred, sum gt}; formed whenever gt is given;
      ext int32 [B, 2, 2, 2] -- for {prediction, ground truth} x {class 1, class 2} the (lowest, highest) row holding the class, (H, -1) when empty: row_extent of
        the hardened and the ground-truth maps; with want_extents (needs gt);
      labels uint8 [B, H, W] -- nhot_to_values(hard, values); whenever `values` (C ints 0..255; the device table is built once per device and kept) is given;
      hard float32 [B, C, H, W] -- the hardened map at the destination size; with want_hard.
    counts / ext / labels / hard: tensors to write into (a captured graph passes its static ones); passing one asks for it.  No copy to the host, no synchronisation.
    Forward only."""
    what = 'nhot_case_tail'
    _no_grad_operands(what, soft, gt)
    if soft.dim() != 4 or soft.dtype != torch.float32:
        raise ValueError('%s: soft %s %s must be a float32 [B, C, h, w] tensor' % (what, soft.dtype, tuple(soft.shape)))
    B, C, h, w = soft.shape
    C = _class_count(what, C, low=2)
    if gt_map not in segx.SegxLib.NHOT_GT_MAPS:
        raise ValueError('%s: gt_map %r is not one of %s' % (what, gt_map, sorted(segx.SegxLib.NHOT_GT_MAPS)))
    if size is None:
        if gt is None:
            raise ValueError('%s: no gt and no size: the destination grid is unknown' % what)
        size = tuple(gt.shape[-2:])
    H, W = (int(v) for v in size)
    if B < 1 or h < 1 or w < 1 or H < 1 or W < 1:
        raise ValueError('%s: empty operand: soft %s, size %s' % (what, tuple(soft.shape), (H, W)))
    if H * W >= 1 << 31:
        raise ValueError('%s: H * W = %d is not below 2^31' % (what, H * W))
    soft = _c(soft.detach())
    dev = soft.device
    gt_channels = C
    if gt is None:
        if counts is not None or ext is not None or want_extents:
            raise ValueError('%s: counts and extents need gt' % what)
    else:
        if gt.dim() != 4 or gt.shape[0] != B or tuple(gt.shape[2:]) != (H, W):
            raise ValueError('%s: gt %s is no [%d, channels, %d, %d] tensor' % (what, tuple(gt.shape), B, H, W))
        gt_channels = int(gt.shape[1])
        if gt_map == 'nhot':
            if gt_channels != C or not gt.is_floating_point():
                raise ValueError('%s: an n-hot gt is a float [%d, %d, %d, %d] tensor, not %s %s' % (what, B, C, H, W, gt.dtype, tuple(gt.shape)))
            gt = _c(gt.detach().float())
        else:
            need_c, need_m = (2, 1) if gt_map == 'polyp' else (3, 2)
            if gt.dtype != torch.uint8 or gt_channels < need_m or C != need_c:
                raise ValueError('%s: a raw %s mask is uint8 with >= %d channels for %d classes, not %s %s for %d' %
                                 (what, gt_map, need_m, need_c, gt.dtype, tuple(gt.shape), C))
            gt = _c(gt.detach())
        counts = _tail_output(what, 'counts', counts, True, (B, C - 1, 3), torch.int32, dev)
        ext = _tail_output(what, 'ext', ext, want_extents, (B, 2, 2, 2), torch.int32, dev)
    table = None
    if values is None:
        if labels is not None:
            raise ValueError('%s: labels need values' % what)
    else:
        table = _value_table(what, values, C, dev)
        labels = _tail_output(what, 'labels', labels, True, (B, H, W), torch.uint8, dev)
    hard = _tail_output(what, 'hard', hard, want_hard, (B, C, H, W), torch.float32, dev)
    if counts is None and ext is None and labels is None and hard is None:
        raise ValueError('%s: nothing to compute (no gt, no values and want_hard=False)' % what)
    segx.lib().nhot_case_tail(soft, gt, segx.SegxLib.NHOT_GT_MAPS[gt_map], gt_channels, table, counts, ext, labels, hard, B, C, h, w, H, W, T)
    return counts, ext, labels, hard
