"""Fused loss + multi-tensor BertAdam kernels (csrc/train.hip) against fp64 references at the sizes where their loops split: slab, grid-stride
and chunk boundaries, saturated logits, soft masks, every loss argument, misaligned / inactive / more than 256 tensors.  Each test runs on the
fiber emulator and, under -m gpu, on the device (the `backend` fixture); two cases are device only (too many workgroups for the emulator)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from util import assert_close

F32, F64 = torch.float32, torch.float64


def _cpu_gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def _randn(shape, gen):
    return torch.randn(shape, generator=gen, device='cpu')


def _rand(shape, gen):
    return torch.rand(shape, generator=gen, device='cpu')


def _ulp(x):
    """one fp32 unit in the last place at magnitude x"""
    return float(np.spacing(np.float32(abs(x))))


# =====================================================================================================================================
# 1. loss
# =====================================================================================================================================
def ref_seg_loss(logits, mask, pos_weight, class_w, dice_w):
    """(1 - dice_w) * BCEWithLogits(pos_weight) + dice_w * sum_c class_w[c] * mean_b Dice_bc (smooth 1e-5), in the dtype of its arguments
    ([B, C, S] logits / mask).  Returns (loss, ce, dice_total, [dice_c for every c])."""
    ce = F.binary_cross_entropy_with_logits(logits.movedim(1, -1), mask.movedim(1, -1), pos_weight=pos_weight)
    sg = torch.sigmoid(logits)
    inter = (sg * mask).sum(-1)                                                        # [B, C]
    dice_bc = 1 - (2 * inter + 1e-5) / ((sg * sg).sum(-1) + (mask * mask).sum(-1) + 1e-5)
    dices = list(dice_bc.mean(0))
    dice_total = sum(d * class_w[c] for c, d in enumerate(dices))
    return (1 - dice_w) * ce + dice_w * dice_total, ce, dice_total, dices


def _trainer_class_w(C):
    cw = torch.ones(C, device='cpu'); cw[0] = 0
    return cw / cw.sum()


def _loss_inputs(B, C, S, seed, soft=False, saturate=False):
    g = _cpu_gen(seed)
    logits = 2.5 * _randn((B, C, S), g)
    if saturate:
        logits.view(-1)[::7] *= 40.0
    mask = _rand((B, C, S), g)
    if not soft:
        mask = (mask > 0.7).float()
    pw = 0.5 + 1.5 * _rand((C,), g)
    return logits, mask, pw


def test_fp64_loss_reference_equals_the_oracle():
    """The reference of this file restates O.seg_loss with an arbitrary class weight; on the trainer's weights (uniform, background 0) the two
    must be the same function: values to 1e-12, gradient to 1e-12 of its largest entry."""
    from oracle import segtran_oracle as O
    B, C, S = 2, 3, 4099
    logits, mask, pw = _loss_inputs(B, C, S, seed=11)
    with torch.device('cpu'):
        a = logits.double().requires_grad_(True)
        b = logits.double().requires_grad_(True)
        mine = ref_seg_loss(a, mask.double(), pw.double(), _trainer_class_w(C).double(), 0.5)
        theirs = O.seg_loss(b, mask.double(), pw.double(), 0.5)
        assert mine[0].dtype == F64 and theirs[0].dtype == F64
        for k in range(3):
            assert abs(float(mine[k]) - float(theirs[k])) < 1e-12, k
        assert len(theirs[3]) == C - 1                                                 # the oracle lists the foreground classes only
        for c in range(1, C):
            assert abs(float(mine[3][c]) - float(theirs[3][c - 1])) < 1e-12, c
        mine[0].backward(); theirs[0].backward()
        assert_close(a.grad, b.grad, 1e-12, 'reference gradient')


def _case(B, C, S, dev_only=False, **kw):
    return dict(B=B, C=C, S=S, dev_only=dev_only, **kw)


LOSS_CASES = [
    pytest.param(_case(1, 3, 1), id='S=1-63_empty_slabs'),
    pytest.param(_case(2, 2, 63), id='S=63-one_short_of_the_slab_count'),
    pytest.param(_case(1, 2, 64 * 257 + 5), id='S=16453-second_pass_of_a_slab-ragged_last_slab'),
    pytest.param(_case(1, 2, 262144 + 77), id='S=262221-backward_grid_stride-tail_block'),
    pytest.param(_case(2, 3, 16453, saturate=True), id='saturated_logits'),
    pytest.param(_case(2, 3, 4099, soft=True), id='soft_mask'),
    pytest.param(_case(2, 4, 4099, dice_w=0.0, upstream=2.5, weighted=True), id='dice_w=0.0-upstream_2.5-class_weights'),
    pytest.param(_case(2, 4, 4099, dice_w=0.3, upstream=2.5, weighted=True), id='dice_w=0.3-upstream_2.5-class_weights'),
    pytest.param(_case(2, 4, 4099, dice_w=1.0, upstream=2.5, weighted=True), id='dice_w=1.0-upstream_2.5-class_weights'),
    pytest.param(_case(5, 64, 37, dev_only=True), id='B*C=320-second_pass_of_the_plane_loop'),
]


@pytest.mark.parametrize('case', LOSS_CASES)
def test_seg_loss_vs_fp64_at_loop_boundaries(backend, case):
    """loss_stage1 / loss_stage2 / loss_bwd against ref_seg_loss in fp64; the bars are those of test_seg_loss_vs_reference (2e-6 absolute on the
    scalars, 2e-5 of max|dlogits| on the gradient).  Every per-class Dice value stats[3 + c] is compared, and everything must be finite.
    Largest errors seen: 6.1e-7 on the scalars on the emulator and on the device alike (saturated logits, loss 3.76), 6.5e-7 at B*C = 320 (device),
    2.8e-7 of max|dlogits| on the gradient (dice_w = 1) on both."""
    from segtran_amd import functional as SF
    B, C, S = case['B'], case['C'], case['S']
    if case['dev_only'] and backend.name == 'emu':
        pytest.skip('20 480 workgroups: minutes on the fiber emulator; runs on the device')
    dice_w, up = case.get('dice_w', 0.5), case.get('upstream', 1.0)
    logits, mask, pw = _loss_inputs(B, C, S, seed=B * 1000 + C * 100 + S % 97, soft=case.get('soft', False), saturate=case.get('saturate', False))
    if case.get('weighted'):
        cw = torch.tensor([0.15, 0.4, 0.05, 0.4][:C], device='cpu')                   # non-uniform, background counted
    else:
        cw = _trainer_class_w(C)
    if case.get('saturate'):
        assert logits.abs().max() > 300 and (logits > 100).any() and (logits < -100).any()    # far beyond where exp() overflows in fp32 (88.7)
    with torch.device('cpu'):
        l64 = logits.double().requires_grad_(True)
        want = ref_seg_loss(l64, mask.double(), pw.double(), cw.double(), dice_w)
        (up * want[0]).backward()
    dev = backend.dev
    lo = logits.to(dev).requires_grad_(True)
    loss, stats = SF.seg_loss(lo, mask.to(dev), pw.to(dev), cw.to(dev), dice_w)
    (up * loss).backward()
    assert stats.shape == (3 + C,)
    got = stats.detach().cpu().double()
    errs = [abs(loss.item() - float(want[0]))] + [abs(float(got[k]) - float(want[k])) for k in range(3)]
    errs += [abs(float(got[3 + c]) - float(want[3][c])) for c in range(C)]
    gerr = (lo.grad.cpu().double() - l64.grad).abs().max().item() / max(l64.grad.abs().max().item(), 1e-30)
    print('loss %s %s: loss %.6f, scalar err max %.2e, dlogits err %.2e of max' % (backend.name, (B, C, S), float(want[0]), max(errs), gerr))
    assert torch.isfinite(loss).all() and torch.isfinite(stats).all() and torch.isfinite(lo.grad).all()
    assert errs[0] < 2e-6 and errs[1] < 2e-6, ('loss', errs[:2])
    assert errs[2] < 2e-6, ('ce', errs[2])
    assert errs[3] < 2e-6, ('dice_total', errs[3])
    for c in range(C):
        assert errs[4 + c] < 2e-6, ('dice of class %d' % c, errs[4 + c])
    assert_close(lo.grad, l64.grad, 2e-5, 'dlogits')
    if case.get('saturate'):
        # where the sigmoid is saturated the Dice term vanishes and the BCE term is 0, +1 or -pos_weight times g * (1 - dice_w) / (B C S)
        sat = logits.abs() > 100
        k_ce = up * (1 - dice_w) / (B * C * S)
        expect = k_ce * torch.where(logits > 0, 1 - mask, -pw.view(1, C, 1) * mask)
        assert_close(lo.grad.cpu()[sat], expect[sat], 1e-6, 'saturated dlogits', scale=k_ce)
        assert set(torch.unique(expect[sat] == 0).tolist()) == {True, False}           # both kinds occur


def test_seg_loss_rejects_more_than_64_classes(backend):
    """loss_stage2 holds its per-class loop in one thread and the entry point requires C <= 64: C = 65 is an error before anything is launched
    (the output buffer keeps its sentinel)."""
    from segtran_amd import functional as SF, segx
    dev = backend.dev
    B, C, S = 1, 65, 4
    g = _cpu_gen(3)
    logits, mask = _randn((B, C, S), g).to(dev), (_rand((B, C, S), g) > 0.5).float().to(dev)
    pw, cw = torch.ones(C, device=dev), torch.full((C,), 1.0 / C, device=dev)
    with pytest.raises(RuntimeError, match='segx_seg_loss_fwd'):
        SF.seg_loss(logits, mask, pw, cw)
    L = segx.lib()
    out = torch.full((3 + C,), -7.0, device=dev)
    ws = torch.full((L.loss_ws(B, C),), -7.0, device=dev)
    with pytest.raises(RuntimeError, match='segx_seg_loss_fwd'):
        L.seg_loss_fwd(logits, mask, pw, cw, out, ws, B, C, S, 0.5)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert (out == -7.0).all() and (ws == -7.0).all()


# =====================================================================================================================================
# 2. BertAdam
# =====================================================================================================================================
WARMUP, T_TOTAL = 0.25, 8                     # schedule factor 0, 0.5, 1 in steps 0, 1, 2


def _chunk_sizes():
    from segtran_amd.optimization import CHUNK
    # multi-chunk, exactly one chunk, a 1-element last chunk, shorter than one float4, a float4 body with scalar tails of 1 (3C+5, C+1), 3 (7, C-1) and 2 elements
    return [3 * CHUNK + 5, CHUNK, CHUNK + 1, 7, CHUNK - 1, 2]


def _params(shapes, seed, dev, misaligned=()):
    g = _cpu_gen(seed)
    out = []
    for i, s in enumerate(shapes):
        n = int(np.prod(s))
        if i in misaligned:
            big = _randn(n + 8, g).to(dev)
            p = torch.nn.Parameter(big[1:1 + n])                                       # 4 bytes past a 16-byte boundary: no float4 access anywhere in this tensor
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(_randn(s, g).to(dev))
        out.append(p)
    return out


def _run_bertadam(backend, params, groups, scales, private, clip, max_grad_norm=0.05, inactive=(), steps=3, seed=0, both_clips=False, ctor=None):
    """`steps` optimizer steps on the kernels (through the BertAdam class) and on the oracle in fp64 and in fp32; after every step parameters and the
    global gradient norm are compared, after the last one the moments.  groups: [(indices into params, dict(lr=, weight_decay=))].
    Bar per tensor list: 4 * max|oracle32 - oracle64| + one fp32 ulp of the list's largest value.  Returns the worst (error, bar) pairs."""
    from segtran_amd.optimization import BertAdam
    from oracle import segtran_oracle as O
    dev = backend.dev
    if ctor is None:
        opt = BertAdam([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups], lr=groups[0][1]['lr'], warmup=WARMUP, t_total=T_TOTAL,
                       weight_decay=groups[0][1]['weight_decay'], max_grad_norm=max_grad_norm, global_grad_clip=clip)
    else:
        opt = ctor()
    if private:
        opt.release_flat_grads()
        assert all(p.grad is None for p in params)
    g0 = opt.param_groups[0]
    warmup, t_total = g0['warmup'], g0['t_total']
    order = [i for idx, _ in groups for i in idx]                                      # the optimizer's own numbering = group order
    assert sorted(order) == list(range(len(params)))
    active = [i for i in range(len(params)) if i not in inactive]
    p0 = [p.detach().clone() for p in params]
    ora = {dt: dict(p=[p.detach().cpu().to(dt).clone() for p in params], st=[dict() for _ in params]) for dt in (F64, F32)}
    gen = _cpu_gen(1000 + seed)
    worst = dict(gn=0.0)

    def compare(what, got, step):
        r64, r32 = [ora[F64][what][i] for i in active], [ora[F32][what][i] for i in active]
        e32 = max((a.double() - b).abs().max().item() for a, b in zip(r32, r64))       # the reference's own fp32 arithmetic
        bar = 4 * e32 + _ulp(max(b.abs().max().item() for b in r64))
        err = max((a.detach().cpu().double() - b).abs().max().item() for a, b in zip(got, r64))
        if what not in worst or err / bar > worst[what][0] / worst[what][1]:
            worst[what] = (err, bar)
        print('bertadam %s step %d %s: err %.3e, fp32 oracle %.3e, bar %.3e' % (backend.name, step, what, err, e32, bar))
        assert err <= bar, '%s after step %d: max err %.3e > %.3e' % (what, step, err, bar)

    for step in range(steps):
        opt.zero_grad()
        gs = {i: scales[i % len(scales)] * _randn(tuple(params[i].shape), gen) for i in active}
        sum((params[i] * gs[i].to(dev)).sum() for i in active).backward()
        if private:
            assert all(params[i].grad is None for i in inactive) and all(params[i].grad.data_ptr() != 0 for i in active)
        opt.step()
        with torch.device('cpu'):
            for dt, o in ora.items():
                grads = [gs[i].to(dt).clone() if i in gs else None for i in range(len(params))]
                act = [gr for gr in grads if gr is not None]
                if clip > 0:
                    total = O.global_clip_(act, clip)
                else:
                    total = torch.norm(torch.stack([gr.norm(2) for gr in act]), 2)
                if dt is F64 and both_clips:
                    norms = [float(gr.norm(2)) for gr in act]
                    assert max(norms) > 1.2 * max_grad_norm and min(norms) < 0.8 * max_grad_norm, 'the inputs must clip some tensors and spare others'
                for idx, kw in groups:
                    O.bertadam_step([o['p'][i] for i in idx], [grads[i] for i in idx], [o['st'][i] for i in idx], kw['lr'],
                                    [kw['weight_decay']] * len(idx), warmup, t_total, max_grad_norm=max_grad_norm)
                o['total'] = float(total)
        compare('p', [params[i] for i in active], step)
        gn, want = float(opt.grad_norm()), ora[F64]['total']
        worst['gn'] = max(worst['gn'], abs(gn - want) / want)
        assert abs(gn - want) <= 1e-5 * want, 'global gradient norm %r vs %r (step %d)' % (gn, want, step)
        for i in inactive:                                                             # no gradient: no update and no weight decay, bit for bit
            assert torch.equal(params[i].detach(), p0[i]), i
    st = opt.state_dict()['state']
    assert sorted(st) == [k for k, i in enumerate(order) if i not in inactive]
    for o in ora.values():
        o['m'] = [s.get('m') for s in o['st']]; o['v'] = [s.get('v') for s in o['st']]
    assert all(st[k]['step'] == steps for k in st)
    compare('m', [st[order.index(i)]['next_m'] for i in active], steps - 1)
    compare('v', [st[order.index(i)]['next_v'] for i in active], steps - 1)
    print('bertadam %s worst: %r' % (backend.name, worst))
    return worst


TWO_GROUPS = lambda: [([0, 1, 3], dict(lr=1e-3, weight_decay=1e-2)), ([2, 4, 5], dict(lr=4e-4, weight_decay=0.0))]     # noqa: E731  a multi-chunk tensor in each


@pytest.mark.parametrize('scales', [[1e-3, 1.0, 1e-6], [1.0, 1e-6, 1e-3]], ids=['one_chunk_tensors_clipped', 'multi_chunk_tensor_clipped'])
@pytest.mark.parametrize('private', [False, True], ids=['flat', 'private'])
def test_bertadam_chunk_boundaries_vs_fp64(backend, private, scales):
    """Tensors of 3 chunks + 5, exactly one chunk, one chunk + 1, 7, one chunk - 1 and 2 elements in two groups (different lr, one without decay);
    gradient scales (cycling over the tensors) that make the per-tensor clip bite on some tensors and not on others after the global clip.  With the first
    set the one-chunk tensors carry the norm and are clipped; with the second the three-chunk tensor does: its norm, summed over chunk_first[t] ..
    chunk_first[t + 1], decides the global norm and its own clip coefficient (with the first set it contributes 7e-7 of the global norm, so a sum over
    its first chunk alone would pass).
    Observed error / bar on the device (the emulator's figures agree to two digits): parameters 4.3e-7 / 2.2e-6 (the fp32 oracle's own error: 4.3e-7),
    m 1.5e-11 / 1.9e-10, v 2.8e-16 / 3.2e-15, global norm 4.7e-8 relative.  The other BertAdam tests of this file: parameters 2.3e-7 .. 4.6e-7 against
    bars of 1.1e-6 .. 2.3e-6; the cfg2 parameter list 2.4e-7 / 1.6e-6."""
    params = _params([(n,) for n in _chunk_sizes()], 21, backend.dev)
    _run_bertadam(backend, params, TWO_GROUPS(), scales, private, clip=0.1, both_clips=True, seed=1)


@pytest.mark.parametrize('private', [False, True], ids=['flat', 'private'])
def test_bertadam_misaligned_and_inactive_tensors_vs_fp64(backend, private):
    """The same sizes; tensors 0 and 2 start 4 bytes past a 16-byte boundary (the all-scalar branch of mt_bertadam_kernel over whole chunks) and
    tensor 3 never receives a gradient: it stays bit-equal, and its norm stays out of the global norm (private mode: a NULL gradient pointer in
    mt_sumsq_kernel)."""
    params = _params([(n,) for n in _chunk_sizes()], 22, backend.dev, misaligned=(0, 2))
    _run_bertadam(backend, params, TWO_GROUPS(), [1e-3, 1.0, 1e-6], private, clip=0.1, inactive=(3,), seed=2)


@pytest.mark.parametrize('clip', [0.1, 0.0], ids=['global_clip', 'no_global_clip'])
@pytest.mark.parametrize('private', [False, True], ids=['flat', 'private'])
def test_bertadam_more_than_256_tensors_vs_fp64(backend, private, clip):
    """300 tensors of 1..9 elements: the second pass of both per-tensor loops of mt_clipcoef_kernel."""
    n = 300
    params = _params([(1 + (i % 9),) for i in range(n)], 23, backend.dev)
    groups = [(list(range(0, n, 2)), dict(lr=1e-3, weight_decay=1e-2)), (list(range(1, n, 2)), dict(lr=4e-4, weight_decay=0.0))]
    _run_bertadam(backend, params, groups, [1e-2, 1.0], private, clip=clip, seed=3)


@pytest.mark.parametrize('private', [False, True], ids=['flat', 'private'])
def test_bertadam_without_clips_or_decay_vs_fp64(backend, private):
    """max_grad_norm = -1, weight_decay = 0, no global clip: plain Adam (without bias correction) on the chunk-boundary sizes.  The three-chunk tensor
    carries the reported global norm."""
    params = _params([(n,) for n in _chunk_sizes()], 24, backend.dev)
    groups = [([0, 1, 3], dict(lr=1e-3, weight_decay=0.0)), ([2, 4, 5], dict(lr=4e-4, weight_decay=0.0))]
    _run_bertadam(backend, params, groups, [1.0, 1e-3, 1e-6], private, clip=0.0, max_grad_norm=-1, seed=4)


def test_bertadam_model_shaped_list_vs_fp64(backend):
    """Device only: the parameter list of the cfg2 Segtran2d network (its real tensor count and largest tensor; no forward pass), fresh random values,
    flat gradients, the trainer's groups and defaults through engine.init_optimizer, 2 steps.  The schedule is shortened to t_total 8 / 2 warm-up steps:
    with init_optimizer's 10 000 / 500 the first two steps run at 0 and 4e-7 times lr and would not move a parameter by one ulp."""
    if backend.name == 'emu':
        pytest.skip('about 2 000 chunks (98 M parameters) per launch: minutes on the fiber emulator; runs on the device')
    from segtran_amd import engine
    dev = backend.dev
    c = dict(engine.CONFIGS['cfg2'], size=(64, 64))
    net = engine.build_model(c, dev, dropout_prob=0.0, attractors=32, synth=False)
    named = [(n, tuple(p.shape)) for n, p in net.named_parameters() if p.requires_grad]
    del net
    assert len(named) > 256 and max(int(np.prod(s)) for _, s in named) > 4 * 65536
    params = _params([s for _, s in named], 25, dev)

    class Shapes:                                          # what init_optimizer reads of a network
        def named_parameters(self):
            return [(n, p) for (n, _), p in zip(named, params)]
    holder = {}

    def ctor():
        holder['opt'] = engine.init_optimizer(Shapes(), 'fundus', t_total=T_TOTAL, warmup_steps=2)
        return holder['opt']
    lr, decay = engine.DEFAULTS['lr'], engine.DEFAULTS['decay']
    low = [i for i, (n, _) in enumerate(named) if 'backbone' in n]
    normal = [i for i, (n, _) in enumerate(named) if 'backbone' not in n]
    assert low and normal and not any('alphas' in n for n, _ in named)
    groups = [(normal, dict(lr=lr, weight_decay=decay)), (low, dict(lr=lr, weight_decay=decay * 0.1))]
    _run_bertadam(backend, params, groups, [1e-3, 1.0, 1e-6], False, clip=engine.DEFAULTS['grad_clip'], steps=2, seed=5, ctor=ctor)
    assert [len(g['params']) for g in holder['opt'].param_groups] == [len(normal), len(low), 0, 0]
