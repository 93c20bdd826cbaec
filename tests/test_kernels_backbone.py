"""backbone.hip kernels (BatchNorm+act, depthwise conv, squeeze-excite) vs plain PyTorch fp32 autograd.
Runs on the fiber emulator here and on the HIP build under -m gpu."""
import pytest
import torch
import torch.nn.functional as F
from segtran_amd import functional as SF
from segtran_amd.segx import Knob


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device='cpu') * scale).to(torch.get_default_device())


def close(a, b, tol=3e-5):
    s = max(b.abs().max().item(), 1e-20)
    err = (a - b).abs().max().item()
    assert err <= tol * s, 'err %.3e scale %.3e' % (err, s)


def _act(u, act):
    return u * torch.sigmoid(u) if act == 1 else F.relu(u) if act == 2 else u


# (1, 2, 130, 130): two reduction slabs per plane (statistics partials + folding apply pass); the others: the channel-resident forms (r04) -- one wave per
# channel with 1 / 2 float4 per lane and plane, the workgroup per channel with 1 / 2 / 4 -- and their limits (B > 8, S % 4 != 0, B = 7 at S = 4096 backward)
@pytest.mark.parametrize('shape', [(3, 5, 6, 10), (2, 4, 3, 4, 5), (2, 7, 8, 8), (1, 2, 130, 130), (6, 3, 16, 32), (5, 2, 32, 32), (3, 2, 40, 48),
                                   (6, 2, 64, 64), (7, 2, 64, 64), (9, 2, 8, 8), (2, 3, 11, 11), (8, 5, 16, 16)])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('training', [True, False])
def test_bn_act(backend, shape, act, training):
    C = shape[1]
    cls = torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm3d
    bn, ref = cls(C, eps=1e-3, momentum=0.01), cls(C, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        for m in (bn, ref):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=1)); m.bias.copy_(0.2 * rnd(C, seed=2))
            m.running_mean.copy_(0.1 * rnd(C, seed=3)); m.running_var.copy_(1 + 0.1 * rnd(C, seed=4).abs())
    bn.train(training); ref.train(training)
    x = (rnd(*shape, seed=5) * 1.7 + 0.4).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    y = SF.bn_act(x, bn, act)
    yr = _act(ref(xr), act)
    close(y, yr.detach())
    G = rnd(*shape, seed=6)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-4)
    close(bn.weight.grad, ref.weight.grad, 1e-4); close(bn.bias.grad, ref.bias.grad, 1e-4)
    close(bn.running_mean, ref.running_mean, 1e-5); close(bn.running_var, ref.running_var, 1e-5)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


@pytest.mark.parametrize('k,stride,pad,H,W', [(3, 1, (1, 1, 1, 1), 20, 18), (5, 1, (2, 2, 2, 2), 17, 33), (3, 2, (0, 1, 0, 1), 32, 32),
                                              (5, 2, (2, 2, 2, 2), 16, 16), (5, 2, (1, 2, 1, 2), 24, 40), (3, 2, (0, 1, 0, 1), 7, 9),
                                              (3, 1, (0, 2, 2, 0), 12, 40),           # lopsided pads: flipped-filter data gradient
                                              (3, 1, (1, 1, 1, 1), 37, 300),          # two column tiles (> 256 wide)
                                              (5, 2, (1, 2, 1, 2), 150, 140),         # several row tiles -> several wgrad strips
                                              (5, 1, (2, 2, 2, 2), 130, 64),
                                              (3, 2, (1, 1, 1, 1), 16, 24),           # float4 path, left pad 1 at stride 2
                                              (3, 1, (1, 1, 1, 1), 100, 128),         # float4 path, two wgrad strips
                                              (5, 2, (2, 2, 2, 2), 96, 256),
                                              (5, 2, (1, 2, 1, 2), 22, 40), (3, 2, (0, 1, 0, 1), 18, 600),    # ragged rows / 2 column tiles
                                              # r06, stride-1 'same': dx and dw from one pass (segx_dwconv2d_bwd_fused) -- 4 / 2 / 1 row groups per wave, ragged last rows
                                              (5, 1, (2, 2, 2, 2), 64, 64), (3, 1, (1, 1, 1, 1), 32, 128), (5, 1, (2, 2, 2, 2), 24, 256), (3, 1, (1, 1, 1, 1), 20, 256)])
def test_dwconv2d(backend, k, stride, pad, H, W):
    B, C = (2, 5) if H * W < 4000 else (2, 2)
    if (k, stride, H, W) in ((5, 1, 64, 64), (3, 1, 32, 128), (5, 1, 24, 256), (3, 1, 20, 256), (3, 1, 37, 300)):
        assert backend.L.dwconv2d_bwd_fused_rows(H, W, H, W, k, stride, pad[2], pad[0]) > 0
    x = rnd(B, C, H, W, seed=7).requires_grad_(True)
    w = rnd(C, 1, k, k, seed=8).requires_grad_(True)
    y = SF.dwconv2d(x, w, stride, pad)
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    yr = F.conv2d(F.pad(xr, pad), wr, None, stride, 0, 1, C)
    assert y.shape == yr.shape
    close(y, yr.detach())
    G = rnd(*y.shape, seed=9)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-4); close(w.grad, wr.grad, 1e-4)


@pytest.mark.parametrize('B,C,Cs,H,W', [(3, 12, 4, 9, 7), (2, 70, 9, 4, 5), (1, 3, 2, 130, 130), (6, 9, 3, 32, 32), (6, 5, 2, 16, 24), (2, 300, 70, 4, 5)])      # third: several chunks per plane; last: Cs > one wave
@pytest.mark.parametrize('training', [True, False])
def test_bn_act_squeeze_excite_fused(backend, B, C, Cs, H, W, training):
    """The one-op form an MBConv block uses (BatchNorm + swish with the squeeze-excite pooling in the same pass, the gate's product rule applied
    inside the BatchNorm backward kernels) vs BatchNorm -> swish -> squeeze-excite in plain PyTorch autograd."""
    bn, ref = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01), torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        for m in (bn, ref):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=1)); m.bias.copy_(0.2 * rnd(C, seed=2))
            m.running_mean.copy_(0.1 * rnd(C, seed=3)); m.running_var.copy_(1 + 0.1 * rnd(C, seed=4).abs())
    bn.train(training); ref.train(training)
    x = (rnd(B, C, H, W, seed=20) * 1.3 + 0.2).requires_grad_(True)
    ps = [rnd(Cs, C, 1, 1, seed=21, scale=0.5), rnd(Cs, seed=22, scale=0.1), rnd(C, Cs, 1, 1, seed=23, scale=0.5), rnd(C, seed=24, scale=0.1)]
    ps = [p.requires_grad_(True) for p in ps]
    z = SF.bn_act_se(x, bn, SF.ACT_SWISH, *ps)
    xr = x.detach().clone().requires_grad_(True)
    pr = [p.detach().clone().requires_grad_(True) for p in ps]
    yr = _act(ref(xr), 1)
    sq = F.conv2d(F.adaptive_avg_pool2d(yr, 1), pr[0], pr[1]); sq = sq * torch.sigmoid(sq)
    zr = torch.sigmoid(F.conv2d(sq, pr[2], pr[3])) * yr
    close(z, zr.detach())
    G = rnd(B, C, H, W, seed=25)
    z.backward(G); zr.backward(G)
    close(x.grad, xr.grad, 1e-4)
    close(bn.weight.grad, ref.weight.grad, 1e-4); close(bn.bias.grad, ref.bias.grad, 1e-4)
    for a, r in zip(ps, pr):
        close(a.grad, r.grad, 1e-4)
    close(bn.running_mean, ref.running_mean, 1e-5); close(bn.running_var, ref.running_var, 1e-5)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


@pytest.mark.parametrize('B,C,Cs,Co,H,W', [(3, 12, 4, 10, 9, 7), (2, 70, 9, 24, 4, 5), (2, 8, 2, 136, 12, 12), (2, 150, 70, 7, 3, 4)])   # last: 3 gate chunks, Cs > one wave
@pytest.mark.parametrize('training', [True, False])
def test_se_gate_folded_into_projection_weights(backend, B, C, Cs, Co, H, W, training):
    """MBConv tail as the product runs it: BatchNorm + swish with the squeeze-excite gate from the same pass, written straight into per-sample projection
    weights W * gate[b] (bn_act_gate_weights), then the projection as a pointwise convolution with those (conv1x1_per_sample) -- against
    BatchNorm -> swish -> squeeze-excite -> conv in PyTorch."""
    bn, ref = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01), torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        for m in (bn, ref):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=1)); m.bias.copy_(0.2 * rnd(C, seed=2))
            m.running_mean.copy_(0.1 * rnd(C, seed=3)); m.running_var.copy_(1 + 0.1 * rnd(C, seed=4).abs())
    bn.train(training); ref.train(training)
    x = (rnd(B, C, H, W, seed=30) * 1.3 + 0.2).requires_grad_(True)
    ps = [rnd(Cs, C, 1, 1, seed=31, scale=0.5), rnd(Cs, seed=32, scale=0.1), rnd(C, Cs, 1, 1, seed=33, scale=0.5), rnd(C, seed=34, scale=0.1),
          rnd(Co, C, 1, 1, seed=35, scale=0.3)]
    ps = [p.requires_grad_(True) for p in ps]
    y, Wb = SF.bn_act_gate_weights(x, bn, SF.ACT_SWISH, *ps)
    out = SF.conv1x1_per_sample(y, Wb)
    xr = x.detach().clone().requires_grad_(True)
    pr = [p.detach().clone().requires_grad_(True) for p in ps]
    yr = _act(ref(xr), 1)
    sq = F.conv2d(F.adaptive_avg_pool2d(yr, 1), pr[0], pr[1]); sq = sq * torch.sigmoid(sq)
    outr = F.conv2d(torch.sigmoid(F.conv2d(sq, pr[2], pr[3])) * yr, pr[4])
    close(out, outr.detach())
    G = rnd(B, Co, H, W, seed=36)
    out.backward(G); outr.backward(G)
    close(x.grad, xr.grad, 1e-4)
    close(bn.weight.grad, ref.weight.grad, 1e-4); close(bn.bias.grad, ref.bias.grad, 1e-4)
    for a, r in zip(ps, pr):
        close(a.grad, r.grad, 1e-4)
    close(bn.running_mean, ref.running_mean, 1e-5); close(bn.running_var, ref.running_var, 1e-5)


@pytest.mark.parametrize('shape', [(6, 5, 6, 10), (5, 3, 36, 36), (4, 2, 130, 130), (6, 2, 64, 64), (6, 6, 16, 16)])
@pytest.mark.parametrize('rate', [0.0, 0.5])
@pytest.mark.parametrize('training', [True, False])
def test_bn_with_skip_add_and_drop_connect(backend, shape, rate, training):
    """The tail of an MBConv block in one pass (efficientnet/model.py:116-122): y = bn(x) * drop_connect scale of the sample + inputs.  The scale is
    drawn inside the kernel (0 or 1 / keep per sample); it is recovered from the output and must then explain the output AND every gradient:
    forward and backward regenerate the same draw, the skip input's gradient is the incoming one."""
    B, C = shape[:2]
    bn, ref = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01), torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        for m in (bn, ref):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=1)); m.bias.copy_(0.2 * rnd(C, seed=2))
            m.running_mean.copy_(0.1 * rnd(C, seed=3)); m.running_var.copy_(1 + 0.1 * rnd(C, seed=4).abs())
    bn.train(training); ref.train(training)
    x = (rnd(*shape, seed=40) * 1.7 + 0.4).requires_grad_(True)
    r = rnd(*shape, seed=41).requires_grad_(True)
    SF.manual_seed(77)
    y = SF.bn_act(x, bn, SF.ACT_NONE, resid=r, drop_connect=rate if training else 0.0)
    xr, rr = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
    br = ref(xr)
    keep = 1.0 - rate
    with torch.no_grad():          # per-sample scale recovered from the first element of each sample
        scale = ((y - r).reshape(B, -1)[:, 0] / br.reshape(B, -1)[:, 0]).detach()
    if rate == 0.0 or not training:
        assert torch.allclose(scale, torch.ones(B), atol=1e-4)
        scale = torch.ones(B)
    else:
        assert all(abs(v) < 1e-4 or abs(v - 1 / keep) < 1e-3 for v in scale.tolist()), scale
        scale = torch.where(scale.abs() < 0.5, torch.zeros(B), torch.full((B,), 1 / keep))
    yr = br * scale.view(B, 1, 1, 1) + rr
    close(y, yr.detach())
    G = rnd(*shape, seed=42)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-4); close(r.grad, rr.grad, 1e-6)
    close(bn.weight.grad, ref.weight.grad, 1e-4); close(bn.bias.grad, ref.bias.grad, 1e-4)
    close(bn.running_mean, ref.running_mean, 1e-5); close(bn.running_var, ref.running_var, 1e-5)


@pytest.mark.parametrize('path,shape', [(p_, s_) for p_ in (1, 2) for s_ in [(3, 5, 6, 10), (2, 3, 130, 132), (6, 2, 64, 64), (2, 4, 3, 4, 5)]] +
                         [(0, (6, 2, 320, 320))])    # default policy on a plane of 102400: forward teams of 6 x 4 workgroups with 32 float4 per lane, backward 6 x 7 with 16
def test_bn_forms_team_and_two_launch(backend, path, shape):
    """segx_tune knob 3.  2 = the TEAM form on every shape (a team of B x chunks workgroups per channel keeps the channel in registers across a team
    barrier -- on the emulator a block that waits for its mates is parked while later blocks run): one chunk per plane on the small shapes, two on
    130 x 132; 1 = never teams (130 x 132 then takes the two-launch form the default no longer reaches).  Plain / relu / swish, the skip + drop_connect
    tail and the squeeze-excite pooling variant must all match PyTorch in forward, backward and running statistics."""
    L = backend.L
    assert L.c.segx_tune(Knob.BN_PATH, 7) < 0           # unknown settings are refused
    with L.tuned(bn_path=path):
        for act in (0, 1, 2):
            test_bn_act.__wrapped__(backend, shape, act, True) if hasattr(test_bn_act, '__wrapped__') else test_bn_act(backend, shape, act, True)
        if len(shape) == 4:
            test_bn_with_skip_add_and_drop_connect(backend, shape, 0.5, True)
            B, C, H, W = shape
            test_bn_act_squeeze_excite_fused(backend, B, C, 2, H, W, True)


@pytest.mark.parametrize('fill', ['ones_bits', 'small_ints', 'previous_call'])
def test_team_exchange_ignores_what_its_buffers_held(backend, fill):
    """The team exchange marks its slots and mailboxes with a per-launch tag and zeroes nothing (common.h: team_exchange), so its scratch may hold anything:
    all-ones bits, small int64 values (what recycled memory often holds -- sequential tags once matched them), or the words a previous call left behind.
    Forward and backward results must equal, bit for bit, those computed with zero-filled scratch."""
    L = backend.L
    B, C, S = 2, 3, 130 * 132                                # two chunks per plane: teams of four workgroups
    x, dy = rnd(B, C, S, seed=70) * 1.5 + 0.3, rnd(B, C, S, seed=71)
    w, b = 1 + 0.2 * rnd(C, seed=72), 0.2 * rnd(C, seed=73)
    npf, nws = L.bn_parts_floats(B, C, S), L.bn_ws(B, C, S)

    def run(parts, ws):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, var, dw, db = (torch.empty(C, device=x.device) for _ in range(4))
        L.bn_act_fwd2(x, parts, 0, mean, var, None, None, 0.0, w, b, y, None, None, 0.0, 0, 0, B, C, S, 1e-3, 1)
        L.bn_act_bwd2(dy, x, mean, var, w, b, dx, dw, db, ws, B, C, S, 1e-3, 1, 1)
        return y, mean, var, dx, dw, db

    ref = run(torch.zeros(npf, device=x.device), torch.zeros(nws, device=x.device))
    if fill == 'ones_bits':
        parts = torch.full((npf,), -1, dtype=torch.int32, device=x.device).view(torch.float32)
        ws = torch.full((nws,), -1, dtype=torch.int32, device=x.device).view(torch.float32)
    elif fill == 'small_ints':
        parts = (torch.arange(npf // 2 + 1, device=x.device, dtype=torch.int64) % 7).view(torch.float32)[:npf].clone()
        ws = (torch.arange(nws // 2 + 1, device=x.device, dtype=torch.int64) % 5).view(torch.float32)[:nws].clone()
    else:
        parts, ws = torch.zeros(npf, device=x.device), torch.zeros(nws, device=x.device)
        run(parts, ws)                                       # leaves its words behind; the next call gets a new tag
    out = run(parts, ws)
    for a, r in zip(out, ref):
        assert torch.equal(a, r)


def _team_case(dev, seed=80, B=2, C=3, S=130 * 132):
    x, dy = rnd(B, C, S, seed=seed) * 1.5 + 0.3, rnd(B, C, S, seed=seed + 1)
    w, b = 1 + 0.2 * rnd(C, seed=seed + 2), 0.2 * rnd(C, seed=seed + 3)
    return x, dy, w, b


def _team_run(L, x, dy, w, b, act=1, run=None):
    B, C, S = x.shape
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, var, dw, db = (torch.empty(C, device=x.device) for _ in range(4))
    parts, ws = torch.zeros(L.bn_parts_floats(B, C, S), device=x.device), torch.zeros(L.bn_ws(B, C, S), device=x.device)
    L.bn_act_fwd2(x, parts, 0, mean, var, run[0] if run else None, run[1] if run else None, 0.1 if run else 0.0, w, b, y, None, None, 0.0, 0, 0, B, C, S, 1e-3, act)
    L.bn_act_bwd2(dy, x, mean.nan_to_num(0.0), var.nan_to_num(1.0), w, b, dx, dw, db, ws, B, C, S, 1e-3, act, 1)
    if x.is_cuda:
        torch.cuda.synchronize()
    return y, mean, var, dx, dw, db


def test_team_exchange_that_times_out_fails_loudly(backend):
    """VERDICT r04 weak 7 / ADVICE r04: a team whose members are not all running must not hand back plausible numbers.  Fault injection (segx_tune knob 13)
    leaves the LAST workgroup of the team grid unlaunched -- a team larger than the grid -- with a short poll bound (knob 12): member 0 of the last channel
    gives up on the missing mate, adds to the process's error word and posts NaN to the members that did arrive.  Expected: the other channels are exact,
    the last channel's statistics / outputs / gradients are NaN, segx_team_status counts the timeouts, team_check() raises (and clears), BertAdam.step()
    raises through it, and the next clean launch is right again with a zero status."""
    L = backend.L
    x, dy, w, b = _team_case(backend.dev)
    B, C, S = x.shape
    assert L.team_cap() >= 4
    L.c.segx_team_status(1)
    ref = _team_run(L, x, dy, w, b)
    assert L.c.segx_team_status(0) == 0
    assert L.c.segx_tune(Knob.TEAM_SPIN, 16) < 0 and L.c.segx_tune(Knob.TEAM_DROP, -1) < 0 and L.c.segx_tune(Knob.TEAM_DROP, 5000) < 0          # out-of-range settings are refused
    try:
        with L.tuned(team_spin=64, team_drop=1):
            y, mean, var, dx, dw, db = _team_run(L, x, dy, w, b)
            n = L.c.segx_team_status(0)
            assert n >= 2                                          # forward AND backward launch of the last channel's team
            assert torch.equal(mean[:C - 1], ref[1][:C - 1]) and torch.equal(y[:, :C - 1], ref[0][:, :C - 1]) and torch.equal(dx[:, :C - 1], ref[3][:, :C - 1])
            assert torch.isnan(mean[C - 1]) and torch.isnan(var[C - 1]) and torch.isnan(dw[C - 1]) and torch.isnan(db[C - 1])
            chunk = 1024 * 16                                      # floats per member (16 float4 per lane); the unlaunched member owns the last chunk of the last plane
            assert torch.isnan(y[:, C - 1].reshape(-1)[:B * S - (S - chunk)]).all() and torch.isnan(dx[0, C - 1]).all()
            with pytest.raises(RuntimeError, match='team exchange'):
                L.team_check()
            assert L.c.segx_team_status(0) == 0                    # team_check cleared the word
            # the failed exchange must not reach the RUNNING statistics (a checkpoint written after the RuntimeError would keep them)
            rm, rv = torch.zeros(C, device=x.device), torch.ones(C, device=x.device)
            _team_run(L, x, dy, w, b, run=(rm, rv))
            assert L.c.segx_team_status(1) >= 2
            assert torch.isfinite(rm).all() and torch.isfinite(rv).all() and rm[C - 1] == 0 and rv[C - 1] == 1 and (rm[:C - 1] != 0).all()
            # the training loop's hook: BertAdam.step() checks the word before it touches the weights
            _team_run(L, x, dy, w, b)
            from segtran_amd.optimization import BertAdam
            p = torch.nn.Parameter(torch.ones(8, device=x.device)); p.grad = torch.ones(8, device=x.device)
            opt = BertAdam([p], lr=1e-3, warmup=-1, t_total=-1)
            with pytest.raises(RuntimeError, match='team exchange'):
                opt.step()
            assert torch.equal(p.detach(), torch.ones(8, device=x.device))
    finally:
        L.c.segx_team_status(1)
    out = _team_run(L, x, dy, w, b)
    for a, r in zip(out, ref):
        assert torch.equal(a, r)
    assert L.c.segx_team_status(0) == 0


def test_bn_launch_refuses_a_buffer_sized_under_another_knob_setting(backend):
    """the team / resident / two-launch form is re-derived at the launch from knob 3; a buffer sized under another setting must be refused,
    not overrun.  Plane of 130 x 132: knob 3 = 1 sizes the slab partials (small), the default launches the team form (slots + mailboxes)."""
    L = backend.L
    B, C, S = 2, 64, 130 * 132
    x = rnd(B, C, S, seed=90)
    w, b = torch.ones(C), torch.zeros(C)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, var, dw, db = (torch.empty(C, device=x.device) for _ in range(4))
    with L.tuned(bn_path=1):
        small_p, small_w = L.bn_parts_floats(B, C, S), L.bn_ws(B, C, S)
    need_p, need_w = L.bn_parts_floats(B, C, S), L.bn_ws(B, C, S)
    assert small_p < need_p and small_w < need_w
    with pytest.raises(RuntimeError, match='partials buffer holds'):
        L.bn_act_fwd2(x, torch.zeros(small_p), 0, mean, var, None, None, 0.0, w, b, y, None, None, 0.0, 0, 0, B, C, S, 1e-3, 0)
    L.bn_act_fwd2(x, torch.zeros(need_p), 0, mean, var, None, None, 0.0, w, b, y, None, None, 0.0, 0, 0, B, C, S, 1e-3, 0)
    with pytest.raises(RuntimeError, match='scratch holds'):
        L.bn_act_bwd2(x, x, mean, var, w, b, dx, dw, db, torch.zeros(small_w), B, C, S, 1e-3, 0, 1)
    L.bn_act_bwd2(x, x, mean, var, w, b, dx, dw, db, torch.zeros(need_w), B, C, S, 1e-3, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('spin', [1 << 20, 256])
@pytest.mark.parametrize('hog', ['all_cus_80kb_lds', 'most_cus_80kb_lds', 'light'])
def test_team_batchnorm_next_to_a_kernel_that_holds_the_compute_units(hog, spin):
    """The team exchange needs its members co-resident; a kernel on ANOTHER stream that holds compute units (what RCCL's reduction kernels do under an
    overlapped all-reduce) delays or shrinks the residency window.  segx_occupy holds `wgs` workgroups (80 KB of LDS each: nothing that needs LDS fits
    beside two of them on a CU) for 30 ms on a side stream while team BatchNorm layers (teams of 42 / 24 / 12 workgroups, the cfg2 shapes) run on
    the main stream.  The property: with the default poll bound (~1 s) the results are bit-identical to the undisturbed run and no timeout is
    recorded; with a bound of 256 polls the exchange MAY expire -- then the error word says so and the statistics are NaN: wrong numbers with a zero
    status never happen."""
    from segtran_amd import segx
    L = segx.lib()
    dev = torch.device('cuda', 0)
    prev = torch.get_default_device(); torch.set_default_device(dev)
    try:
        cases = [_team_case(dev, seed=100, B=6, C=24, S=320 * 320), _team_case(dev, seed=110, B=6, C=48, S=128 * 128), _team_case(dev, seed=120, B=2, C=96, S=130 * 132)]
        L.c.segx_team_status(1)
        refs = [_team_run(L, *c) for c in cases]
        assert L.c.segx_team_status(0) == 0
        side = torch.cuda.Stream()
        wgs = {'all_cus_80kb_lds': 512, 'most_cus_80kb_lds': 480, 'light': 2048}[hog]
        try:
            with L.tuned(team_spin=spin):
                for rep in range(3):
                    with torch.cuda.stream(side):
                        L.check(L.c.segx_occupy(wgs, 0 if hog == 'light' else 1, 30.0, None, L.stream(cases[0][0])), 'segx_occupy')
                    outs = [_team_run(L, *c) for c in cases]
                    torch.cuda.synchronize()
                    n = L.c.segx_team_status(1)
                    exact = all(torch.equal(a, r) for o, rf in zip(outs, refs) for a, r in zip(o, rf))
                    if spin == 1 << 20:
                        assert n == 0 and exact, (hog, n, exact)
                    else:
                        poisoned = any(bool(torch.isnan(o[1]).any()) or bool(torch.isnan(o[4]).any()) for o in outs)
                        assert (n == 0 and exact) or (n > 0 and poisoned), (hog, n, exact, poisoned)
        finally:
            torch.cuda.synchronize()
            L.c.segx_team_status(1)
    finally:
        torch.set_default_device(prev)


def test_drop_connect_draws_differ_between_calls_and_follow_the_seed(backend):
    B, C = 16, 2
    bn = torch.nn.BatchNorm2d(C).train()
    x, r = rnd(B, C, 4, 4, seed=50), torch.zeros(B, C, 4, 4)

    def draw():
        with torch.no_grad():
            y = SF.bn_act(x, bn, SF.ACT_NONE, resid=r, drop_connect=0.5)
        return (y.reshape(B, -1).abs().sum(1) > 0)
    SF.manual_seed(5); a1, a2 = draw(), draw()
    SF.manual_seed(5); b1 = draw()
    assert torch.equal(a1, b1) and not torch.equal(a1, a2)
    assert 0 < int(a1.sum()) + int(a2.sum()) < 2 * B          # some samples kept, some dropped


@pytest.mark.parametrize('shape', [(2, 16, 6, 10), (3, 8, 3, 4, 5), (1, 24, 9, 9)])
def test_group_norm(backend, shape):
    C = shape[1]
    gn, ref = torch.nn.GroupNorm(8, C), torch.nn.GroupNorm(8, C)
    with torch.no_grad():
        for m in (gn, ref):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=1)); m.bias.copy_(0.2 * rnd(C, seed=2))
    x = (rnd(*shape, seed=3) * 1.3 + 0.7).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    y = SF.group_norm(x, gn); yr = ref(xr)
    close(y, yr.detach())
    G = rnd(*shape, seed=4)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-4); close(gn.weight.grad, ref.weight.grad, 1e-4); close(gn.bias.grad, ref.bias.grad, 1e-4)



def test_group_norm_backward_also_returns_the_plane_sums_of_its_input_gradient(backend):
    """segx_groupnorm_bwd(plane_dx_sums): sum over every (sample, channel) plane of dX in closed form from the plane sums (no extra pass) == dX summed."""
    L = backend.L
    B, C, G, S = 3, 16, 4, 6 * 10 * 7
    x, dy = rnd(B, C, S, seed=30) * 1.4 + 0.6, rnd(B, C, S, seed=31)
    w, b = 1 + 0.3 * rnd(C, seed=32), 0.2 * rnd(C, seed=33)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(B * G), torch.empty(B * G)
    L.groupnorm_fwd(x, w, b, y, mean, rstd, torch.empty(L.gn_ws(B, C, G)), B, C, G, S, 1e-5)
    dw, db, rs = torch.empty(C), torch.empty(C), torch.full((B * C,), float('nan'))
    L.groupnorm_bwd(dy, x, w, mean, rstd, dx, dw, db, torch.empty(L.gn_ws(B, C, G)), B, C, G, S, rs)
    ref = dx.double().sum(dim=2).reshape(-1)
    assert float((rs.double() - ref).abs().max()) <= 2e-5 * float(dx.abs().sum(dim=2).max())        # plane sums cancel: compare against the planes' absolute mass
    dx2 = torch.empty_like(x)
    L.groupnorm_bwd(dy, x, w, mean, rstd, dx2, dw, db, torch.empty(L.gn_ws(B, C, G)), B, C, G, S)       # without the extra output: same dX
    assert torch.equal(dx, dx2)


# (d, h, w) -> (D, H, W) with D * H * W / 4 a multiple of 256 (whole 1024-float chunks per plane: the fused form); the last case is not (falls back to the two ops)
@pytest.mark.parametrize('B,C,G,insize,size', [(2, 8, 4, (4, 8, 8), (8, 16, 16)), (1, 16, 8, (2, 8, 16), (4, 16, 32)), (2, 8, 2, (8, 4, 4), (16, 8, 16)),
                                               (2, 8, 4, (8, 8, 8), (8, 16, 16)), (1, 8, 2, (4, 4, 32), (4, 16, 32)),      # depth (and width) not resized: the out_gn2b level

                                               (1, 8, 4, (3, 5, 6), (6, 10, 12))])
def test_up_group_norm_fused_level_matches_the_two_ops_and_feeds_the_bias_gradient(backend, B, C, G, insize, size):
    """SF.up_group_norm (r05): gn(trilinear-up(x) + conv1x1(f)) with the GroupNorm partials produced by the resampling pass and the lateral convolution's
    bias gradient taken from the backward's plane sums.  Against PyTorch (F.interpolate + nn.GroupNorm + nn.Conv3d): outputs and EVERY gradient -- x, the
    lateral's input, weight and bias, the GroupNorm affine -- and the row-sum kernel must not have been launched on the fused path."""
    L = backend.L
    Cf = 6
    gn, ref_gn = torch.nn.GroupNorm(G, C), torch.nn.GroupNorm(G, C)
    conv = torch.nn.Conv3d(Cf, C, 1)
    with torch.no_grad():
        for m in (gn, ref_gn):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=41)); m.bias.copy_(0.2 * rnd(C, seed=42))
        conv.weight.copy_(0.4 * rnd(C, Cf, 1, 1, 1, seed=43)); conv.bias.copy_(0.3 * rnd(C, seed=44))
    x = (rnd(B, C, *insize, seed=45) + 0.5).requires_grad_(True)
    f = rnd(B, Cf, *size, seed=46).requires_grad_(True)
    xr, fr = x.detach().clone().requires_grad_(True), f.detach().clone().requires_grad_(True)
    wr, br = conv.weight.detach().clone().requires_grad_(True), conv.bias.detach().clone().requires_grad_(True)
    from segtran_amd import segx
    Lf = segx.lib()                                            # the instance the autograd layer calls (on the device not the fixture's object)
    calls = []
    orig = Lf.rowsum
    Lf.rowsum = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        y = SF.up_group_norm(x, size, SF.conv1x1(f, conv.weight, conv.bias), gn)
        Gd = rnd(*y.shape, seed=47)
        y.backward(Gd)
    finally:
        del Lf.rowsum
    yr = ref_gn(F.interpolate(xr, size=size, mode='trilinear', align_corners=False) + F.conv3d(fr, wr, br))
    yr.backward(Gd)
    fused = L.interp_gn_nparts(size[0] * size[1] * size[2] // 4, C // G) > 0
    assert fused == (size != (6, 10, 12)) and (len(calls) == 0) == fused
    close(y, yr.detach(), 2e-5)
    close(x.grad, xr.grad, 1e-4); close(f.grad, fr.grad, 1e-4)
    close(conv.weight.grad, wr.grad, 1e-4); close(conv.bias.grad, br.grad, 2e-4)
    close(gn.weight.grad, ref_gn.weight.grad, 1e-4); close(gn.bias.grad, ref_gn.bias.grad, 1e-4)



def test_plane_sums_are_dropped_when_the_gradient_is_touched_in_place(backend):
    """the plane sums that _UpGN*.backward attach to the gradient of the lateral are bound to its version counter, storage and (B, C, S): a hook that
    rescales that gradient IN PLACE must make the lateral's bias gradient come from the row-sum kernel again (the stale closed-form sums were used before)."""
    B, C, G, Cf, insize, size = 2, 8, 4, 6, (4, 8, 8), (8, 16, 16)
    gn = torch.nn.GroupNorm(G, C)
    conv = torch.nn.Conv3d(Cf, C, 1)
    with torch.no_grad():
        conv.weight.copy_(0.4 * rnd(C, Cf, 1, 1, 1, seed=43)); conv.bias.copy_(0.3 * rnd(C, seed=44))
    x = (rnd(B, C, *insize, seed=45) + 0.5).requires_grad_(True)
    f = rnd(B, Cf, *size, seed=46).requires_grad_(True)
    grads = {}
    for scale in (None, 3.0):
        for t in (x, f, conv.weight, conv.bias):
            t.grad = None
        base = SF.conv1x1(f, conv.weight, conv.bias)
        if scale is not None:
            base.register_hook(lambda g: (g.mul_(scale), None)[1])          # in place, returns None: autograd hands the SAME (modified) tensor on
        y = SF.up_group_norm(x, size, base, gn)
        y.backward(rnd(*y.shape, seed=47))
        grads[scale] = (conv.bias.grad.clone(), conv.weight.grad.clone())
    close(grads[3.0][1], 3.0 * grads[None][1], 1e-5)
    close(grads[3.0][0], 3.0 * grads[None][0], 1e-5)


@pytest.mark.parametrize('B,C,G,Cout,insize,size,with_bias', [(2, 8, 4, 12, (4, 8, 8), (8, 16, 16), True), (2, 8, 4, 6, (4, 8, 8), (8, 16, 16), True), (1, 16, 8, 3, (2, 8, 16), (4, 16, 32), False), (1, 16, 8, 9, (2, 8, 16), (4, 16, 32), False),
                                                           (2, 8, 2, 5, (8, 8, 8), (8, 16, 16), True), (1, 8, 4, 4, (3, 5, 6), (6, 10, 12), True)])
def test_group_norm_folded_into_its_pointwise_consumer(backend, B, C, G, Cout, insize, size, with_bias):
    """SF.up_group_norm_conv (r05): conv1x1(gn(up(x) + lateral(f))) with the GroupNorm folded into per-sample weights / biases -- the normalised level is never
    written, the backward needs one pass over it (segx_gn_fold_bwd) and takes the gradients of scale / shift from the consumer's per-sample weight and bias
    gradients.  Against PyTorch: the output and EVERY gradient (x, f, lateral weight + bias, GroupNorm affine, consumer weight + bias); Cout <= 8 takes the one-node form whose backward builds the consumer's
    data gradient on the fly (_UpGNFoldProj), Cout > 8 the (level, scale, shift) node + a per-sample GEMM; the last case does not split into 1024-float chunks
    and takes the unfolded ops."""
    Cf = 5
    gn, ref_gn = torch.nn.GroupNorm(G, C), torch.nn.GroupNorm(G, C)
    lat, cons = torch.nn.Conv3d(Cf, C, 1), torch.nn.Conv3d(C, Cout, 1, bias=with_bias)
    with torch.no_grad():
        for m in (gn, ref_gn):
            m.weight.copy_(1 + 0.3 * rnd(C, seed=71)); m.bias.copy_(0.3 * rnd(C, seed=72))
        lat.weight.copy_(0.4 * rnd(C, Cf, 1, 1, 1, seed=73)); lat.bias.copy_(0.3 * rnd(C, seed=74))
        cons.weight.copy_(0.5 * rnd(Cout, C, 1, 1, 1, seed=75))
        if with_bias:
            cons.bias.copy_(0.2 * rnd(Cout, seed=76))
    x = (rnd(B, C, *insize, seed=77) + 0.4).requires_grad_(True)
    f = rnd(B, Cf, *size, seed=78).requires_grad_(True)
    y = SF.up_group_norm_conv(x, size, SF.conv1x1(f, lat.weight, lat.bias), gn, cons.weight, cons.bias)
    Gd = rnd(*y.shape, seed=79)
    y.backward(Gd)
    xr, fr = x.detach().clone().requires_grad_(True), f.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in dict(lw=lat.weight, lb=lat.bias, cw=cons.weight, **({'cb': cons.bias} if with_bias else {})).items()}
    yr = F.conv3d(ref_gn(F.interpolate(xr, size=size, mode='trilinear', align_corners=False) + F.conv3d(fr, P['lw'], P['lb'])), P['cw'], P.get('cb'))
    yr.backward(Gd)
    close(y, yr.detach(), 3e-5)
    close(x.grad, xr.grad, 2e-4); close(f.grad, fr.grad, 2e-4)
    close(lat.weight.grad, P['lw'].grad, 2e-4); close(lat.bias.grad, P['lb'].grad, 3e-4)
    close(cons.weight.grad, P['cw'].grad, 2e-4)
    if with_bias:
        close(cons.bias.grad, P['cb'].grad, 2e-4)
    close(gn.weight.grad, ref_gn.weight.grad, 2e-4); close(gn.bias.grad, ref_gn.bias.grad, 2e-4)
    # the A/B switch gives the same function through the unfolded ops
    prev = SF.fold_group_norm
    SF.fold_group_norm = False
    try:
        y2 = SF.up_group_norm_conv(x.detach(), size, SF.conv1x1(f.detach(), lat.weight, lat.bias), gn, cons.weight, cons.bias)
    finally:
        SF.fold_group_norm = prev
    close(y2.detach(), y.detach(), 3e-5)



@pytest.mark.parametrize('B,C,G,Cout,insize,size', [(2, 8, 4, 3, (16, 16), (32, 32)), (2, 8, 4, 10, (16, 16), (32, 32)), (1, 16, 8, 5, (8, 32), (32, 64)), (2, 8, 2, 4, (5, 6), (10, 12))])
def test_group_norm_folded_into_its_pointwise_consumer_2d(backend, B, C, G, Cout, insize, size):
    """the same fold on 2-D maps (Segtran2d.out_head_forward: bilinear up-sampling = the x pass + a y pass that leaves the statistics); last case: unfolded ops"""
    Cf = 5
    gn, ref_gn = torch.nn.GroupNorm(G, C), torch.nn.GroupNorm(G, C)
    lat, cons = torch.nn.Conv2d(Cf, C, 1), torch.nn.Conv2d(C, Cout, 1)
    with torch.no_grad():
        for m in (gn, ref_gn):
            m.weight.copy_(1 + 0.3 * rnd(C, seed=81)); m.bias.copy_(0.3 * rnd(C, seed=82))
        lat.weight.copy_(0.4 * rnd(C, Cf, 1, 1, seed=83)); lat.bias.copy_(0.3 * rnd(C, seed=84))
        cons.weight.copy_(0.5 * rnd(Cout, C, 1, 1, seed=85)); cons.bias.copy_(0.2 * rnd(Cout, seed=86))
    x = (rnd(B, C, *insize, seed=87) + 0.4).requires_grad_(True)
    f = rnd(B, Cf, *size, seed=88).requires_grad_(True)
    y = SF.up_group_norm_conv(x, size, SF.conv1x1(f, lat.weight, lat.bias), gn, cons.weight, cons.bias)
    Gd = rnd(*y.shape, seed=89)
    y.backward(Gd)
    xr, fr = x.detach().clone().requires_grad_(True), f.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in dict(lw=lat.weight, lb=lat.bias, cw=cons.weight, cb=cons.bias).items()}
    yr = F.conv2d(ref_gn(F.interpolate(xr, size=size, mode='bilinear', align_corners=False) + F.conv2d(fr, P['lw'], P['lb'])), P['cw'], P['cb'])
    yr.backward(Gd)
    close(y, yr.detach(), 3e-5)
    close(x.grad, xr.grad, 2e-4); close(f.grad, fr.grad, 2e-4)
    close(lat.weight.grad, P['lw'].grad, 2e-4); close(lat.bias.grad, P['lb'].grad, 3e-4)
    close(cons.weight.grad, P['cw'].grad, 2e-4); close(cons.bias.grad, P['cb'].grad, 2e-4)
    close(gn.weight.grad, ref_gn.weight.grad, 2e-4); close(gn.bias.grad, ref_gn.bias.grad, 2e-4)


def test_group_norm_partials_of_a_badly_centred_tensor(backend):
    """The partials are sums around a per-workgroup pivot merged with Chan's formula: a level whose mean is 1000 standard deviations away from zero must
    still normalise to unit variance (a plain sum / sum-of-squares form loses every digit of the variance there)."""
    B, C, G = 1, 8, 2
    gn = torch.nn.GroupNorm(G, C)
    x = rnd(B, C, 4, 8, 8, seed=50) * 1e-2
    base = rnd(B, C, 8, 16, 16, seed=51) * 1e-2 + 10.0
    y = SF.up_group_norm(x, (8, 16, 16), base, gn)
    yr = torch.nn.functional.group_norm(F.interpolate(x.double(), size=(8, 16, 16), mode='trilinear', align_corners=False) + base.double(), G, gn.weight.double(), gn.bias.double(), gn.eps)
    assert float((y.double() - yr).abs().max()) < 2e-3            # fp32 input rounding at |x| = 10 with std 1e-2 bounds what ANY fp32 kernel can do: ~1e-6 / 1e-2 relative
    v = y.reshape(B, G, -1).var(dim=2, unbiased=False)          # var / (var + eps) with var ~ 1.3e-4 (the blend of the up-sampled part included) and eps = 1e-5
    assert 0.85 < float(v.min()) and float(v.max()) < 1.0


@pytest.mark.parametrize('inshape,size', [((2, 3, 4, 5), (8, 10)), ((1, 2, 7, 7), (14, 14)), ((2, 2, 8, 6), (16, 24)), ((1, 3, 16, 16), (13, 9)),
                                          ((1, 2, 3, 4, 5), (6, 8, 10)), ((2, 2, 6, 7, 7), (12, 14, 14)), ((1, 2, 4, 3, 3), (4, 12, 12)),
                                          ((1, 2, 8, 5, 5), (4, 5, 5)), ((1, 1, 12, 14, 14), (48, 56, 56)),
                                          # r04, y and z in one pass (W % 4 == 0, both resized): ragged sizes, a non-integer ratio, x not resized; an axis that is not
                                          # resized / W % 4 != 0 keep the one-axis passes
                                          ((2, 2, 9, 17, 20), (18, 34, 40)), ((1, 3, 5, 9, 12), (8, 16, 20)), ((1, 2, 6, 10, 36), (6, 20, 72)),
                                          ((1, 1, 3, 4, 6), (6, 8, 10))])
@pytest.mark.parametrize('with_base', [False, True])
def test_interp_linear(backend, inshape, size, with_base):
    mode = 'bilinear' if len(size) == 2 else 'trilinear'
    x = rnd(*inshape, seed=5).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    base = rnd(*(inshape[:2] + tuple(size)), seed=6).requires_grad_(True) if with_base else None
    br = base.detach().clone().requires_grad_(True) if with_base else None
    y = SF.interp_linear(x, size, base)
    yr = F.interpolate(xr, size=size, mode=mode, align_corners=False)
    if with_base:
        yr = yr + br
    close(y, yr.detach(), 1e-5)
    G = rnd(*y.shape, seed=7)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-5)
    if with_base:
        close(base.grad, br.grad, 1e-6)



@pytest.mark.parametrize('w,W,align', [(16, 64, False), (5, 20, False), (7, 12, False), (40, 16, False), (9, 36, True), (3, 8, False), (1, 4, False)])
@pytest.mark.parametrize('with_base', [False, True])
def test_contiguous_axis_pass_with_float4_access(backend, w, W, align, with_base):
    """r05: segx_interp_linear_{fwd,bwd}_axis with inner == 1 and n_out % 4 == 0 (the x pass of the pyramid's up-sampling) -- four outputs per thread forward,
    aligned float4 candidate reads backward -- against F.interpolate along the last axis: x4 and non-integer ratios, a down-sampling, align_corners, base add."""
    L = backend.L
    rows = 37
    x = rnd(rows, w, seed=60)
    base = rnd(rows, W, seed=61) if with_base else None
    scale = 0.0 if not align else -((w - 1) / (W - 1))
    out = torch.empty(rows, W)
    L.interp_fwd_axis(x, base, out, rows, w, W, 1, scale)
    ref = F.interpolate(x.double().view(1, rows, w), size=W, mode='linear', align_corners=align).view(rows, W)
    if with_base:
        ref = ref + base.double()
    assert float((out.double() - ref).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max()))
    G = rnd(rows, W, seed=62)
    dx = torch.empty(rows, w)
    L.interp_bwd_axis(G, dx, rows, W, w, 1, scale)
    xr = x.double().clone().requires_grad_(True)
    F.interpolate(xr.view(1, rows, w), size=W, mode='linear', align_corners=align).backward(G.double().view(1, rows, W))
    assert float((dx.double() - xr.grad).abs().max()) < 2e-6 * max(1.0, float(xr.grad.abs().max()))



@pytest.mark.parametrize('d,h,D,H', [(4, 6, 8, 12), (3, 5, 12, 20), (5, 4, 7, 9), (6, 8, 3, 4), (2, 3, 18, 27)])
def test_fixed_contributor_adjoints_equal_the_candidate_loops_bit_for_bit(backend, d, h, D, H):
    """r05: interp_bwd_axis2_fixed / interp_bwd_axis4_fixed collect a cell's contributing outputs first and then load them back to back; the loops they replace
    (segx_tune knob 1 = 1 keeps them) walk a conservative candidate range with a branch per load.  Same contributors, same order, same weight expression: identical bits on the emulator, to an ulp of a weight on the device -- at ratios 2 and 4 (the pyramid), a non-integer ratio, a down-sampling, and ratio 9 (more than 8 contributors: the loop form serves both)."""
    L = backend.L
    planes, W = 3, 8
    G = rnd(planes, D, H, W, seed=95)
    outs = {}
    for variant in (0, 1):
        with L.tuned(interp_variant=variant):
            g2 = torch.empty(planes * d * h * W); L.interp_bwd_axis2(G, g2, planes, D, d, H, h, W)
            g1 = torch.empty(planes * d * H * W); L.interp_bwd_axis(G, g1, planes, D, d, H * W, 0.0)
            gx = torch.empty(planes * D * H * (W // 4)) if W % 4 == 0 else None          # the contiguous axis (x4 / column-per-thread forms vs the per-cell form)
            if gx is not None:
                L.interp_bwd_axis(G, gx, planes * D * H, W, W // 4, 1, 0.0)
            gy = torch.empty(planes * D * H * (W // 2)); L.interp_bwd_axis(G, gy, planes * D * H, W, W // 2, 1, 0.0)
            outs[variant] = (g2, g1, gx, gy)
    for a, b in zip(outs[0], outs[1]):
        if a is None:
            continue
        if a.is_cuda:
            close(a, b, 1e-6)                                  # hipcc contracts the weight expression per kernel (fma or mul + add): an ulp in a weight, session r05_g
        else:
            assert torch.equal(a, b)


def test_two_axis_resampling_pass_equals_the_one_axis_passes(backend):
    """segx_interp_linear_{fwd,bwd}_axis2 (y and z of a trilinear resampling in one pass) against the two one-axis passes they replace: the same
    blends in the same order (the compiler may contract the multiply-adds differently: a few ulp)."""
    L = backend.L
    B, C, d, h, w, D, H, W = 2, 3, 9, 17, 20, 18, 34, 40
    t1, base, G = rnd(B * C * d * h * W, seed=90), rnd(B, C, D, H, W, seed=91), rnd(B, C, D, H, W, seed=92)
    out = torch.empty(B, C, D, H, W)
    L.interp_fwd_axis2(t1, base, out, B * C, d, D, h, H, W)
    t2 = torch.empty(B * C * d * H * W); L.interp_fwd_axis(t1, None, t2, B * C * d, h, H, W, 0.0)
    ref = torch.empty(B, C, D, H, W); L.interp_fwd_axis(t2, base, ref, B * C, d, D, H * W, 0.0)
    close(out, ref, 1e-6)
    g12 = torch.empty(B * C * d * h * W)
    L.interp_bwd_axis2(G, g12, B * C, D, d, H, h, W)
    g1 = torch.empty(B * C * d * H * W); L.interp_bwd_axis(G, g1, B * C, D, d, H * W, 0.0)
    g2 = torch.empty(B * C * d * h * W); L.interp_bwd_axis(g1, g2, B * C * d, H, h, W, 0.0)
    close(g12, g2, 1e-6)


@pytest.mark.parametrize('shape,C,kw', [((7, 10), 6, dict(scale_factor=1. / 3)), ((7, 10), 8, dict(scale_factor=0.5)), ((8, 12), 5, dict(scale_factor=0.25)),
                                        ((5, 6, 7), 4, dict(scale_factor=0.5)), ((2, 3), 8, dict(out_shape=(7, 10))), ((2, 3, 3), 3, dict(out_shape=(5, 6, 7))),
                                        ((4, 4), 4, dict(scale_factor=1.0))])
def test_interp_tokens_channels_last(backend, shape, C, kw):
    """resize_flat_features on channels-last tokens: the scale_factor form keeps the GIVEN factor for the source coordinates
    (7 -> 2 at factor 1/3 steps by 3.0, not 3.5), the size form uses n_in/n_out; both == F.interpolate on the NC[D]HW view."""
    B, N = 2, int(torch.tensor(shape).prod())
    x = rnd(B, N, C, seed=31).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    y = SF.interp_tokens(x, shape, **kw)
    mode = 'bilinear' if len(shape) == 2 else 'trilinear'
    g = xr.permute(0, 2, 1).reshape(B, C, *shape)
    yr = F.interpolate(g, size=kw.get('out_shape'), scale_factor=kw.get('scale_factor'), mode=mode, align_corners=False)
    yr = yr.reshape(B, C, -1).permute(0, 2, 1)
    assert y.shape == yr.shape
    close(y, yr.detach(), 1e-6)
    G = rnd(*y.shape, seed=32)
    y.backward(G); yr.backward(G)
    close(x.grad, xr.grad, 1e-5)


@pytest.mark.parametrize('n', [4096 * 3, 1003])
def test_standalone_dropout(backend, n):
    """segx_dropout (--outdrop): keep fraction ~ 1-p, survivors scaled by 1/(1-p), backward re-uses the forward mask, the
    Philox stream advances between calls, and eval / p = 0 is the identity."""
    x = (rnd(n, seed=41).abs() + 0.5).requires_grad_(True)
    SF.manual_seed(9)
    y = SF.dropout(x, 0.25)
    keep = y != 0
    assert abs(keep.float().mean().item() - 0.75) < (0.02 if n > 4096 else 0.06)
    close(y[keep], (x.detach() / 0.75)[keep], 1e-6)
    G = rnd(n, seed=42)
    y.backward(G)
    assert torch.equal(x.grad != 0, keep & (G != 0))
    close(x.grad[keep], (G / 0.75)[keep], 1e-6)
    y2 = SF.dropout(x.detach(), 0.25)
    assert not torch.equal(y2 != 0, keep)
    assert SF.dropout(x, 0.25, training=False) is x and SF.dropout(x, 0.0) is x


@pytest.mark.parametrize('grid', [(6, 5), (3, 4, 5)])
def test_composed_output_head_equals_reference_op_order(backend, grid):
    """out_conv(bridge(cur) + up(y)) == conv(cur; W_out W_bridge, W_out b_bridge + b_out) + up(conv_tokens(y; W_out)): values and
    the gradients of every factor (W_out, b_out, W_bridge, b_bridge, cur, y), against the reference op order in plain PyTorch."""
    nd = len(grid)
    B, d3, Fd, nc = 2, 12, 20, 3
    big = tuple(2 * g for g in grid)
    N = int(torch.tensor(grid).prod())
    ones = (1,) * nd
    cur = rnd(B, d3, *big, seed=51).requires_grad_(True)
    tok = rnd(B, N, Fd, seed=52).requires_grad_(True)
    Wb = (rnd(Fd, d3, *ones, seed=53) * 0.3).requires_grad_(True); bb = rnd(Fd, seed=54).requires_grad_(True)
    Wo = (rnd(nc, Fd, *ones, seed=55) * 0.3).requires_grad_(True); bo = rnd(nc, seed=56).requires_grad_(True)
    lateral = SF.conv1x1(cur, *SF.compose_conv1x1(Wo, bo, Wb, bb))
    y = SF.interp_linear(SF.conv1x1_tokens(tok, grid, Wo), big, lateral)
    ref_in = [t.detach().clone().requires_grad_(True) for t in (cur, tok, Wb, bb, Wo, bo)]
    c_, t_, Wb_, bb_, Wo_, bo_ = ref_in
    conv = F.conv2d if nd == 2 else F.conv3d
    ymap = t_.view(B, *grid, Fd).permute(0, nd + 1, *range(1, nd + 1))
    yr = conv(conv(c_, Wb_, bb_) + F.interpolate(ymap, size=big, mode='bilinear' if nd == 2 else 'trilinear', align_corners=False), Wo_, bo_)
    close(y, yr.detach(), 1e-5)
    G = rnd(*y.shape, seed=57)
    y.backward(G); yr.backward(G)
    for a, b in zip((cur, tok, Wb, bb, Wo, bo), ref_in):
        close(a.grad, b.grad, 1e-4)


@pytest.mark.parametrize('shape', [(3, 4, 6, 10), (6, 2, 32, 32), (2, 3, 130, 132)])       # channel-resident wave form, workgroup form, two-launch form
def test_bn_backward_reads_a_concatenation_gradient_in_place(backend, shape):
    """torch.cat's backward hands every operand a narrow() view of the concatenation's gradient; the BatchNorm backward kernels read such a channel
    slice in place (batch stride = the wide tensor's) instead of through a contiguous copy -- the four branches of an Inception module."""
    B, C = shape[:2]
    bns = [torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01) for _ in range(2)]
    refs = [torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01) for _ in range(2)]
    with torch.no_grad():
        for i, (m, r) in enumerate(zip(bns, refs)):
            m.weight.copy_(1 + 0.2 * rnd(C, seed=60 + i)); m.bias.copy_(0.2 * rnd(C, seed=62 + i)); r.load_state_dict(m.state_dict())
    xs = [(rnd(*shape, seed=64 + i) * 1.3 + 0.2).requires_grad_(True) for i in range(2)]
    xr = [x.detach().clone().requires_grad_(True) for x in xs]
    out = torch.cat([SF.bn_act(x, m, SF.ACT_RELU) for x, m in zip(xs, bns)], dim=1)
    outr = torch.cat([F.relu(r(x)) for x, r in zip(xr, refs)], dim=1)
    close(out, outr.detach())
    G = rnd(B, 2 * C, *shape[2:], seed=66)
    out.backward(G); outr.backward(G)
    for x, r, m, rm in zip(xs, xr, bns, refs):
        close(x.grad, r.grad, 1e-4); close(m.weight.grad, rm.weight.grad, 1e-4); close(m.bias.grad, rm.bias.grad, 1e-4)


@pytest.mark.parametrize('path,shape', [(0, (3, 4, 6, 10)), (0, (6, 2, 32, 32)), (1, (2, 3, 130, 132)), (2, (2, 3, 130, 132)), (2, (2, 4, 3, 4, 4)), (0, (2, 4, 3, 4, 5)),
                                        (0, (2, 3, 5, 7))])
@pytest.mark.parametrize('training', [True, False])
def test_bn_branches_write_their_slices_of_the_concatenation(backend, path, shape, training):
    """r05: SF.bn_act_cat = torch.cat([head, relu(bn_1(x_1)), relu(bn_2(x_2)), relu(bn_3(x_3))], 1) with every BatchNorm kernel form (wave- / workgroup-resident, team:
    knob 3 = 2, two launches: knob 3 = 1, eval) writing its channels into the concatenation (segx_bn_act_fwd2 y_bs); planes that are not float4 multiples (5 x 7) keep
    the copy.  Bit-equal to the separate ops in forward, running statistics and every gradient (the backward IS the separate ops'); the head may be a strided slice."""
    L = backend.L
    B, C = shape[:2]
    Cs = (C, C + 4, 2 * C)
    bn_cls = torch.nn.BatchNorm3d if len(shape) == 5 else torch.nn.BatchNorm2d
    def layers():
        ms = [bn_cls(c, eps=1e-3, momentum=0.01) for c in Cs]
        with torch.no_grad():
            for i, m in enumerate(ms):
                m.weight.copy_(1 + 0.2 * rnd(m.num_features, seed=160 + i)); m.bias.copy_(0.2 * rnd(m.num_features, seed=163 + i))
                m.running_mean.copy_(0.1 * rnd(m.num_features, seed=166 + i)); m.running_var.copy_(1 + 0.1 * rnd(m.num_features, seed=169 + i).abs())
            for m in ms:
                m.train(training)
        return ms
    wide = rnd(B, 8, *shape[2:], seed=172)
    def inputs():
        return [(rnd(B, c, *shape[2:], seed=173 + i) * 1.3 + 0.2).requires_grad_(True) for i, c in enumerate(Cs)], wide.detach().clone().requires_grad_(True)
    with L.tuned(bn_path=path):
        bns, (xs, wd) = layers(), inputs()
        out = SF.bn_act_cat(wd[:, 3:8], list(zip(xs, bns)), SF.ACT_RELU)
        refs, (xr, wr) = layers(), inputs()
        outr = torch.cat([wr[:, 3:8]] + [SF.bn_act(x, m, SF.ACT_RELU) for x, m in zip(xr, refs)], dim=1)
        assert out.shape == outr.shape and out.is_contiguous()
        assert torch.equal(out, outr)
        for m, r in zip(bns, refs):
            assert torch.equal(m.running_mean, r.running_mean) and torch.equal(m.running_var, r.running_var) and m.num_batches_tracked == r.num_batches_tracked
        G = rnd(*out.shape, seed=180)
        out.backward(G); outr.backward(G)
        assert torch.equal(wd.grad, wr.grad) and wd.grad[:, :3].abs().sum() == 0
        for x, r, m, rm in zip(xs, xr, bns, refs):
            assert torch.equal(x.grad, r.grad) and torch.equal(m.weight.grad, rm.weight.grad) and torch.equal(m.bias.grad, rm.bias.grad)
        # and against PyTorch itself
        tb = layers()
        xt = [x.detach().clone().requires_grad_(True) for x in xs]
        outt = torch.cat([wide[:, 3:8]] + [F.relu(m(x)) for x, m in zip(xt, tb)], dim=1)
        close(out, outt.detach())
        outt.backward(G)
        for x, t in zip(xs, xt):
            close(x.grad, t.grad, 1e-4)


def test_bn_forward_refuses_an_output_slice_it_cannot_write_in_quads(backend):
    L = backend.L
    B, C, S = 2, 3, 35
    x = rnd(B, C, S, seed=181)
    wide = torch.zeros(B, 8, S)
    w, b = torch.ones(C), torch.zeros(C)
    mean, var = torch.empty(C), torch.empty(C)
    parts = torch.empty(L.bn_parts_floats(B, C, S))
    with pytest.raises(Exception, match='output slice'):
        L.c.segx_bn_act_fwd2(x.data_ptr(), parts.data_ptr(), 0, mean.data_ptr(), var.data_ptr(), None, None, 0.0, w.data_ptr(), b.data_ptr(), wide[:, 4:7].data_ptr(), None, None,
                             0.0, 0, 0, B, C, S, 1e-3, 0, parts.numel(), 8 * S, L.stream(x)) and L.check(-1, 'segx_bn_act_fwd2')
