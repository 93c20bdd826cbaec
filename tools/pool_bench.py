"""Stride-1 3 x 3 x 3 'same' max-pools of the I3D Inception modules: the slab-in-LDS form (segx_tune knob 14) against the four-cells-per-thread / tile-gather
forms, forward and backward, on the planes of cfg4 (112 x 112 x 96) and cfg5 (128^3) at batch 4.  GPU box:  python tools/pool_bench.py"""
import os, sys, statistics, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from segtran_amd import segx

dev = torch.device('cuda', 0)
L = segx.lib()
# (name, channels, (D, H, W)) of the pooled tensor (the Inception module's input), batch 4
CASES = [('cfg4 Mixed_3b', 192, (48, 28, 28)), ('cfg4 Mixed_3c', 256, (48, 28, 28)), ('cfg4 Mixed_4b', 480, (24, 14, 14)), ('cfg4 Mixed_4f', 528, (24, 14, 14)),
         ('cfg4 Mixed_5b', 832, (12, 7, 7)), ('cfg5 Mixed_3b', 192, (64, 32, 32)), ('cfg5 Mixed_3c', 256, (64, 32, 32)), ('cfg5 Mixed_4b', 480, (32, 16, 16)),
         ('cfg5 Mixed_4f', 528, (32, 16, 16)), ('cfg5 Mixed_5b', 832, (16, 8, 8))]


def timed(fn, reps=10, rounds=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ts)


g = torch.Generator(device='cpu').manual_seed(0)
for name, C, (D, H, W) in CASES:
    B = 4
    x = torch.relu(torch.randn(B, C, D, H, W, generator=g)).to(dev)
    dy = torch.randn(B, C, D, H, W, generator=g).to(dev)
    geom = (D, H, W, D, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1)
    nbytes = 3 * x.numel() * 4
    res, ref = {}, None
    for policy in (2, 0, 1):
        assert L.c.segx_tune(segx.Knob.POOL_SLAB, policy) == 0
        y, arg, dx = torch.empty_like(x), torch.empty(x.shape, dtype=torch.int32, device=dev), torch.empty_like(x)
        tf = timed(lambda: L.maxpool3d_fwd(x, y, arg, B * C, geom))
        tb = timed(lambda: L.maxpool3d_bwd(dy, arg, dx, B * C, geom))
        if ref is None:
            ref = (y.clone(), arg.clone(), dx.clone())
        same = torch.equal(y, ref[0]) and torch.equal(arg, ref[1]) and torch.equal(dx, ref[2])
        res[policy] = (tf, tb, same)
    L.c.segx_tune(segx.Knob.POOL_SLAB, 0)
    print('%-14s C=%4d %2dx%2dx%2d  %6.1f MB/pass | ' % (name, C, D, H, W, nbytes / 3e6) +
          ' | '.join('policy %d: fwd %6.1f us %4.2f TB/s, bwd %6.1f us %4.2f TB/s%s' % (p, r[0] * 1e3, nbytes / r[0] / 1e9, r[1] * 1e3, nbytes / r[1] / 1e9, '' if r[2] else ' MISMATCH')
                     for p, r in res.items()), flush=True)
