"""Surface-distance metrics on the device (metrics.hip): time of infer3d.calculate_metric_percase(surface=True, hd95=True) on synthetic blobs.

  python tools/surface_bench.py [--reps 20] [--warmup 5] [--shape 240,240,155] [--out profiles/surface_metrics_bench.json]

One process.  Class maps [4, *shape] (three foreground classes of a few balls each, prediction = ground truth with every ball moved and resized a little).  Timed with
HIP events on the launch stream, medians over `reps` calls after `warmup`:
  percase_surface_hd95   the whole call: Dice sums, 2 x border, 2 x transform, 2 x histogram, the one device-to-host copy and the float64 finish on the host
  percase_surface        the same without hd95 (one transform, one histogram)
  percase_default        Dice / Jaccard only (what the call cost before)
  border / edt_sq / hist one kernel family each, on the three foreground planes (edt_sq = the W, H and D passes)
When scipy is importable, `host_scipy_ms` is the host restatement (binary_erosion + distance_transform_edt per class and direction, as medpy does it) on the same
masks, wall clock, one run.  Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from segtran_amd import functional as SF                       # noqa: E402
from segtran_amd import infer3d                                # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def blobs(shape, dev, seed, jitter):
    """[4, *shape] n-hot 0/1 floats: three classes of four balls; jitter moves / resizes every ball (the same seed gives the same balls)"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    ax = [torch.arange(s, device=dev, dtype=torch.float32).view([-1 if i == a else 1 for i in range(3)]) for a, s in enumerate(shape)]
    out = torch.zeros((4,) + tuple(shape), device=dev)
    for c in range(1, 4):
        for _ in range(4):
            ctr = [float(torch.rand(1, generator=g)) * s for s in shape]
            r = (0.08 + 0.12 * float(torch.rand(1, generator=g))) * min(shape)
            ctr, r = [v + jitter for v in ctr], r * (1.0 + 0.02 * jitter)
            out[c] = torch.maximum(out[c], (sum((a - v) ** 2 for a, v in zip(ax, ctr)) <= r * r).float())
    out[0] = 1.0 - out[1:].amax(0)
    return out


def host_scipy(pred, gt):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 1)
    t0 = time.perf_counter()
    for c in range(pred.shape[0]):
        p, g = pred[c] != 0, gt[c] != 0
        if not (p.any() and g.any()):
            continue
        bp, bg = p ^ ndimage.binary_erosion(p, st), g ^ ndimage.binary_erosion(g, st)
        dg, dp = ndimage.distance_transform_edt(~bg), ndimage.distance_transform_edt(~bp)
        dg[bp].mean(); np.percentile(np.hstack((dg[bp], dp[bg])), 95)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shape', default='240,240,155')
    ap.add_argument('--out', default=os.path.join('profiles', 'surface_metrics_bench.json'))
    a = ap.parse_args()
    assert a.reps >= 20, 'the median is taken over at least 20 repetitions'
    shape = tuple(int(v) for v in a.shape.split(','))
    dev = torch.device('cuda', 0)
    gt, pred = blobs(shape, dev, 7, 0.0), blobs(shape, dev, 7, 2.5)
    fg = pred[1:].contiguous()
    border = SF.surface_border(fg)
    d2 = SF.edt_sq(border)
    forms = {'percase_surface_hd95': lambda: infer3d.calculate_metric_percase(pred, gt, 4, surface=True, hd95=True),
             'percase_surface': lambda: infer3d.calculate_metric_percase(pred, gt, 4, surface=True),
             'percase_default': lambda: infer3d.calculate_metric_percase(pred, gt, 4),
             'border': lambda: SF.surface_border(fg), 'edt_sq': lambda: SF.edt_sq(border), 'hist': lambda: SF.surface_hist(border, d2)}
    ms = {k: [] for k in forms}
    for i in range(a.warmup + a.reps):
        for k, fn in forms.items():
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
    metric, valid = forms['percase_surface_hd95']()
    out = {'tool': 'surface_bench', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'classes': 3, 'reps': a.reps, 'warmup': a.warmup,
           'median_ms': {k: round(statistics.median(v), 4) for k, v in ms.items()}, 'min_ms': {k: round(min(v), 4) for k, v in ms.items()},
           'metric': [[round(float(x), 6) for x in row] for row in metric], 'valid': valid.tolist()}
    try:
        import scipy                                            # noqa: F401
        out['host_scipy_ms'] = round(host_scipy(pred[1:].cpu().numpy(), gt[1:].cpu().numpy()), 1)
    except ImportError:
        out['host_scipy_ms'] = None
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
