"""Eval-mode throughput with and without BatchNorm folded into the backbone's kernels (Segtran2d.fold_batchnorm).

  python tools/infer_bench.py [--reps 20] [--warmup 5] [--cfgs cfg1,cfg2,cfg3] [--no-window]

One process: for every configuration (its BASELINE batch) the SAME model runs the eval forward unfolded and folded in alternation -- warm-up, then `reps` pairs, each
forward timed with HIP events on the launch stream; the medians and their ratio are reported.  Then test_single_batch (sliding-window inference) on a 576 x 576 image
with the cfg1 model, the same way.  Output: ONE JSON line.  The unfolded forward is the path every earlier commit ran, so the ratio needs no second box.

  --once cfgN:folded|unfolded   run ONE warm eval forward of one variant and exit (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py --once cfg2:folded)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, test_util2d as T2              # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(net, run, reps, warmup):
    """-> (median ms unfolded, median ms folded): the two variants take turns, so drift of the box hits both alike"""
    ms = {False: [], True: []}
    for i in range(warmup + reps):
        for folded in (False, True):
            if folded:
                net.fold_batchnorm()
            else:
                net.unfold_batchnorm()
            t = timed(run)
            if i >= warmup:
                ms[folded].append(t)
    net.unfold_batchnorm()
    return statistics.median(ms[False]), statistics.median(ms[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cfgs', default='cfg1,cfg2,cfg3')
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--once', default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.once, 'the median is taken over at least 20 repetitions'
    dev = torch.device('cuda', 0)
    if a.once:
        name, variant = a.once.split(':')
        net = engine.build_model(name, dev, dropout_prob=0.0).eval()
        if variant == 'folded':
            net.fold_batchnorm()
        x, _ = engine.synth_batch(name, engine.CONFIGS[name]['bs'], dev)
        with torch.no_grad():
            for _ in range(3):
                net(x)
        torch.cuda.synchronize()
        return
    out = {'tool': 'infer_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'configs': {}}
    for name in a.cfgs.split(','):
        c = engine.CONFIGS[name]
        net = engine.build_model(name, dev, dropout_prob=0.0).eval()
        x, _ = engine.synth_batch(name, c['bs'], dev)

        def run():
            with torch.no_grad():
                net(x)
        unf, fold = alternate(net, run, a.reps, a.warmup)
        out['configs'][name] = {'batch': c['bs'], 'size': list(c['size']), 'unfolded_ms': round(unf, 4), 'folded_ms': round(fold, 4),
                                'folded_over_unfolded': round(fold / unf, 4), 'unfolded_images_per_s': round(c['bs'] * 1e3 / unf, 2),
                                'folded_images_per_s': round(c['bs'] * 1e3 / fold, 2)}
        del net
        torch.cuda.empty_cache()
    if not a.no_window:
        c = engine.CONFIGS['cfg1']
        net = engine.build_model('cfg1', dev, dropout_prob=0.0).eval()
        img, _ = engine.synth_batch(dict(c, size=(576, 576)), 1, dev)
        S = c['size'][0]

        def run_w():
            T2.test_single_batch(net, img, (S, S), (S, S), (S // 2, S // 2), c['task'], c['num_classes'])
        unf, fold = alternate(net, run_w, a.reps, a.warmup)
        out['test_single_batch_576'] = {'model': 'cfg1', 'window': [S, S], 'stride': [S // 2, S // 2], 'unfolded_ms': round(unf, 4), 'folded_ms': round(fold, 4),
                                        'folded_over_unfolded': round(fold / unf, 4), 'folded_images_per_s': round(1e3 / fold, 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
