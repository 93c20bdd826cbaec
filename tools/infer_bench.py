"""Eval-mode throughput with and without BatchNorm folded into the backbone's kernels (Segtran2d.fold_batchnorm).

  python tools/infer_bench.py [--reps 20] [--warmup 5] [--cfgs cfg1,cfg2,cfg3] [--no-window]

One process: for every configuration (its BASELINE batch) the SAME model runs the eval forward unfolded and folded in alternation -- warm-up, then `reps` pairs, each
forward timed with HIP events on the launch stream; the medians and their ratio are reported.  Then test_single_batch (sliding-window inference) on a 576 x 576 image
with the cfg1 model, the same way.  Output: ONE JSON line.  The unfolded forward is the path every earlier commit ran, so the ratio needs no second box.

  --3d    the 3-D models instead (BatchNorm3d folded into the I3D backbone's kernels, infer3d.fold_batchnorm): cfg4 112 x 112 x 96 and cfg5 128^3 at batch 4
          and batch 1, each six-term and under inference_precision('bf16x3'); per case the median and quartiles of `reps` alternating forwards of one model after
          `warmup` pairs (every switch of variant is followed by one untimed forward: a new fold fills its operand cache at its first call), and the device launches of one forward of each variant (torch.profiler, after the timing).  Written to --out
          (profiles/fold_infer_bench_3d.json) and printed as one JSON line.
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


def count_kernels(fn):
    """device kernels of one call (None where the profiler is not usable)"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA'))
    except Exception as exc:                                   # a figure for the report, not a measurement the ratios rest on
        print('launch count unavailable: %r' % (exc,), file=sys.stderr)
        return None


def _quartiles(v):
    q1, q2, q3 = statistics.quantiles(v, n=4)
    return [round(q1, 4), round(q2, 4), round(q3, 4)]


def main_3d(a):
    """the 3-D cases: one model per (configuration, batch); unfolded and folded forwards take turns inside each precision"""
    from segtran_amd import infer3d
    dev = torch.device('cuda', 0)
    out = {'tool': 'infer_bench --3d', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'cases': {}}
    for name in a.cfgs.split(','):
        c = engine.CONFIGS[name]
        for batch in (c['bs'], 1):
            net = engine.build_model(name, dev, dropout_prob=0.0).eval()
            x, _ = engine.synth_batch(name, batch, dev)

            def run():
                net(x)
            for precision in ('fp32', 'bf16x3'):
                ms = {False: [], True: []}
                with torch.no_grad(), infer3d.inference_precision(precision):
                    for i in range(a.warmup + a.reps):
                        for folded in (False, True):
                            (infer3d.fold_batchnorm if folded else infer3d.unfold_batchnorm)(net)
                            run()                               # untimed: the first forward after a fold fills its per-layer operand cache (unfolding drops it)
                            t = timed(run)
                            if i >= a.warmup:
                                ms[folded].append(t)
                    launches = {}
                    for folded in (False, True):
                        (infer3d.fold_batchnorm if folded else infer3d.unfold_batchnorm)(net)
                        run()                                   # (a fresh fold: the first call fills its operand cache)
                        launches[folded] = count_kernels(run)
                    infer3d.unfold_batchnorm(net)
                qu, qf = _quartiles(ms[False]), _quartiles(ms[True])
                out['cases']['%s_b%d_%s' % (name, batch, precision)] = {
                    'batch': batch, 'size': list(c['size']), 'precision': precision, 'unfolded_ms_q1_median_q3': qu, 'folded_ms_q1_median_q3': qf,
                    'folded_over_unfolded': round(qf[1] / qu[1], 4), 'quartiles_overlap': not (qf[2] < qu[0] or qu[2] < qf[0]),
                    'unfolded_launches': launches[False], 'folded_launches': launches[True]}
                print(name, batch, precision, out['cases']['%s_b%d_%s' % (name, batch, precision)], file=sys.stderr, flush=True)
            del net
            torch.cuda.empty_cache()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1, sort_keys=True) + '\n')
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--3d', dest='three_d', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cfgs', default='cfg1,cfg2,cfg3')
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--once', default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.once, 'the median is taken over at least 20 repetitions'
    if a.three_d:
        if a.cfgs == 'cfg1,cfg2,cfg3':
            a.cfgs = 'cfg4,cfg5'
        if a.out is None:
            a.out = os.path.join('profiles', 'fold_infer_bench_3d.json')
        return main_3d(a)
    dev = torch.device('cuda', 0)
    if a.once:
        name, variant = a.once.split(':')
        net = engine.build_model(name, dev, dropout_prob=0.0).eval()
        if variant == 'folded':
            if engine.CONFIGS[name]['dim'] == 3:
                from segtran_amd import infer3d
                infer3d.fold_batchnorm(net)
            else:
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
