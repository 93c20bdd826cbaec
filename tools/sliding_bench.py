"""Sliding-window evaluation of a 2-D image batch: the eager window loop against the fused sequence and its hipGraph replay.

  python tools/sliding_bench.py [--reps 20] [--warmup 5] [--cases cfg1,cfg2] [--out profiles/sliding_infer_bench.json] [--launches]

One process.  Per case ONE model, folded once up front (so that no form pays for a fold per call), and the forms take turns -- warm-up rounds, then `reps` rounds, every
call timed with HIP events on the launch stream; medians and their ratios to the eager form are reported:
  eager         infer2d.test_single_batch(fold_bn=True): crop + forward + window_accum per window, harden_segmap (the path every earlier commit ran)
  fused         the same with fused=True: window_gather, the forward on the windows stacked (as many per call as the library's plane limit allows: cfg1 runs
                16 windows as 12 + 4, cfg2 its 9 windows in one call), window_merge
  fused_wb1     fused=True, window_batch=1: one forward per window (the eager path's GEMM shapes)
  graph         GraphedSlidingWindow replay, windows stacked as in `fused`
  graph_wb1     GraphedSlidingWindow replay, window_batch=1
Cases: cfg1 model, 576 x 576 image, batch 2 (256 x 256 windows, stride 128); cfg2 model, 1024 x 1024 image, batch 1 (512 x 512 windows, stride 256).
--launches: additionally count the device kernels of one call of every form with torch.profiler (after the timing, so it cannot disturb it).
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, infer2d                        # noqa: E402

CASES = {'cfg1': dict(model='cfg1', image=576, batch=2), 'cfg2': dict(model='cfg2', image=1024, batch=1)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cases', default='cfg1,cfg2')
    ap.add_argument('--out', default=os.path.join('profiles', 'sliding_infer_bench.json'))
    ap.add_argument('--launches', action='store_true')
    a = ap.parse_args()
    assert a.reps >= 20, 'the median is taken over at least 20 repetitions'
    dev = torch.device('cuda', 0)
    out = {'tool': 'sliding_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'cases': {}}
    for name in a.cases.split(','):
        case = CASES[name]
        c = engine.CONFIGS[case['model']]
        S = c['size'][0]
        net = engine.build_model(case['model'], dev, dropout_prob=0.0).eval()
        net.fold_batchnorm()
        img, _ = engine.synth_batch(dict(c, size=(case['image'],) * 2), case['batch'], dev)
        geo = dict(orig_input_size=(S, S), patch_size=(S, S), stride=(S // 2, S // 2))
        kw = dict(geo, task_name=c['task'], num_classes=c['num_classes'], fold_bn=True)
        graphs = {'graph': infer2d.GraphedSlidingWindow(net, img.shape, num_classes=c['num_classes'], **geo),
                  'graph_wb1': infer2d.GraphedSlidingWindow(net, img.shape, num_classes=c['num_classes'], window_batch=1, **geo)}
        forms = {'eager': lambda: infer2d.test_single_batch(net, img, **kw),
                 'fused': lambda: infer2d.test_single_batch(net, img, fused=True, **kw),
                 'fused_wb1': lambda: infer2d.test_single_batch(net, img, fused=True, window_batch=1, **kw),
                 'graph': lambda: graphs['graph'](img),
                 'graph_wb1': lambda: graphs['graph_wb1'](img)}
        ms = {k: [] for k in forms}
        for i in range(a.warmup + a.reps):
            for k, fn in forms.items():
                t = timed(fn)
                if i >= a.warmup:
                    ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        # the forms compute the same thing: say how far apart they are
        ref_hard, ref_soft = forms['eager']()
        diff = {}
        for k in ('fused', 'fused_wb1', 'graph', 'graph_wb1'):
            hard, soft = forms[k]()
            diff[k] = {'max_abs_soft_diff': float((soft - ref_soft).abs().max()), 'labels_differing': int((hard != ref_hard).sum())}
        res = {'model': case['model'], 'image': [case['image']] * 2, 'batch': case['batch'], 'window': [S, S], 'stride': [S // 2, S // 2],
               'windows': graphs['graph'].plan.table.nwin,
               'ms': {k: round(v, 4) for k, v in med.items()}, 'min_ms': {k: round(min(v), 4) for k, v in ms.items()},
               'over_eager': {k: round(med[k] / med['eager'], 4) for k in med}, 'vs_eager': diff,
               'window_batch': graphs['graph'].plan.window_batch, 'graph_not_slower_than_eager': bool(med['graph'] <= med['eager'])}
        if a.launches:
            res['device_kernels_per_call'] = {k: count_kernels(fn) for k, fn in forms.items()}
        out['cases'][name] = res
        for g in graphs.values():
            g.close()
        del net, graphs, forms
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
