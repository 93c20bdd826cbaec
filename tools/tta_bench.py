"""Flip test-time augmentation of the sliding-window evaluation: the loop a user writes around the fused evaluation against tta= and its hipGraph replay.

  python tools/tta_bench.py [--reps 10] [--warmup 3] [--cases 2d,3d] [--out profiles/tta_bench.json]

One process.  Per case ONE model; the forms take turns -- warm-up rounds, then `reps` rounds, every call timed with HIP events on the launch stream; medians, minima and the
ratios to the composed form are reported:
  composed  per view: torch.flip of the image, the fused evaluation (test_single_batch / test_single_case with fused=True), torch.flip of preds_soft; the adds in view
            order and the division in ATen; SF.harden_segmap on the mean
  fused     the same entry point with fused=True, tta=views: one gather launch for all views, the same forwards, one merge launch
  graph     GraphedSlidingWindow / GraphedSlidingWindow3d built with tta=views: a replay
Cases: 2d -- cfg1 model (BatchNorm folded once up front), a 576 x 576 batch of 6, 256 x 256 windows at stride 128, views (), (1,), (0,), (0, 1);
       3d -- cfg4 model, a 240 x 240 x 155 case, 112 x 112 x 96 windows at stride 56 / 48, batch 4, views (), (0,).
The forwards are the same in all three forms and dominate; what differs is the flips, the per-view merges, the adds and the host's launches.  After the timing every form's
result is compared with the composed one.
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, infer2d, infer3d               # noqa: E402
from segtran_amd import functional as SF                       # noqa: E402
from segtran_amd.synth import synth_brats                      # noqa: E402
from sliding_bench import timed                                # noqa: E402

VIEWS_2D = ((), (1,), (0,), (0, 1))
VIEWS_3D = ((), (0,))
IMAGE_3D, WINDOW_3D, STRIDE_XY, STRIDE_Z, BATCH_3D = (240, 240, 155), (112, 112, 96), 56, 48, 4


def composed(evaluate, image, views, first_axis, mode):
    """the loop tta= replaces, around the FUSED evaluation"""
    total = None
    for view in views:
        dims = tuple(first_axis + a for a in view)
        _, soft = evaluate(torch.flip(image, dims) if dims else image)
        soft = torch.flip(soft, dims) if dims else soft
        total = soft if total is None else total + soft
    mean = total / total.new_full((), float(len(views)))
    soft, hard = SF.harden_segmap(mean if first_axis == 2 else mean.unsqueeze(0), mode=mode)
    return (hard, soft) if first_axis == 2 else (hard[0], soft[0])


def measure(forms, reps, warmup):
    ms = {k: [] for k in forms}
    for i in range(warmup + reps):
        for k, fn in forms.items():
            t = timed(fn)
            if i >= warmup:
                ms[k].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ref_hard, ref_soft = forms['composed']()
    diff = {}
    for k in ('fused', 'graph'):
        hard, soft = forms[k]()[:2]
        diff[k] = {'soft_equal': bool(torch.equal(soft, ref_soft)), 'max_abs_soft_diff': float((soft - ref_soft).abs().max()),
                   'labels_differing': int((hard.float() != ref_hard.float()).sum())}
    return {'ms': {k: round(v, 3) for k, v in med.items()}, 'min_ms': {k: round(min(v), 3) for k, v in ms.items()},
            'over_composed': {k: round(med[k] / med['composed'], 4) for k in med}, 'vs_composed': diff,
            'fused_not_slower_than_composed': bool(med['fused'] <= med['composed']), 'graph_not_slower_than_composed': bool(med['graph'] <= med['composed'])}


def case_2d(dev, reps, warmup):
    c = engine.CONFIGS['cfg1']
    S = c['size'][0]
    net = engine.build_model('cfg1', dev, dropout_prob=0.0).eval()
    net.fold_batchnorm()
    img, _ = engine.synth_batch(dict(c, size=(576, 576)), 6, dev)
    geo = dict(orig_input_size=(S, S), patch_size=(S, S), stride=(S // 2, S // 2))
    kw = dict(geo, task_name=c['task'], num_classes=c['num_classes'], fused=True)
    graph = infer2d.GraphedSlidingWindow(net, img.shape, num_classes=c['num_classes'], tta=VIEWS_2D, **geo)
    with torch.no_grad():
        forms = {'composed': lambda: composed(lambda x: infer2d.test_single_batch(net, x, **kw), img, VIEWS_2D, 2, 0),
                 'fused': lambda: infer2d.test_single_batch(net, img, tta=VIEWS_2D, **kw),
                 'graph': lambda: graph(img)}
        res = dict(model='cfg1', image=[576, 576], batch=6, window=[S, S], stride=[S // 2, S // 2], views=[list(v) for v in VIEWS_2D],
                   windows=graph.plan.table.nwin, window_batch=graph.plan.window_batch, **measure(forms, reps, warmup))
    graph.close()
    return res


def case_3d(dev, reps, warmup):
    net = engine.build_model('cfg4', dev, dropout_prob=0.0).eval()
    x, _ = synth_brats(1, *IMAGE_3D, 1337)
    image = x[0].to(dev)
    geo = (WINDOW_3D, WINDOW_3D, BATCH_3D, STRIDE_XY, STRIDE_Z)
    graph = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_labels=False, tta=VIEWS_3D)
    with torch.no_grad():
        forms = {'composed': lambda: composed(lambda v: infer3d.test_single_case(net, v, *geo, 'brats', fused=True), image, VIEWS_3D, 1, 1),
                 'fused': lambda: infer3d.test_single_case(net, image, *geo, 'brats', fused=True, tta=VIEWS_3D),
                 'graph': lambda: graph(image)}
        res = dict(model='cfg4', image=list(IMAGE_3D), window=list(WINDOW_3D), stride=[STRIDE_XY, STRIDE_Z], batch=BATCH_3D, views=[list(v) for v in VIEWS_3D],
                   windows=graph.plan.table.nwin, net_calls=len(graph.plan.chunks), **measure(forms, reps, warmup))
    graph.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cases', default='2d,3d')
    ap.add_argument('--out', default=os.path.join('profiles', 'tta_bench.json'))
    a = ap.parse_args()
    assert a.reps >= 10, 'the median is taken over at least 10 repetitions'
    dev = torch.device('cuda', 0)
    out = {'tool': 'tta_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'cases': {}}
    for name in a.cases.split(','):
        out['cases'][name] = {'2d': case_2d, '3d': case_3d}[name](dev, a.reps, a.warmup)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
