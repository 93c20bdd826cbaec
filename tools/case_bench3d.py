"""Evaluation of one BraTS case: the eager window loop with the ATen tail against the fused sequence with the tail kernel and against the hipGraph replay.

  python tools/case_bench3d.py [--reps 10] [--warmup 3] [--out profiles/case3d_bench.json] [--no-launches]

One process, ONE cfg4 model (unfolded, fp32) on a synthetic 240 x 240 x 155 case: window 112 x 112 x 96, stride 56 / 48, batch 4 -- 48 windows in 12 net() calls (each
of the four x rows of 12 windows runs as three batches of 4).  The forms take turns -- warm-up rounds, then `reps` rounds, every call timed with HIP events on the launch stream;
medians and their ratios to the eager form are reported.  Every form ends with the case's metrics inputs and the export label volume on the device:
  eager   infer3d.test_single_case (canvas copy, crop + forward + window_accum per window, harden_segmap, clone) and the tail from ATen calls: brats_map_label,
          calculate_metric_percase, brats_inv_map_label + argmax + the 3 -> 4 relabel (the path the commit before this tool ran)
  fused   test_single_case(fused=True) (window_gather, the same 12 forwards, window_merge) and SF.brats_case_tail
  graph   GraphedSlidingWindow3d(with_mask=True) replay: gather, forwards, merge and tail as one graph launch
The device kernels of one call of every form are counted with torch.profiler after the timing (--no-launches skips that).
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, infer3d                        # noqa: E402
from segtran_amd import functional as SF                       # noqa: E402
from segtran_amd import test_util3d as T3                      # noqa: E402
from segtran_amd.dataloaders import datasets3d as D3           # noqa: E402
from segtran_amd.synth import synth_brats                      # noqa: E402
from sliding_bench import timed, count_kernels                 # noqa: E402

IMAGE, WINDOW, STRIDE_XY, STRIDE_Z, BATCH = (240, 240, 155), (112, 112, 96), 56, 48, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'case3d_bench.json'))
    ap.add_argument('--no-launches', action='store_true')
    a = ap.parse_args()
    assert a.reps >= 10, 'the median is taken over at least 10 repetitions'
    dev = torch.device('cuda', 0)
    net = engine.build_model('cfg4', dev, dropout_prob=0.0).eval()
    x, lab = synth_brats(1, *IMAGE, 1337)
    image, mask = x[0].to(dev), lab[0].to(dev)
    mask[::2][mask[::2] == 3] = 4                               # raw BraTS files hold 4 for the enhancing tumour
    geo = (WINDOW, WINDOW, BATCH, STRIDE_XY, STRIDE_Z)
    graph = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_mask=True)

    def eager():
        hard, soft = infer3d.test_single_case(net, image, *geo, 'brats')
        m = mask.long()
        gt = D3.brats_map_label((m - (m == 4).long()).unsqueeze(0).float())[0]
        metric = T3.calculate_metric_percase(hard, gt, 4)
        out = torch.argmax(D3.brats_inv_map_label(soft), dim=0)
        out += (out == 3).long()
        return hard, soft, out, metric

    def fused():
        hard, soft = infer3d.test_single_case(net, image, *geo, 'brats', fused=True)
        counts, labels = SF.brats_case_tail(soft, hard, mask)
        return hard, soft, labels, counts

    forms = {'eager': eager, 'fused': fused, 'graph': lambda: graph(image, mask)}
    ms = {k: [] for k in forms}
    for i in range(a.warmup + a.reps):
        for k, fn in forms.items():
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the forms compute the same thing: say so
    ref_hard, ref_soft, ref_labels, (ref_metric, ref_valid) = eager()
    same = {}
    for k in ('fused', 'graph'):
        hard, soft, labels, counts = forms[k]()
        metric, valid = infer3d.case_metrics(counts)
        same[k] = {'soft_equal': bool(torch.equal(soft, ref_soft)), 'hard_equal': bool(torch.equal(hard, ref_hard)),
                   'labels_equal': bool(torch.equal(labels.long(), ref_labels)),
                   'max_abs_metric_diff': float(abs(metric - ref_metric).max()), 'valid_equal': bool((valid == ref_valid).all())}
    res = {'tool': 'case_bench3d', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'model': 'cfg4', 'image': list(IMAGE),
           'window': list(WINDOW), 'stride': [STRIDE_XY, STRIDE_Z], 'batch': BATCH, 'windows': graph.plan.table.nwin, 'net_calls': len(graph.plan.chunks),
           'ms': {k: round(v, 3) for k, v in med.items()}, 'min_ms': {k: round(min(v), 3) for k, v in ms.items()},
           'over_eager': {k: round(med[k] / med['eager'], 4) for k in med}, 'vs_eager': same,
           'graph_not_slower_than_eager': bool(med['graph'] <= med['eager'])}
    if not a.no_launches:
        res['device_kernels_per_case'] = {k: count_kernels(fn) for k, fn in forms.items()}
    graph.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
