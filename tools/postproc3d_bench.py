"""Connected-component post-processing of one BraTS case on the device: what the labelling and the rule cost, alone and inside the case evaluation,
next to the route a user had before -- preds_hard to the host, scipy.ndimage.label, back to the device.

  python tools/postproc3d_bench.py [--reps 10] [--warmup 3] [--out profiles/postproc3d_bench.json] [--parent-tree DIR] [--rounds 3]

One process, ONE cfg4 model (unfolded, fp32) on the synthetic 240 x 240 x 155 case of tools/case_bench3d.py (window 112 x 112 x 96, stride 56 / 48, batch 4).  Medians
over `reps` calls after `warmup`, timed with HIP events on the launch stream; the launches that take well under a millisecond are timed 20 calls to an event pair.
  label           segx_ccl3d alone (26- and 6-connectivity) on the WT channel of the case's prediction and on a blob mask (7^3 blocks at density 0.06 plus speckle)
  rule            SF.brats_postprocess with every option on, and SF.brats_relabel
  fused / graph   test_single_case(fused=True) + SF.brats_case_tail and the GraphedSlidingWindow3d replay, with and without postprocess=
  host_route      WT channel -> host, scipy.ndimage.label + bincount + the keep rule, keep mask -> device (where scipy imports; host clock around a synchronise)
--parent-tree DIR: a checkout of the parent commit with its library built.  The default path (postprocess=None) of the replay is then timed in fresh processes that
import the package from DIR and from this tree in turn, `rounds` times each (--replay-only is that child), and both sets of medians go into the result.
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE, WINDOW, STRIDE_XY, STRIDE_Z, BATCH = (240, 240, 155), (112, 112, 96), 56, 48, 4
POST = dict(wt_min_voxels=500, wt_largest_only=True, et_min_voxels=500, connectivity=26)
MANY = 20


def setup(tree):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, tree)
    import torch
    from segtran_amd import engine, infer3d
    from segtran_amd.synth import synth_brats
    dev = torch.device('cuda', 0)
    net = engine.build_model('cfg4', dev, dropout_prob=0.0).eval()
    x, lab = synth_brats(1, *IMAGE, 1337)
    image, mask = x[0].to(dev), lab[0].to(dev)
    mask[::2][mask[::2] == 3] = 4                               # raw BraTS files hold 4 for the enhancing tumour
    return torch, infer3d, net, image, mask


def medians(forms, warmup, reps):
    from sliding_bench import timed
    ms = {k: [] for k in forms}
    for i in range(warmup + reps):
        for k, fn in forms.items():
            t = timed(fn)
            if i >= warmup:
                ms[k].append(t)
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}, {k: round(min(v), 4) for k, v in ms.items()}


def replay_only(a):
    """the child of the parent / this-tree comparison: the default replay, nothing of the new interface"""
    torch, infer3d, net, image, mask = setup(os.path.abspath(a.tree))
    graph = infer3d.GraphedSlidingWindow3d(net, image.shape, WINDOW, WINDOW, BATCH, STRIDE_XY, STRIDE_Z, fold_bn=False, with_mask=True)
    med, low = medians({'replay': lambda: graph(image, mask)}, a.warmup, a.reps)
    counts = graph(image, mask)[3].cpu().tolist()
    graph.close()
    print(json.dumps({'tree': a.tree, 'replay_ms': med['replay'], 'min_ms': low['replay'], 'counts': counts}))


def against_parent(a):
    runs = {'parent': [], 'this': []}
    trees = {'parent': os.path.abspath(a.parent_tree), 'this': ROOT}
    for _ in range(a.rounds):
        for side in ('parent', 'this'):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--replay-only', '--tree', trees[side], '--reps', str(a.reps), '--warmup', str(a.warmup)],
                                 stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
            runs[side].append(json.loads(out.strip().splitlines()[-1]))
    res = {side: {'replay_ms': [r['replay_ms'] for r in v], 'median_ms': round(statistics.median(r['replay_ms'] for r in v), 4)} for side, v in runs.items()}
    res['counts_equal'] = all(r['counts'] == runs['parent'][0]['counts'] for v in runs.values() for r in v)
    spread = max(max(v['replay_ms']) - min(v['replay_ms']) for v in (res['parent'], res['this']))
    res['same_side_spread_ms'] = round(spread, 4)                # what two runs of the same code differ by: the noise band of this comparison
    res['this_minus_parent_ms'] = round(res['this']['median_ms'] - res['parent']['median_ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'postproc3d_bench.json'))
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--replay-only', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    a = ap.parse_args()
    assert a.reps >= 10, 'the median is taken over at least 10 repetitions'
    if a.replay_only:
        return replay_only(a)
    default_path = against_parent(a) if a.parent_tree else None           # before this process opens the device
    torch, infer3d, net, image, mask = setup(ROOT)
    from segtran_amd import functional as SF
    from segtran_amd import segx
    dev = image.device
    geo = (WINDOW, WINDOW, BATCH, STRIDE_XY, STRIDE_Z)
    L = segx.lib()
    hard, soft = infer3d.test_single_case(net, image, *geo, 'brats', fused=True)
    g = torch.Generator(device='cpu').manual_seed(3)
    blobs = (torch.rand(35, 35, 23, generator=g) < 0.06).to(dev).repeat_interleave(7, 0).repeat_interleave(7, 1).repeat_interleave(7, 2)[:240, :240, :155]
    blobs = (blobs | (torch.rand(*IMAGE, generator=g) < 0.002).to(dev)).float().contiguous()
    labels = torch.empty(IMAGE, dtype=torch.int32, device=dev)
    sizes = torch.empty(IMAGE, dtype=torch.int32, device=dev)

    def many(fn):
        def run():
            for _ in range(MANY):
                fn()
        return run
    small = {'label26_prediction': lambda: L.ccl3d(hard[2], 0, labels, sizes, 1, *IMAGE, 26), 'label6_prediction': lambda: L.ccl3d(hard[2], 0, labels, sizes, 1, *IMAGE, 6),
             'label26_blobs': lambda: L.ccl3d(blobs, 0, labels, sizes, 1, *IMAGE, 26), 'label6_blobs': lambda: L.ccl3d(blobs, 0, labels, sizes, 1, *IMAGE, 6),
             'rule': lambda: SF.brats_postprocess(hard, **POST)}
    hard_pp, flag = SF.brats_postprocess(hard, **POST)
    tail_labels = SF.brats_case_tail(soft, hard_pp)[1]
    small['relabel'] = lambda: SF.brats_relabel(tail_labels, hard_pp, flag)
    with torch.no_grad():
        med_small, _ = medians({k: many(fn) for k, fn in small.items()}, a.warmup, a.reps)
    med_small = {k: round(v / MANY, 4) for k, v in med_small.items()}
    _, s = SF.label_components3d(hard[2]); _, sb = SF.label_components3d(blobs)
    shape_of = {'prediction': {'wt_voxels': int(hard[2].sum()), 'components26': int((s > 0).sum())}, 'blobs': {'voxels': int(blobs.sum()), 'components26': int((sb > 0).sum())}}

    g_plain = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_mask=True)
    g_post = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_mask=True, postprocess=POST)

    def fused(post):
        def run():
            h, sft = infer3d.test_single_case(net, image, *geo, 'brats', fused=True)
            f = None
            if post:
                h, f = SF.brats_postprocess(h, **POST)
            counts, lab = SF.brats_case_tail(sft, h, mask)
            return SF.brats_relabel(lab, h, f, out=lab) if post else lab
        return run
    big = {'fused': fused(False), 'fused_postprocess': fused(True), 'graph': lambda: g_plain(image, mask), 'graph_postprocess': lambda: g_post(image, mask)}
    med_big, min_big = medians(big, a.warmup, a.reps)
    same = bool(torch.equal(g_post(image, mask)[0], hard_pp))
    g_plain.close(); g_post.close()

    host = None
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        struct = ndimage.generate_binary_structure(3, 3)

        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wt = hard[2].cpu().numpy()                          # device -> host
            lab, n = ndimage.label(wt, structure=struct)
            count = np.bincount(lab.reshape(-1))
            count[0] = 0
            stay = (count >= POST['wt_min_voxels']) & (np.arange(n + 1) == count.argmax())
            keep = torch.from_numpy(stay[lab]).to(dev)          # host -> device
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, keep
        times = [host_route()[0] for _ in range(a.warmup + a.reps)][a.warmup:]
        host = {'ms': round(statistics.median(times), 3), 'min_ms': round(min(times), 3), 'labeller': 'scipy.ndimage.label',
                'keep_equal_device': bool(torch.equal(host_route()[1], hard_pp[2] != 0))}
    res = {'tool': 'postproc3d_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'model': 'cfg4', 'image': list(IMAGE),
           'window': list(WINDOW), 'stride': [STRIDE_XY, STRIDE_Z], 'batch': BATCH, 'postprocess': POST, 'masks': shape_of, 'calls_per_event_pair': MANY,
           'ms': dict(med_small, **med_big), 'min_ms': min_big, 'postprocess_cost_ms': {'fused': round(med_big['fused_postprocess'] - med_big['fused'], 4),
                                                                                         'graph': round(med_big['graph_postprocess'] - med_big['graph'], 4)},
           'graph_postprocess_equals_eager_rule': same, 'host_route': host if host is not None else 'not measured: scipy does not import here',
           'default_path_vs_parent': default_path if default_path is not None else 'not measured: no --parent-tree'}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
