"""Lesion-wise evaluation of one BraTS case on the device: what each kernel and the whole call cost, alone and inside the case evaluation, next to
the route a user had before -- the regions to the host, scipy.ndimage.binary_dilation and label per region.

  python tools/lesionwise_bench.py [--reps 10] [--warmup 3] [--out profiles/lesionwise_bench.json] [--parent-tree DIR] [--rounds 4]

One process, ONE cfg4 model (unfolded, fp32) on the synthetic 240 x 240 x 155 case of tools/case_bench3d.py (window 112 x 112 x 96, stride 56 / 48, batch 4).  Medians
over `reps` calls after `warmup`, timed with HIP events on the launch stream; the launches that take about a millisecond or less are timed 20 calls to an event pair.
  kernels         on a constructed case -- a few nested ET < TC < WT blobs per region, the prediction a shifted copy with two stray components --: segx_dilate3d
                  (3 iterations, 18 neighbours, raw labels -> three regions), segx_ccl3d of the dilated stack and of the prediction, segx_lesion_match (the time of
                  restoring the two size arrays it consumes is measured alone and taken off), segx_lesion_reduce
  call            infer3d.lesionwise_metrics on that case, its device-to-host copy included
  host_route      the same rows from scipy.ndimage (where scipy imports; host clock around a synchronise), and whether they equal the device's
  graph           the GraphedSlidingWindow3d replay with and without lesionwise=
--parent-tree DIR: a checkout of the parent commit with its library built.  The default replay (lesionwise=None) is then timed in fresh processes that import the
package from DIR and from this tree in turn, `rounds` times each (--replay-only is that child); the run-to-run spread is the PARENT's own (max - min of its medians).
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from postproc3d_bench import BATCH, IMAGE, STRIDE_XY, STRIDE_Z, WINDOW, medians, setup      # noqa: E402

LW = dict(dilation_iters=3, dilation_connectivity=18, connectivity=26, min_lesion_voxels=0)
MANY = 20


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
    lo, hi = min(res['parent']['replay_ms']), max(res['parent']['replay_ms'])
    res['parent_spread_ms'] = round(hi - lo, 4)                  # what repeated medians of the PARENT differ by: the band the default path has to stay in
    res['this_minus_parent_ms'] = round(res['this']['median_ms'] - res['parent']['median_ms'], 4)
    res['this_inside_parent_spread'] = bool(lo <= res['this']['median_ms'] <= hi)
    return res


def constructed_case(torch, dev):
    """(raw labels int32 [X, Y, Z], prediction float [3, X, Y, Z]): five nested blobs (WT 30^3 > TC 18^3 > ET 8^3) and three small WT-only ones; the prediction is the
    ground truth moved by (3, 2, 4) without its last blob, plus two stray components"""
    raw = torch.zeros(IMAGE, dtype=torch.int32, device=dev)
    for cx, cy, cz in ((50, 60, 40), (120, 120, 80), (180, 70, 110), (70, 180, 60), (190, 190, 30)):
        raw[cx - 15:cx + 15, cy - 15:cy + 15, cz - 15:cz + 15] = 2
        raw[cx - 9:cx + 9, cy - 9:cy + 9, cz - 9:cz + 9] = 1
        raw[cx - 4:cx + 4, cy - 4:cy + 4, cz - 4:cz + 4] = 4
    small = ((20, 20, 20), (220, 30, 140), (30, 220, 100))
    for cx, cy, cz in small:
        raw[cx:cx + 5, cy:cy + 5, cz:cz + 5] = 2
    moved = torch.zeros_like(raw)
    moved[3:, 2:, 4:] = raw[:-3, :-2, :-4]
    cx, cy, cz = small[-1]
    moved[cx:cx + 10, cy:cy + 10, cz:cz + 10] = 0
    moved[120:126, 20:26, 20:26] = 4
    moved[20:24, 120:124, 130:134] = 2
    pred = torch.stack([moved == 4, (moved >= 1) & (moved <= 4), (moved == 1) | (moved == 4)]).float().contiguous()
    return raw, pred


def host_rows(np, ndimage, pred, raw):
    """the definition through scipy, per region: [n, 4] rows sorted by root label, (n_fp, fp_voxels)"""
    lab = np.where(raw == 4, 3, raw)
    regions = (lab == 3, (lab >= 1) & (lab <= 3), (lab == 1) | (lab == 3))
    st = ndimage.generate_binary_structure(3, 3)
    out = []
    for g, p in zip(regions, pred):
        p = p != 0
        gd = ndimage.binary_dilation(g, ndimage.generate_binary_structure(3, 2), iterations=LW['dilation_iters'])
        GL, n = ndimage.label(gd, structure=st)
        PL, m = ndimage.label(p, structure=st)
        psize = np.bincount(PL.reshape(-1), minlength=m + 1)
        first = np.full(n + 1, GL.size, dtype=np.int64)
        np.minimum.at(first, GL.reshape(-1), np.arange(GL.size))
        gvol = np.bincount(GL[g], minlength=n + 1)
        tp = np.bincount(GL[g & p], minlength=n + 1)
        both = (GL > 0) & (PL > 0)
        pairs = np.unique(np.stack([GL[both], PL[both]], 1), axis=0)
        pvol = np.zeros(n + 1, dtype=np.int64)
        np.add.at(pvol, pairs[:, 0], psize[pairs[:, 1]])
        rows = np.stack([first[1:] + 1, tp[1:], gvol[1:], pvol[1:]], 1)
        fp = np.setdiff1d(np.arange(1, m + 1), pairs[:, 1])
        out.append((rows[np.argsort(rows[:, 0])], (len(fp), int(psize[fp].sum()))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'lesionwise_bench.json'))
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--rounds', type=int, default=4)
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
    raw, pred = constructed_case(torch, dev)
    X, Y, Z = IMAGE
    S = X * Y * Z
    kern = {k: v for k, v in LW.items() if k != 'min_lesion_voxels'}

    gd, tmp = torch.empty((3,) + IMAGE, dtype=torch.uint8, device=dev), torch.empty((3,) + IMAGE, dtype=torch.uint8, device=dev)
    gl, gs, pl, ps = (torch.empty((3,) + IMAGE, dtype=torch.int32, device=dev) for _ in range(4))
    ws = torch.empty(L.lesion_ws_bytes(3), dtype=torch.uint8, device=dev)
    rows = torch.empty(3, L.LESION_MAX_GT, 4, dtype=torch.int32, device=dev)
    header = torch.empty(3, L.LESION_HEADER, dtype=torch.int32, device=dev)
    L.dilate3d(raw, 1, gd, tmp, 3, X, Y, Z, LW['dilation_connectivity'], LW['dilation_iters'])
    L.ccl3d(gd, 0, gl, gs, 3, X, Y, Z, LW['connectivity'])
    L.ccl3d(pred, 0, pl, ps, 3, X, Y, Z, LW['connectivity'])
    gs0, ps0 = gs.clone(), ps.clone()

    def restore():
        gs.copy_(gs0); ps.copy_(ps0)

    def match():
        restore()
        L.lesion_match(raw, 1, gl, gs, pl, ps, ws, 3, S)

    def many(fn):
        def run():
            for _ in range(MANY):
                fn()
        return run
    small = {'dilate': lambda: L.dilate3d(raw, 1, gd, tmp, 3, X, Y, Z, LW['dilation_connectivity'], LW['dilation_iters']),
             'label_dilated': lambda: L.ccl3d(gd, 0, gl, gs, 3, X, Y, Z, LW['connectivity']), 'label_prediction': lambda: L.ccl3d(pred, 0, pl, ps, 3, X, Y, Z, LW['connectivity']),
             'restore_sizes': restore, 'restore_and_match': match, 'reduce': lambda: L.lesion_reduce(ws, rows, header, 3),
             'lesion_rows': lambda: SF.lesion_rows(pred, raw, gt_map='brats', **kern)}
    with torch.no_grad():
        med_small, _ = medians({k: many(fn) for k, fn in small.items()}, a.warmup, a.reps)
    med_small = {k: round(v / MANY, 4) for k, v in med_small.items()}
    med_small['match'] = round(med_small['restore_and_match'] - med_small['restore_sizes'], 4)
    nhot = torch.stack([(raw == 3) | (raw == 4), (raw >= 1) & (raw <= 4), (raw == 1) | (raw == 3) | (raw == 4)])
    med_call, _ = medians({'lesionwise_metrics': lambda: infer3d.lesionwise_metrics(pred, nhot, **LW)}, a.warmup, a.reps)
    result = infer3d.lesionwise_metrics(pred, nhot, **LW)
    mapped = infer3d.lesionwise_from_tables(*SF.lesion_rows(pred, raw, gt_map='brats', **kern))
    case = [{'lesions': len(r['lesions']), 'n_fp': r['n_fp'], 'n_detected': r['n_detected'], 'lesion_dice': r['lesion_dice']} for r in result]
    map_equal = all((x['lesions'] == y['lesions']).all() and x['lesion_dice'] == y['lesion_dice'] for x, y in zip(result, mapped))

    g_plain = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_mask=True)
    g_lw = infer3d.GraphedSlidingWindow3d(net, image.shape, *geo, fold_bn=False, with_mask=True, lesionwise=LW)
    med_big, min_big = medians({'graph': lambda: g_plain(image, mask), 'graph_lesionwise': lambda: g_lw(image, mask)}, a.warmup, a.reps)
    hard = g_lw(image, mask)[0]
    head = g_lw.lesion_header.cpu().tolist()
    net_shape = [{'lesions': h[0], 'pred_components': h[1], 'n_fp': h[2], 'overflow': h[4]} for h in head]          # the synthetic-weight network's own prediction
    graph_equal = None
    if not any(h[4] for h in head):
        net_case = infer3d.lesionwise_from_tables(g_lw.lesion_rows, g_lw.lesion_header)
        direct = infer3d.lesionwise_from_tables(*SF.lesion_rows(hard[1:4], mask, gt_map='brats', **kern))
        graph_equal = all((x['lesions'] == y['lesions']).all() and x['n_fp'] == y['n_fp'] for x, y in zip(net_case, direct))
    g_plain.close(); g_lw.close()

    host = None
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        def host_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = host_rows(np, ndimage, pred.cpu().numpy(), raw.cpu().numpy())       # device -> host, then scipy
            return (time.perf_counter() - t0) * 1e3, out
        runs = [host_route() for _ in range(3)]
        times, got = [r[0] for r in runs[1:]], runs[-1][1]
        host = {'ms': round(statistics.median(times), 3), 'min_ms': round(min(times), 3), 'runs': len(times), 'library': 'scipy.ndimage binary_dilation + label',
                'rows_equal_device': all(np.array_equal(h[0], r['lesions']) and h[1] == (r['n_fp'], r['fp_voxels']) for h, r in zip(got, result))}
    res = {'tool': 'lesionwise_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'model': 'cfg4', 'image': list(IMAGE),
           'window': list(WINDOW), 'stride': [STRIDE_XY, STRIDE_Z], 'batch': BATCH, 'lesionwise': LW, 'calls_per_event_pair': MANY, 'constructed_case': case,
           'brats_map_equals_nhot': bool(map_equal), 'network_case': net_shape, 'graph_tables_equal_direct_call': graph_equal,
           'ms': dict(med_small, **med_call, **med_big), 'min_ms': min_big, 'lesionwise_cost_in_graph_ms': round(med_big['graph_lesionwise'] - med_big['graph'], 4),
           'host_route': host if host is not None else 'not measured: scipy does not import here',
           'default_path_vs_parent': default_path if default_path is not None else 'not measured: no --parent-tree'}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
