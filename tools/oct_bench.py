"""The class cap raised to 16 and the one-hot evaluation tail, timed on the device.

  python tools/oct_bench.py [--parent-lib PATH/libsegx.so] [--groups 7] [--reps 20] [--inner 10] [--out profiles/oct_bench.json]

(a) Regression at C <= 8: segx_window_merge and segx_harden_segmap at C = 3 on a 576 x 576 batch of 6 -- four overlapping 384 x 384 windows (stride 192), scores at
    the window's size ('same') and at half of it ('resampled') -- through the library of THIS tree and through --parent-lib, a build of the parent commit's sources
    (both loaded into this one process; the same tensors, the calls alternating).  A timing is `inner` launches between two HIP events; a group is the median of
    `reps` timings; `groups` groups per library.  The spread of the parent is the range of its group medians; `within_parent_spread` says whether this tree's median
    group lies at or below the parent's slowest group.  Without --parent-lib only this tree is timed and the comparison is reported as null.
(b) The fused tail at C = 10: SF.onehot_case_tail (counts, labels and rgb in one launch) on a 288 x 512 batch of 6 against the composed calls -- harden_segmap,
    index_onehot, dice_scores on the foreground planes of every image (calc_batch_metric's launches, without its per-image reads to the host), onehot_inv_map with
    the colour table.  Reported; there is no threshold.  The two forms' results are compared.
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import functional as SF, segx                 # noqa: E402
from segtran_amd.dataloaders import datasets2d as D2           # noqa: E402
from segtran_amd.synth import synth_oct_mask                   # noqa: E402
from sliding_bench import timed                                # noqa: E402

IMAGE, WINDOW, STRIDE, BATCH = (576, 576), (384, 384), 192, 6
OCT_IMAGE, OCT_CLASSES = (288, 512), 10


def group_medians(forms, groups, reps, inner, warmup=3):
    """{name: [median ms per call of each group]}: the forms take turns inside every repetition"""
    out = {k: [] for k in forms}
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(groups):
        ms = {k: [] for k in forms}
        for _ in range(reps):
            for k, fn in forms.items():
                ms[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
        for k in forms:
            out[k].append(statistics.median(ms[k]))
    return out


def regression(libs, a, dev):
    C, B = 3, BATCH
    origins = [(y, x) for y in (0, STRIDE) for x in (0, STRIDE)]
    table = SF.WindowTable(origins, dev)
    g = torch.Generator(device='cpu').manual_seed(3)
    soft, hard = torch.empty(B, C, *IMAGE, device=dev), torch.empty(B, C, *IMAGE, device=dev)
    acc = torch.rand(B, C, *IMAGE, generator=g).to(dev)
    geom = lambda s: (1,) + s + (1,) + WINDOW + (1,) + IMAGE + (0, 0, 0) + (1,) + IMAGE      # noqa: E731
    res = {}
    for case, size in (('same', WINDOW), ('resampled', (WINDOW[0] // 2, WINDOW[1] // 2))):
        scores = (torch.randn(len(origins) * B, C, *size, generator=g) * 2).to(dev)
        forms, outs = {}, {}
        for name, L in libs.items():
            forms['window_merge/' + name] = lambda L=L: L.window_merge(scores, table.dev, table.host, soft, hard, table.nwin, B, C, geom(size), 0, 0.5)
            forms['harden/' + name] = lambda L=L: L.harden_segmap(acc, None, soft, hard, B, C, IMAGE[0] * IMAGE[1], 0, 0.5)
        for k, fn in forms.items():                                              # the libraries compute the same bits: say so
            fn()
            outs[k] = (soft.clone(), hard.clone())
        med = group_medians(forms, a.groups, a.reps, a.inner)
        entry = {}
        for op in ('window_merge', 'harden'):
            new = med[op + '/this']
            e = {'this_ms': round(statistics.median(new), 5), 'this_groups_ms': [round(v, 5) for v in new]}
            if 'parent' in libs:
                old = med[op + '/parent']
                e.update(parent_ms=round(statistics.median(old), 5), parent_groups_ms=[round(v, 5) for v in old], parent_spread_ms=[round(min(old), 5), round(max(old), 5)],
                         this_over_parent=round(statistics.median(new) / statistics.median(old), 4), within_parent_spread=bool(statistics.median(new) <= max(old)),
                         bit_identical=bool(torch.equal(outs[op + '/this'][0], outs[op + '/parent'][0]) and torch.equal(outs[op + '/this'][1], outs[op + '/parent'][1])))
            entry[op] = e
        res[case] = entry
    res['harden'] = res['same'].pop('harden')                                   # harden does not depend on the scores' size: keep the first timing only
    res['resampled'].pop('harden')
    return res


def fused_tail(a, dev):
    C, B, (H, W) = OCT_CLASSES, BATCH, OCT_IMAGE
    g = torch.Generator(device='cpu').manual_seed(4)
    soft = torch.rand(B, C, H, W, generator=g).pow(2).to(dev)
    gt = synth_oct_mask(B, H, W, C, 9)[:, 0].contiguous().to(dev)
    cmap = torch.randint(0, 256, (C, 3), generator=g).to(torch.uint8).to(dev)

    def composed():
        hard = SF.harden_segmap(soft, mode=0, want_soft=False)[1]
        nh = SF.index_onehot(gt, C)
        dice = torch.stack([SF.dice_scores(hard[b, 1:].reshape(C - 1, -1), nh[b, 1:].reshape(C - 1, -1)) for b in range(B)])    # per image, as calc_batch_metric
        return dice, D2.onehot_inv_map(hard, cmap)

    def fused():
        counts, labels, rgb = SF.onehot_case_tail(soft, gt, cmap)
        c = counts.float()
        return (2 * c[..., 0] + 1e-5) / (c[..., 1] + c[..., 2] + 1e-5), rgb

    med = group_medians({'composed': composed, 'fused': fused}, a.groups, a.reps, a.inner)
    (d0, r0), (d1, r1) = composed(), fused()
    m = {k: statistics.median(v) for k, v in med.items()}
    return {'image': [H, W], 'batch': B, 'classes': C, 'composed_ms': round(m['composed'], 5), 'fused_ms': round(m['fused'], 5),
            'fused_over_composed': round(m['fused'] / m['composed'], 4), 'composed_groups_ms': [round(v, 5) for v in med['composed']],
            'fused_groups_ms': [round(v, 5) for v in med['fused']], 'dice_equal': bool(torch.equal(d0, d1)), 'rgb_equal': bool(torch.equal(r0, r1))}


def load_parent(path):
    """a binding of an older build: only the symbols it exports are bound (the parent has none of the one-hot calls)"""
    import ctypes
    have, sigs = ctypes.CDLL(path), segx._SIGS
    segx._SIGS = {k: v for k, v in sigs.items() if hasattr(have, k)}
    try:
        return segx.SegxLib(path)
    finally:
        segx._SIGS = sigs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="libsegx.so built from the parent commit's sources")
    ap.add_argument('--groups', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'oct_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'oct_bench times the device: it needs the GPU'
    dev = torch.device('cuda', 0)
    libs = {'this': segx.lib()}
    if a.parent_lib:
        libs['parent'] = load_parent(a.parent_lib)
    res = {'tool': 'oct_bench', 'device': torch.cuda.get_device_name(0), 'groups': a.groups, 'reps': a.reps, 'inner': a.inner,
           'regression_c3': dict(image=list(IMAGE), window=list(WINDOW), stride=STRIDE, batch=BATCH, parent_lib=bool(a.parent_lib), **regression(libs, a, dev)),
           'fused_tail_c10': fused_tail(a, dev)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
