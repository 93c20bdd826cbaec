"""Writes tests/golden/fragments2d.npz: inputs and what the REAL reference functions make of them -- remove_fragmentary_segs and calc_batch_metric (test_util2d.py),
calc_vcdr (utils/losses.py), fundus_inv_map_mask / polyp_inv_map_mask (dataloaders/datasets2d.py) -- run through make_golden._ref_functions.  Needs the reference
checkout and scipy; the tests read the file and import neither.

cv2 is not installed where this runs, so the one cv2 call of remove_fragmentary_segs, cv2.connectedComponents(img) -> (count, labels) with its default connectivity 8,
is served by scipy.ndimage.label with the full 3 x 3 structure.  Only inputs and outputs are stored (small uint8 / float arrays).

Every fragment case is asserted to lie inside the reference's domain: a background pixel exists, a foreground component exists, and the second and third largest
label counts differ (numpy.argpartition's order among equal counts is unspecified).

    frag_<case>_in / _out   uint8 [H, W] label image and the reference's result;  frag_<case>_bg   its bg_value
    vcdr_<case>_in          float32 n-hot maps [3, H, W] / [B, 3, H, W];  vcdr_<case>_d0 / _d1   calc_vcdr with delta 0 / 1 (the batch form ignores delta)
    metric_pred<i> / metric_gt<i>   soft predictions / n-hot masks per instance;  metric_table   calc_batch_metric(..., 3, do_calc_vcdr_error=True)
    inv_fundus_in / _out, inv_fundus3_in / _out, inv_polyp_in / _out   n-hot maps and their pixel-value images

    python tests/golden/make_fragments_golden.py
"""
import os
import types

import numpy as np
import torch
from scipy import ndimage

import make_golden as G             # puts the repository root on sys.path
from segtran_amd import segx

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
TH, TW = segx.SegxLib.CCL_TILE       # SEGX_CCL_TILE_H / _W of include/segx.h (tests/test_fragments.py holds the two equal): the cases straddle tile seams


def connected_components(img):
    labels, count = ndimage.label(img, structure=np.ones((3, 3), int))
    return count + 1, labels.astype(np.int32)


def in_domain(seg, bg):
    labels, count = ndimage.label(seg != bg, structure=np.ones((3, 3), int))
    counts = np.sort(np.bincount(labels.ravel()))[::-1]
    assert (seg == bg).any(), 'no background pixel'
    assert count >= 1, 'no foreground component'
    assert len(counts) < 3 or counts[1] != counts[2], 'tie at the cut: %s' % counts[:4]


def disc(shape, cy, cx, r):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def fragment_cases(rng):
    cases = {}
    # fundus: disc with the cup inside over a tile corner, distant specks of both values
    shape = (2 * TH + 7, 2 * TW + 9)
    seg = np.full(shape, 255, np.uint8)
    seg[disc(shape, TH + 2, TW - 3, 22)] = 128
    seg[disc(shape, TH + 4, TW - 1, 9)] = 0
    for (y, x, v) in ((2, 3, 128), (3, 4, 0), (shape[0] - 2, shape[1] - 3, 128), (5, shape[1] - 1, 0), (shape[0] - 1, 0, 128), (TH - 1, 2 * TW, 128), (TH, 2 * TW + 1, 128)):
        seg[y, x] = v
    cases['fundus'] = (seg, 255)
    # polyp: background 0, two blobs and speckle
    shape = (TH + 9, TW + 30)
    seg = np.zeros(shape, np.uint8)
    seg[disc(shape, 14, 20, 9)] = 255
    seg[disc(shape, TH + 1, TW + 8, 6)] = 255
    seg[(rng.random_sample(shape) < 0.02) & ~disc(shape, 14, 20, 11) & ~disc(shape, TH + 1, TW + 8, 8)] = 255
    cases['polyp'] = (seg, 0)
    # two foreground components that both exceed the background; a third, small one goes
    shape = (TH + 4, TW + 6)
    seg = np.full(shape, 7, np.uint8)
    seg[:, :30] = 1
    seg[:, 33:] = 2
    seg[:3, 31] = 3
    cases['twofg'] = (seg, 7)
    # small: one plane inside one tile, three components of different sizes
    seg = np.zeros((9, 11), np.uint8)
    seg[1:4, 1:5] = 9; seg[6:8, 6:9] = 9; seg[0, 10] = 9
    cases['small'] = (seg, 0)
    return cases


def vcdr_cases(rng):
    def soft(hard):
        return np.where(hard, rng.uniform(0.5, 1.0, hard.shape), rng.uniform(0.0, 0.499, hard.shape)).astype(np.float32)
    H, W = 20, 70
    dm, cm = np.zeros((H, W), bool), np.zeros((H, W), bool)
    dm[3:15, 5:60] = True; cm[6:11, 66:69] = True                                    # disc rows 3..14, cup rows 6..10 (the cup in the last lanes of the second sweep)
    normal = np.stack([~dm, dm, cm])
    nodisc = np.stack([~cm, np.zeros_like(dm), cm])
    nocup = np.stack([~dm, dm, np.zeros_like(cm)])
    full = np.stack([np.zeros_like(dm), np.ones_like(dm), cm])                       # every row occupied by the disc: the batch form's minimum is 1, not 0
    gap = dm.copy(); gap[8] = False
    gapped = np.stack([~gap, gap, cm])
    onerow = np.zeros((H, W), bool); onerow[H - 1, 0] = True
    last = np.stack([~onerow, onerow, onerow])                                      # a single pixel in the last row: lengths of -delta
    out = {'normal': soft(normal), 'nodisc': soft(nodisc), 'nocup': soft(nocup), 'lastrow': soft(last), 'hard': normal.astype(np.float32),
           'batch': np.stack([soft(normal), soft(full), soft(gapped), soft(nodisc), soft(nocup)])}
    return out


def main():
    rng = np.random.RandomState(20240911)
    t2 = G._ref_functions('test_util2d.py', ['remove_fragmentary_segs'], dict(cv2=types.SimpleNamespace(connectedComponents=connected_components), pdb=None))
    out = {}
    for name, (seg, bg) in fragment_cases(rng).items():
        in_domain(seg, bg)
        res = t2['remove_fragmentary_segs'](torch.from_numpy(seg.copy()), bg)        # the reference writes into the host copy it is given
        out['frag_%s_in' % name], out['frag_%s_bg' % name], out['frag_%s_out' % name] = seg, np.array(bg), res.numpy().astype(np.uint8)
        assert (out['frag_%s_out' % name] != seg).any(), name + ': nothing was removed'
    lo = G._ref_functions('utils/losses.py', ['calc_vcdr'])
    for name, m in vcdr_cases(rng).items():
        out['vcdr_%s_in' % name] = m
        for delta in (0, 1):
            out['vcdr_%s_d%d' % (name, delta)] = lo['calc_vcdr'](torch.from_numpy(m), delta=delta).numpy()
    assert abs(float(out['vcdr_hard_d1']) - 0.3) < 1e-4 and out['vcdr_hard_d1'].dtype == np.float32 and out['vcdr_nodisc_d1'] == -1 and out['vcdr_nocup_d0'] == 0
    d2 = G._ref_functions('dataloaders/datasets2d.py', ['harden_segmap2d', 'fundus_inv_map_mask', 'polyp_inv_map_mask'])
    t2 = G._ref_functions('test_util2d.py', ['calc_batch_metric', 'calc_dice'], dict(harden_segmap2d=d2['harden_segmap2d'], calc_vcdr=lo['calc_vcdr']))
    preds, gts = [], []
    for i, shape in enumerate(((24, 28), (33, 20))):
        g = np.zeros((3,) + shape, bool)
        g[1] = disc(shape, shape[0] // 2, shape[1] // 2, 8); g[2] = disc(shape, shape[0] // 2 + 1, shape[1] // 2, 3 + i); g[0] = ~g[1]
        p = np.zeros((3,) + shape, bool)
        p[1] = disc(shape, shape[0] // 2 + 1, shape[1] // 2 - 1, 7 + i); p[2] = disc(shape, shape[0] // 2, shape[1] // 2, 4 - i); p[0] = ~p[1]
        ps = np.where(p, rng.uniform(0.5, 1.0, p.shape), rng.uniform(0.0, 0.499, p.shape)).astype(np.float32)
        preds.append(torch.from_numpy(ps)); gts.append(torch.from_numpy(g.astype(np.float32)))
        out['metric_pred%d' % i], out['metric_gt%d' % i] = ps, g.astype(np.float32)
    out['metric_table'] = t2['calc_batch_metric'](preds, gts, 3, do_calc_vcdr_error=True)
    assert out['metric_table'].shape == (2, 3) and (out['metric_table'][:, 2] > 0).all()
    nh = (rng.random_sample((2, 3, 10, 12)) < 0.4).astype(np.float32)
    nh[0, :, 0, 0] = (1, 1, 0); nh[0, :, 0, 1] = (1, 0, 1); nh[0, :, 0, 2] = (0, 0, 0); nh[0, :, 0, 3] = (1, 1, 1)      # two classes on: the later wins; none: 0
    out['inv_fundus_in'], out['inv_fundus_out'] = nh, d2['fundus_inv_map_mask'](torch.from_numpy(nh)).numpy()
    out['inv_fundus3_in'], out['inv_fundus3_out'] = nh[1], d2['fundus_inv_map_mask'](torch.from_numpy(nh[1])).numpy()
    out['inv_polyp_in'], out['inv_polyp_out'] = nh[:, :2], d2['polyp_inv_map_mask'](torch.from_numpy(nh[:, :2].copy())).numpy()
    assert out['inv_fundus_out'].dtype == np.uint8 and tuple(out['inv_fundus_out'][0, 0, :4]) == (128, 0, 0, 0)
    np.savez_compressed(os.path.join(OUT_DIR, 'fragments2d.npz'), **out)
    print('wrote fragments2d.npz (%.0f KB, %d arrays)' % (os.path.getsize(os.path.join(OUT_DIR, 'fragments2d.npz')) / 1024, len(out)))


if __name__ == '__main__':
    main()
