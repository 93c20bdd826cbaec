"""Writes tests/golden/surface3d.npz: binary masks and what medpy 0.4's metric.binary surface distances make of them, restated with scipy.ndimage (unit voxel
spacing, connectivity 1).  Needs scipy; the tests read the file and never import scipy.

    border(m)        = m XOR binary_erosion(m, generate_binary_structure(m.ndim, 1))          (border_value 0: outside the array is unset)
    dt(ref)          = distance_transform_edt(~border(ref))                                    (every voxel, not only the outside ones)
    asd(res, ref)    = dt(ref)[border(res)].mean()                                             (one direction)
    hd95(res, ref)   = numpy.percentile(hstack(dt(ref)[border(res)], dt(res)[border(ref)]), 95)

Per case <c> the file holds <c>_pred / <c>_gt (uint8 [P, *shape]), <c>_bpred / <c>_bgt (their borders), <c>_d2gt / <c>_d2pred (int32 squared distance to the border
of gt / pred; INF throughout a plane whose mask is empty), <c>_asd / <c>_hd95 / <c>_valid (float64 [P]; 0 where either mask is empty).  The medium case keeps only
masks and metrics.  `percase_*`: class maps [4, 9, 20, 33] and the [dice, jc, hd, asd] table / validity of the reference's calculate_metric_percase, with and without
its commented-out hd95.

    python tests/golden/make_surface_golden.py
"""
import os
import numpy as np
from scipy import ndimage

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
INF = 0x40000000                      # SEGX_EDT_INF of include/segx.h


def border(m):
    m = m.astype(bool)
    return m ^ ndimage.binary_erosion(m, structure=ndimage.generate_binary_structure(m.ndim, 1), iterations=1)


def dt(b):
    return ndimage.distance_transform_edt(~b)


def d2_of(b):
    if not b.any():
        return np.full(b.shape, INF, np.int32)
    d = dt(b) ** 2
    r = np.rint(d)
    assert np.abs(d - r).max() < 1e-6
    return r.astype(np.int32)


def asd(res, ref):
    return dt(border(ref))[border(res)].mean()


def hd95(res, ref):
    br, bf = border(res), border(ref)
    return np.percentile(np.hstack((dt(bf)[br], dt(br)[bf])), 95)


def balls(rng, shape, n, rmax):
    """union of n balls with random centres (some outside the faces, so blobs touch faces, edges and corners) and radii"""
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'))
    m = np.zeros(shape, bool)
    for _ in range(n):
        c = np.array([rng.uniform(-1, s) for s in shape]).reshape((-1,) + (1,) * len(shape))
        m |= ((grid - c) ** 2).sum(0) <= rng.uniform(1.0, rmax) ** 2
    return m


def planes(rng, shape):
    """(pred, gt) [7, *shape]: blobs + speckle; fully set vs blobs; empty vs blobs; one corner voxel vs the opposite corner; identical; blobs vs empty; both empty"""
    rmax = max(2.0, min(max(shape) / 3.0, 9.0))
    a, b = balls(rng, shape, 4, rmax), balls(rng, shape, 4, rmax)
    a |= rng.random(shape) < 0.03
    b[tuple(0 for _ in shape)] = True                    # a corner, an edge and a face voxel
    b[(0,) + tuple(s // 2 for s in shape[1:])] = True
    a[tuple(s - 1 for s in shape[:-1]) + (shape[-1] // 2,)] = True
    full, empty = np.ones(shape, bool), np.zeros(shape, bool)
    c0, c1 = empty.copy(), empty.copy()
    c0[tuple(0 for _ in shape)] = True
    c1[tuple(s - 1 for s in shape)] = True
    same = balls(rng, shape, 3, rmax)
    if not same.any():
        same[tuple(s // 2 for s in shape)] = True
    pred = np.stack([a, full, empty, c0, same, balls(rng, shape, 2, rmax) | c0, empty])
    gt = np.stack([b, balls(rng, shape, 3, rmax) | c1, b, c1, same, empty, empty])
    return pred, gt


def metrics(pred, gt, want_hd=True):
    P = pred.shape[0]
    a, h, v = np.zeros(P), np.zeros(P), np.zeros(P)
    for p in range(P):
        if pred[p].any() and gt[p].any():
            v[p] = 1
            a[p] = asd(pred[p], gt[p])
            if want_hd:
                h[p] = hd95(pred[p], gt[p])
    return a, h, v


def case(out, name, pred, gt, fields=True):
    out[name + '_pred'], out[name + '_gt'] = pred.astype(np.uint8), gt.astype(np.uint8)
    if fields:
        bp, bg = np.stack([border(m) for m in pred]), np.stack([border(m) for m in gt])
        out[name + '_bpred'], out[name + '_bgt'] = bp.astype(np.uint8), bg.astype(np.uint8)
        out[name + '_d2gt'], out[name + '_d2pred'] = np.stack([d2_of(b) for b in bg]), np.stack([d2_of(b) for b in bp])
    if pred.ndim == 4:
        out[name + '_asd'], out[name + '_hd95'], out[name + '_valid'] = metrics(pred, gt)


def main():
    rng = np.random.RandomState(20240607)
    out = {}
    for name, shape in (('s5x6x7', (5, 6, 7)), ('s9x20x33', (9, 20, 33)), ('s1x17x40', (1, 17, 40)), ('s3x5x130', (3, 5, 130)), ('s70x3x5', (70, 3, 5)),
                        ('s17x40', (17, 40))):
        case(out, name, *planes(rng, shape))
    # one-directional asd: `one` is a blob, `two` the same blob and a far one -- asd(one, two) = 0, asd(two, one) is large
    shape = (9, 20, 33)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'))
    one = ((grid - np.array([4, 6, 7]).reshape(3, 1, 1, 1)) ** 2).sum(0) <= 9
    two = one | (((grid - np.array([4, 14, 27]).reshape(3, 1, 1, 1)) ** 2).sum(0) <= 9)
    case(out, 'twoblob', np.stack([one, two]), np.stack([two, one]))
    # medium: several slabs and workgroups on the device; masks and metrics only
    shape = (40, 48, 72)
    pred = np.stack([balls(rng, shape, 6, 11.0) for _ in range(3)])
    gt = np.stack([balls(rng, shape, 6, 11.0) for _ in range(3)])
    gt[1] = pred[1] ^ (balls(rng, shape, 3, 5.0))                      # nearly agreeing surfaces
    case(out, 'medium', pred, gt, fields=False)
    # calculate_metric_percase (reference test_util3d.py:186-215): n-hot class maps [4, 9, 20, 33]; class 3 is empty in the prediction
    shape = (9, 20, 33)
    cp = np.stack([balls(rng, shape, 3, 6.0) for _ in range(4)])
    cg = np.stack([balls(rng, shape, 3, 6.0) for _ in range(4)])
    cg[1], cg[2] = np.roll(cp[1], 2, axis=2), np.roll(cp[2], 1, axis=1) | balls(rng, shape, 1, 4.0)          # overlapping classes: Dice and Jaccard away from 0
    cp[3] = False
    cp[0], cg[0] = ~cp[1:].any(0), ~cg[1:].any(0)
    table, valid = np.zeros((3, 4)), np.ones((3, 4))
    for c in range(1, 4):
        p, g = cp[c], cg[c]
        inter = float((p & g).sum())
        dice = 2.0 * inter / float(p.sum() + g.sum()) if p.sum() + g.sum() else 0.0
        if g.sum() > 0:
            jc = inter / float((p | g).sum())
        else:
            jc = 0.0; valid[c - 1, 1] = 0
        if p.sum() > 0 and g.sum() > 0:
            table[c - 1] = [dice, jc, hd95(p, g), asd(p, g)]
        else:
            table[c - 1] = [dice, jc, 0, 0]; valid[c - 1, 2:] = 0
    out['percase_pred'], out['percase_gt'] = cp.astype(np.uint8), cg.astype(np.uint8)
    out['percase_metric_hd95'], out['percase_valid'] = table, valid
    ref = table.copy(); ref[:, 2] = 0                                   # the reference's own return value: hd = 0
    out['percase_metric'] = ref
    np.savez_compressed(os.path.join(OUT_DIR, 'surface3d.npz'), **out)


if __name__ == '__main__':
    main()
