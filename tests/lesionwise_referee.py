"""The torch referee of tests/test_lesionwise.py and tests/test_gpu_lesionwise.py, written independently of the kernels from the definition in DESIGN.md 5zb: dilation by
shifted ORs, labelling through components3d_referee.ref_labels3d, matching by torch.unique over the stacked (component label, lesion label) pairs of the voxels that
carry both, counts by torch.bincount.  It works on whatever device its input is on.  Not a test module."""
import numpy as np
import torch

from components3d_referee import ref_labels3d


def _shift(m, off):
    """m [V, X, Y, Z] moved by off = (dx, dy, dz): out[p + off] = m[p], unset where nothing arrives"""
    out = torch.zeros_like(m)
    src, dst = [slice(None)], [slice(None)]
    for d, n in zip(off, m.shape[1:]):
        src.append(slice(max(0, -d), n - max(0, d)))
        dst.append(slice(max(0, d), n - max(0, -d)))
    out[tuple(dst)] = m[tuple(src)]
    return out


def ref_dilate(mask, iters, connectivity):
    """bool [V, X, Y, Z] dilated iters times by the centre and its 6 / 18 / 26 nearest neighbours; outside the volume is unset"""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= reach]
    assert len(offs) == connectivity and mask.dtype == torch.bool
    for _ in range(iters):
        grown = mask.clone()
        for off in offs:
            grown |= _shift(mask, off)
        mask = grown
    return mask


def ref_summary(lesions, n_fp, min_lesion_voxels=0):
    """the summary of the definition from the sorted integer rows: (kept, n_detected, n_missed, lesion_dice)"""
    kept = lesions[:, 2] >= min_lesion_voxels
    total = 0.0
    for _, tp, gvol, pvol in lesions[kept].tolist():
        total += 2.0 * tp / (gvol + pvol)
    n = int(kept.sum())
    detected = int((lesions[kept][:, 1] > 0).sum())
    return kept, detected, n - detected, (total / (n + n_fp) if n + n_fp > 0 else 1.0)


def ref_lesionwise(pred, gt, dilation_iters=3, dilation_connectivity=18, connectivity=26, min_lesion_voxels=0, check_every=1):
    """pred, gt [V, X, Y, Z] of any dtype (set = not 0) -> a list of V dicts with the keys of infer3d.lesionwise_from_tables plus 'n_pred'"""
    pred, gt = pred != 0, gt != 0
    V, S = pred.shape[0], pred[0].numel()
    gd = ref_dilate(gt, dilation_iters, dilation_connectivity)
    GL, _ = ref_labels3d(gd, connectivity, check_every)
    PL, psizes = ref_labels3d(pred, connectivity, check_every)
    out = []
    for v in range(V):
        g, p, isgt = GL[v].reshape(-1).long(), PL[v].reshape(-1).long(), gt[v].reshape(-1)
        size_of = torch.cat([torch.zeros(1, dtype=torch.int64, device=g.device), psizes[v].reshape(-1).long()])      # by component label
        gvol = torch.bincount(g[isgt], minlength=S + 1)
        tp = torch.bincount(g[isgt & (p > 0)], minlength=S + 1)
        both = (g > 0) & (p > 0)
        pairs = torch.unique(torch.stack([p[both], g[both]], 1), dim=0)                 # distinct (component, lesion) pairs that share a voxel
        pvol = torch.zeros(S + 1, dtype=torch.int64, device=g.device)
        pvol.scatter_add_(0, pairs[:, 1], size_of[pairs[:, 0]])
        roots = torch.unique(g[g > 0])                                                  # ascending
        lesions = torch.stack([roots, tp[roots], gvol[roots], pvol[roots]], 1).cpu().numpy().astype(np.int64).reshape(-1, 4)
        comps = torch.unique(p[p > 0])
        untouched = comps[~torch.isin(comps, pairs[:, 0])]
        n_fp, fp_voxels = int(untouched.numel()), int(size_of[untouched].sum())
        kept, detected, missed, dice = ref_summary(lesions, n_fp, min_lesion_voxels)
        out.append(dict(lesions=lesions, kept=kept, n_fp=n_fp, fp_voxels=fp_voxels, n_detected=detected, n_missed=missed, lesion_dice=dice,
                        n_pred=int(comps.numel())))
    return out
