"""The torch referee of tests/test_components3d.py and tests/test_gpu_postprocess3d.py, written independently of the kernels: labels start as 1 + raster index on set
voxels and take the minimum over the set 3 x 3 x 3 neighbourhood (connectivity 26) or over the 6 face neighbours until nothing changes; sizes by counting labels; the
keep rule by sorting (size descending, first index ascending); the BraTS rule as plain torch.  It works on whatever device its input is on.  Not a test module."""
import torch


def _shifted_min(lab, big, axis):
    """the minimum of lab and its two neighbours along `axis`, `big` beyond the volume's ends"""
    n = lab.shape[axis]
    lo = torch.cat([lab.narrow(axis, 1, n - 1), torch.full_like(lab.narrow(axis, 0, 1), big)], axis)
    hi = torch.cat([torch.full_like(lab.narrow(axis, 0, 1), big), lab.narrow(axis, 0, n - 1)], axis)
    return torch.minimum(lab, torch.minimum(lo, hi))


def ref_labels3d(fg, connectivity=26, check_every=1):
    """fg bool [V, X, Y, Z] -> (labels, sizes) int32 as segx_ccl3d defines them"""
    assert connectivity in (6, 26) and fg.dim() == 4 and fg.dtype == torch.bool
    V, X, Y, Z = fg.shape
    S = X * Y * Z
    big = S + 1
    idx = torch.arange(1, S + 1, dtype=torch.int32, device=fg.device).view(1, X, Y, Z).expand(V, X, Y, Z)
    lab = torch.where(fg, idx, torch.full_like(idx, big))
    it = 0
    while True:
        if connectivity == 26:                       # the minimum over a box is the minimum along z, then y, then x (unset voxels hold `big`)
            m = _shifted_min(_shifted_min(_shifted_min(lab, big, 3), big, 2), big, 1)
        else:
            m = torch.minimum(torch.minimum(_shifted_min(lab, big, 3), _shifted_min(lab, big, 2)), _shifted_min(lab, big, 1))
        new = torch.where(fg, m, lab)
        it += 1
        if it % check_every == 0 and torch.equal(new, lab):
            break
        lab = new
    labels = torch.where(fg, lab, torch.zeros_like(lab))
    sizes = torch.zeros(V, S + 1, dtype=torch.int64, device=fg.device)
    sizes.scatter_add_(1, labels.view(V, -1).long(), torch.ones(V, S, dtype=torch.int64, device=fg.device))
    return labels, sizes[:, 1:].reshape(V, X, Y, Z).to(torch.int32)


def ref_keep3d(labels, sizes, min_voxels=0, largest_only=False):
    """uint8 [V, X, Y, Z]: the documented rule by sorting each volume's components (size descending, first index ascending)"""
    V = labels.shape[0]
    flat = sizes.reshape(V, -1).long().cpu()
    keep = torch.zeros_like(labels, dtype=torch.uint8)
    for v in range(V):
        comps = sorted(((int(flat[v, i]), int(i)) for i in flat[v].nonzero().view(-1)), key=lambda c: (-c[0], c[1]))
        if largest_only:
            comps = comps[:1]
        stay = torch.tensor([i + 1 for size, i in comps if size >= min_voxels], dtype=labels.dtype, device=labels.device)
        keep[v] = torch.isin(labels[v], stay).to(torch.uint8)
    return keep


def ref_remove3d(mask, min_voxels=0, largest_only=False, connectivity=26, check_every=1):
    """mask [V, X, Y, Z] of any dtype -> the cleaned stack, by the referee alone"""
    labels, sizes = ref_labels3d(mask != 0, connectivity, check_every)
    return torch.where(ref_keep3d(labels, sizes, min_voxels, largest_only).bool(), mask, torch.zeros_like(mask))


def ref_brats(hard, labels=None, wt_min_voxels=0, wt_largest_only=False, et_min_voxels=0, connectivity=26, check_every=1):
    """The BraTS rule on hard float [4, X, Y, Z] = (background, ET, WT, TC) in plain torch.  Returns (hard', labels' or None, dropped)"""
    wt = ref_remove3d(hard[2:3], wt_min_voxels, wt_largest_only, connectivity, check_every)[0]
    et, tc = hard[1] * wt, hard[3] * wt
    dropped = int((et != 0).sum()) < et_min_voxels
    if dropped:
        et = torch.zeros_like(et)
    bg = ((et + wt + tc) == 0).to(hard.dtype)
    out = torch.stack([bg, et, wt, tc])
    if labels is None:
        return out, None, dropped
    new = torch.where(wt == 0, torch.zeros_like(labels), labels)
    if dropped:
        new = torch.where(new == 4, torch.ones_like(new), new)
    return out, new, dropped
