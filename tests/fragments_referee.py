"""The torch referee of tests/test_fragments.py and tests/test_gpu_fragments.py, written independently of the kernels and of the fixture: labels start as
1 + raster index on set pixels and take the minimum over the set 3 x 3 neighbourhood until nothing changes; sizes by counting labels; the two labels to keep by
sorting (count descending, label ascending).  It works on whatever device its input is on.  Not a test module."""
import torch


def ref_labels(fg, check_every=1):
    """fg bool [P, H, W] -> (labels, sizes) int32 as segx_ccl2d defines them"""
    P, H, W = fg.shape
    big = H * W + 1
    idx = torch.arange(1, H * W + 1, dtype=torch.int64, device=fg.device).view(1, H, W).expand(P, H, W)
    lab = torch.where(fg, idx, torch.full_like(idx, big))
    it = 0
    while True:
        pad = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=big)
        m = lab
        for dy in range(3):
            for dx in range(3):
                m = torch.minimum(m, pad[:, dy:dy + H, dx:dx + W])
        new = torch.where(fg, m, lab)
        it += 1
        if it % check_every == 0 and torch.equal(new, lab):
            break
        lab = new
    labels = torch.where(fg, lab, torch.zeros_like(lab))
    sizes = torch.zeros(P, H * W + 1, dtype=torch.int64, device=fg.device)
    sizes.scatter_add_(1, labels.view(P, -1), torch.ones(P, H * W, dtype=torch.int64, device=fg.device))
    return labels.to(torch.int32), sizes[:, 1:].reshape(P, H, W).to(torch.int32)


def ref_keep(sizes):
    """int [P, 2]: the documented rule -- background (when it has a pixel) and components by count descending, label ascending; -1 where fewer than two"""
    P = sizes.shape[0]
    flat = sizes.reshape(P, -1).long().cpu()
    keep = []
    for p in range(P):
        nz = flat[p].nonzero().view(-1)
        cand = [(int(flat[p, i]), int(i) + 1) for i in nz]
        bgc = flat.shape[1] - int(flat[p].sum())
        if bgc > 0:
            cand.append((bgc, 0))
        cand.sort(key=lambda cl: (-cl[0], cl[1]))
        keep.append([c[1] for c in cand[:2]] + [-1] * (2 - min(2, len(cand))))
    return torch.tensor(keep, dtype=torch.int32, device='cpu')


def ref_remove(seg, bg, check_every=1):
    """seg uint8 [P, H, W] -> the cleaned planes, by the referee alone"""
    labels, sizes = ref_labels(seg != bg, check_every)
    keep = ref_keep(sizes).to(seg.device)
    stay = (labels == 0) | (labels == keep[:, 0].view(-1, 1, 1)) | (labels == keep[:, 1].view(-1, 1, 1))
    return torch.where(stay, seg, torch.full_like(seg, bg))
