"""On-device label maps of the 2D train step and of the evaluation's export (mirror of reference code/dataloaders/datasets2d.py:22-171, 200-250).
Only the in-step label -> n-hot maps and the n-hot -> pixel-value maps are built; file I/O and imgaug pipelines are out of scope."""
import torch


def index_to_onehot(mask, num_classes):
    """reference datasets2d.py:22-51 for tensors: an integer index mask [B, 1, H, W], [B, H, W] or [H, W] -> float32 one-hot maps with the class dimension first
    ([C, H, W]) or after the batch ([B, C, H, W]).  On the device this is segx_index_onehot; for CPU tensors the torch expression below states it.  A label outside
    0 .. num_classes - 1 sets no class (the reference's scatter_ raises there)."""
    if mask.dim() == 4 and mask.shape[1] == 1:
        lab = mask[:, 0]
    elif mask.dim() in (2, 3):
        lab = mask if mask.dim() == 3 else mask.unsqueeze(0)
    else:
        raise ValueError('index_to_onehot: an index mask [B, 1, H, W], [B, H, W] or [H, W], not %s' % (tuple(mask.shape),))
    if lab.is_cuda:
        from .. import functional as SF
        out = SF.index_onehot(lab, num_classes)
    else:
        classes = torch.arange(num_classes, device=lab.device).view(1, num_classes, 1, 1)
        out = (lab.long().unsqueeze(1) == classes).float()
    return out[0] if mask.dim() == 2 else out


def onehot_inv_map(mask_onehot, colormap=None):
    """reference datasets2d.py:54-88: n-hot maps [B, C, H, W] or [C, H, W] -> [..., H, W, 3]: the arg-max over the classes (the lowest index wins a tie) looked up
    in colormap ([C, 3] colours 0 .. 255: uint8 result) or, without one, repeated three times (int64 result, as the reference returns).  segx_onehot_colormap."""
    from .. import functional as SF
    if mask_onehot.dim() not in (3, 4):
        raise ValueError('onehot_inv_map: n-hot maps [C, H, W] or [B, C, H, W], not %s' % (tuple(mask_onehot.shape),))
    batched = mask_onehot.dim() == 4
    out = SF.onehot_colormap(mask_onehot if batched else mask_onehot.unsqueeze(0), colormap)
    if colormap is None:
        out = out.long()
    return out if batched else out[0]


def fundus_map_mask(mask, exclusive=False):
    """uint8 {0,255} [B,3,H,W] (ch0 = disc region incl. cup, ch1 = cup) -> float n-hot [B,3,H,W] (bg, disc, cup)."""
    assert mask.dim() == 4 and mask.shape[1] >= 2, 'batched [B,3,H,W] masks only'
    out = torch.zeros((mask.shape[0], 3) + tuple(mask.shape[2:]), device=mask.device)
    out[:, 0] = (mask[:, 0] == 0)
    out[:, 1] = (mask[:, 0] >= 1) if not exclusive else ((mask[:, 0] >= 1) & (mask[:, 1] == 0))
    out[:, 2] = (mask[:, 1] >= 1)
    return out


def polyp_map_mask(mask, exclusive=True):
    """single 0/255 channel tiled x3 -> float [B,2,H,W] (bg, polyp)."""
    assert mask.dim() == 4
    out = torch.zeros((mask.shape[0], 2) + tuple(mask.shape[2:]), device=mask.device)
    out[:, 0] = (mask[:, 0] == 0)
    out[:, 1] = (mask[:, 0] > 0)
    return out


def harden_segmap2d(mask_soft, T=0.5):
    """reference datasets2d.py:178-196: per-class threshold; background = none of the others.  (batch, channel, h, w) or
    (channel, h, w) -> int32 0/1 maps (segx_harden_segmap)."""
    from .. import functional as SF
    batched = mask_soft.dim() == 4
    x = mask_soft if batched else mask_soft.unsqueeze(0)
    _, hard = SF.harden_segmap(x.float().contiguous(), None, mode=0, T=T, want_soft=False)
    hard = hard.to(torch.int32)
    return hard if batched else hard[0]


def _inv_map(what, mask_nhot, values):
    from .. import functional as SF
    if mask_nhot.dim() not in (3, 4) or mask_nhot.shape[-3] < len(values):
        raise ValueError('%s: n-hot maps [C, H, W] or [B, C, H, W] with C >= %d, not %s' % (what, len(values), tuple(mask_nhot.shape)))
    batched = mask_nhot.dim() == 4
    x = mask_nhot if batched else mask_nhot.unsqueeze(0)
    out = SF.nhot_to_values(x[:, :len(values)], values)
    return out if batched else out[0]


def fundus_inv_map_mask(mask_nhot):
    """reference datasets2d.py:144-171: n-hot (bg, disc, cup) [C, H, W] or [B, C, H, W] -> the REFUGE annotation format, uint8: 255 background, 128 optic disc,
    0 optic cup; assigned in that order, so a pixel with several classes on takes the last one's value, and one with none stays 0 (segx_nhot_to_values)."""
    return _inv_map('fundus_inv_map_mask', mask_nhot, (255, 128, 0))


def polyp_inv_map_mask(mask_nhot):
    """reference datasets2d.py:225-250: n-hot (bg, polyp) [C, H, W] or [B, C, H, W] -> uint8 0 background / 255 polyp (segx_nhot_to_values)."""
    return _inv_map('polyp_inv_map_mask', mask_nhot, (0, 255))
