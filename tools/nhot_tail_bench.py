"""The evaluation tail of the n-hot 2-D tasks (fundus, polyp) as one launch, timed on the device against the composed path.

  python tools/nhot_tail_bench.py [--groups 5] [--reps 10] [--out profiles/nhot_tail_bench.json]

(a) A batch of 6 with 3 classes, soft 576 x 576, at two mask sizes: 576 x 576 (no resampling) and 1024 x 1024 (the bilinear gather is in the measurement).  Three forms,
    taking turns inside every repetition:
      composed  infer2d.calc_batch_metric(do_calc_vcdr_error=True) + infer2d.export_masks(fundus_inv_map_mask): per image resample, harden, Dice, two calc_vcdr, two
                reads, and the resample / harden / inverse map again for the label image -- the path this tool's commit leaves untouched;
      fused     the same two calls with fused=True: one tail launch and one read for the table, one tail launch for the label images;
      tail      ONE SF.nhot_case_tail launch into preallocated tensors that forms counts, extents and label images together (what GraphedBatchEvaluation captures).
    A timing is one call between two HIP events (the composed and the fused form read the device, so the events also bracket the host's part); a group is the median
    of `reps` timings; the figure is the median of `groups` groups.  The forms' results are compared for equality.
(b) cfg1 model, 256 x 256 image (one window), batch 2, masks 256 x 256: one GraphedBatchEvaluation replay (forward and tail in one graph; no read) against one
    GraphedSlidingWindow replay followed by the composed tail, and against the replay followed by the fused calls.
`not_slower` states for every comparison whether the fused form's median is at or below the composed one's.  Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, functional as SF, infer2d     # noqa: E402
from segtran_amd.dataloaders.datasets2d import fundus_inv_map_mask, fundus_map_mask      # noqa: E402
from oct_bench import group_medians                            # noqa: E402

BATCH, CLASSES, SOFT, MASKS, VALUES = 6, 3, (576, 576), ((576, 576), (1024, 1024)), (255, 128, 0)


def synth_mask(B, H, W, seed):
    """raw fundus masks uint8 [B, 3, H, W]: a disc and a cup ellipse per image, centred off the middle"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    m = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    for b in range(B):
        cy, cx = (0.35 + 0.3 * torch.rand(2, generator=g)) * torch.tensor([H, W])
        r = (0.15 + 0.1 * float(torch.rand(1, generator=g))) * min(H, W)
        d2 = ((yy - cy) / 1.2) ** 2 + (xx - cx) ** 2
        m[b, 0] = (d2 <= r * r).to(torch.uint8) * 255
        m[b, 1] = (d2 <= (0.5 * r) ** 2).to(torch.uint8) * 255
    m[:, 2] = m[:, 0]
    return m


def summarize(med, base):
    m = {k: statistics.median(v) for k, v in med.items()}
    out = {k + '_ms': round(v, 5) for k, v in m.items()}
    out.update({k + '_groups_ms': [round(x, 5) for x in v] for k, v in med.items()})
    out.update({k + '_over_' + base: round(m[k] / m[base], 4) for k in m if k != base})
    out['not_slower'] = {k: bool(m[k] <= m[base]) for k in m if k != base}
    return out


def tail_forms(a, dev, size):
    B, C, (H, W) = BATCH, CLASSES, size
    g = torch.Generator(device='cpu').manual_seed(5)
    soft = torch.rand(B, C, *SOFT, generator=g).pow(2).to(dev)
    gt = fundus_map_mask(synth_mask(B, H, W, 6).to(dev))
    sizes = [size] * B
    counts, ext = torch.empty(B, C - 1, 3, dtype=torch.int32, device=dev), torch.empty(B, 2, 2, 2, dtype=torch.int32, device=dev)
    labels = torch.empty(B, H, W, dtype=torch.uint8, device=dev)

    def composed():
        return infer2d.calc_batch_metric(soft, gt, C, do_calc_vcdr_error=True), infer2d.export_masks(soft, sizes, fundus_inv_map_mask)

    def fused():
        return infer2d.calc_batch_metric(soft, gt, C, do_calc_vcdr_error=True, fused=True), infer2d.export_masks(soft, sizes, fundus_inv_map_mask, fused=True)

    def tail():
        return SF.nhot_case_tail(soft, gt, values=VALUES, counts=counts, ext=ext, labels=labels)

    med = group_medians({'composed': composed, 'fused': fused, 'tail': tail}, a.groups, a.reps, 1)
    (t0, m0), (t1, m1) = composed(), fused()
    tail()
    res = {'soft': list(SOFT), 'masks': [H, W], 'batch': B, 'classes': C, 'resampled': size != SOFT}
    res.update(summarize(med, 'composed'))
    res.update(table_equal=bool((t0 == t1).all()), labels_equal=bool(all(torch.equal(x, y) for x, y in zip(m0, m1)) and torch.equal(labels, torch.stack(m0))))
    return res


def graphed(a, dev):
    c = engine.CONFIGS['cfg1']
    S, B, C = c['size'][0], c['bs'], c['num_classes']
    net = engine.build_model('cfg1', dev, dropout_prob=0.0).eval()
    img, _ = engine.synth_batch(c, B, dev)
    gt = fundus_map_mask(synth_mask(B, S, S, 7).to(dev))
    geo = dict(orig_input_size=(S, S), patch_size=(S, S), stride=(S // 2, S // 2))
    plain = infer2d.GraphedSlidingWindow(net, img.shape, num_classes=C, **geo)
    both = infer2d.GraphedBatchEvaluation(net, img.shape, num_classes=C, mask_size=(S, S), values=VALUES, with_extents=True, **geo)
    sizes = [(S, S)] * B

    def composed():
        _, soft = plain(img)
        return infer2d.calc_batch_metric(soft, gt, C, do_calc_vcdr_error=True), infer2d.export_masks(soft, sizes, fundus_inv_map_mask)

    def fused():
        _, soft = plain(img)
        return infer2d.calc_batch_metric(soft, gt, C, do_calc_vcdr_error=True, fused=True), infer2d.export_masks(soft, sizes, fundus_inv_map_mask, fused=True)

    def graph():
        return both(img, gt)

    try:
        med = group_medians({'replay_composed': composed, 'replay_fused': fused, 'one_graph': graph, 'replay_alone': lambda: plain(img)}, a.groups, a.reps, 1)
        (t0, m0), (_, _, counts, ext, labels) = composed(), graph()
        cf = counts.float()
        dice = ((2 * cf[..., 0] + 1e-5) / (cf[..., 1] + cf[..., 2] + 1e-5)).cpu().numpy()
        vp, vg = infer2d.vcdr_from_extents(ext)
        res = {'model': 'cfg1', 'image': [S, S], 'batch': B, 'windows': both.plan.table.nwin}
        res.update(summarize(med, 'replay_composed'))
        res.update(table_equal=bool((dice == t0[:, :C - 1]).all() and ((vg - vp).abs().cpu().numpy() == t0[:, C - 1]).all()),
                   labels_equal=bool(torch.equal(labels, torch.stack(m0))))
        return res
    finally:
        both.close()
        plain.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'nhot_tail_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'nhot_tail_bench times the device: it needs the GPU'
    dev = torch.device('cuda', 0)
    res = {'tool': 'nhot_tail_bench', 'device': torch.cuda.get_device_name(0), 'groups': a.groups, 'reps': a.reps,
           'tail': {'%dx%d' % size: tail_forms(a, dev, size) for size in MASKS}, 'graphed_256_bs2': graphed(a, dev)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
