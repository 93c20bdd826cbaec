"""Fragment removal and the vCDR error column on the device (components.hip) against the host path the reference takes.

  python tools/frag_bench.py [--reps 20] [--warmup 5] [--out profiles/frag_bench.json]

One process, two inputs: one 2048 x 2048 fundus-like label image (background 255, a disc of 128 with a cup of 0 inside, 400 specks) and a batch of six 512 x 512 ones.
Timed with HIP events on the launch stream, medians over `reps` calls after `warmup`:
  remove_fragmentary_segs   infer2d.remove_fragmentary_segs on the stack (labelling, selection, repaint)
  ccl2d / keep2 / apply     its three ABI calls one by one
  vcdr_error                |calc_vcdr(gt) - calc_vcdr(pred)| per image on n-hot maps (two row-extent calls and scalar arithmetic each), left on the device
  host_remove               the reference's route, wall clock around a synchronised call: device -> host copy, labelling (scipy.ndimage.label with the 3 x 3 structure
                            where scipy is importable -- cv2.connectedComponents is not installed -- else a torch minimum-propagation on the CPU), numpy counts and
                            repaint, copy back.  `host_reps` repetitions.
  torch_vcdr_error          the same column by row reductions in torch on the device (any over W, masked index min / max), with the .cpu() per image the reference has
Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from segtran_amd import segx                                   # noqa: E402
from segtran_amd import infer2d                                # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def fundus_like(P, n, dev, specks=400):
    """uint8 [P, n, n]: per plane a disc and a cup whose centres move with the plane, and specks of 1 to 3 pixels away from the disc"""
    y, x = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing='ij')
    out = torch.full((P, n, n), 255, dtype=torch.uint8, device=dev)
    k = torch.arange(specks, device=dev)
    for p in range(P):
        cy, cx, r = n // 2 + 7 * p, n // 2 - 5 * p, int(0.3 * n)
        out[p][(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 128
        out[p][(y - cy) ** 2 + (x - cx - r // 8) ** 2 <= (r * 2 // 5) ** 2] = 0
        sy, sx = (k * 389 + 17 + 31 * p) % n, (k * 683 + 5) % n
        far = (sy - cy) ** 2 + (sx - cx) ** 2 > (r + n // 32) ** 2
        for d in range(3):
            on = far & (k % 3 >= d)
            out[p][sy[on], (sx[on] + d) % n] = 128
    return out


def nhot_of(seg):
    return torch.stack([seg == 255, seg <= 128, seg == 0], dim=1).float()


def cpu_labels(fg):
    """8-connected labels of a numpy bool image without scipy: minimum propagation in torch on the CPU (slow; only where scipy is missing)"""
    H, W = fg.shape
    f = torch.from_numpy(fg)
    big = H * W + 1
    lab = torch.where(f, torch.arange(1, H * W + 1).view(H, W), torch.full((H, W), big))
    while True:
        pad = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=big)
        m = lab
        for dy in range(3):
            for dx in range(3):
                m = torch.minimum(m, pad[dy:dy + H, dx:dx + W])
        new = torch.where(f, m, lab)
        if torch.equal(new, lab):
            return torch.where(f, lab, torch.zeros_like(lab)).numpy()
        lab = new


def host_remove(seg, bg, label):
    out = []
    for plane in seg:
        a = plane.cpu().numpy()
        comp = label(a != bg)
        values, counts = np.unique(comp, return_counts=True)
        top = values[np.argsort(-counts, kind='stable')[:2]]
        a[(comp != top[0]) & (comp != top[-1])] = bg
        out.append(torch.from_numpy(a).to(seg.device))
    return torch.stack(out)


def torch_vcdr(m, thres=0.5, delta=1):
    lens = []
    for c in (1, 2):
        rows = (m[c] >= thres).any(dim=1).nonzero().view(-1)
        if rows.numel() == 0:
            return torch.tensor(-1. if c == 1 else 0., device=m.device)
        lens.append(rows.max() - rows.min() - delta)
    return lens[1] / (lens[0] + 0.0001)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'frag_bench.json'))
    a = ap.parse_args()
    assert a.reps >= 20, 'the median is taken over at least 20 repetitions'
    dev = torch.device('cuda', 0)
    L = segx.lib()
    try:
        from scipy import ndimage
        label, labeller = (lambda fg: ndimage.label(fg, structure=np.ones((3, 3), int))[0]), 'scipy.ndimage.label'
    except ImportError:
        label, labeller = cpu_labels, 'torch minimum propagation (CPU)'
    out = {'tool': 'frag_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'host_reps': a.host_reps, 'host_labeller': labeller,
           'cases': {}}
    for name, (P, n) in (('1x2048x2048', (1, 2048)), ('6x512x512', (6, 512))):
        seg = fundus_like(P, n, dev)
        pred, gt = nhot_of(seg), nhot_of(torch.roll(seg, (n // 64, -(n // 50)), dims=(1, 2)))
        labels = torch.empty(seg.shape, dtype=torch.int32, device=dev)
        sizes, keep, clean = torch.empty_like(labels), torch.empty(P, 2, dtype=torch.int32, device=dev), torch.empty_like(seg)
        forms = {'remove_fragmentary_segs': lambda: infer2d.remove_fragmentary_segs(seg, 255),
                 'ccl2d': lambda: L.ccl2d(seg, 255, labels, sizes, P, n, n),
                 'keep2': lambda: L.frag_keep2(sizes, keep, P, n, n),
                 'apply': lambda: L.frag_apply(seg, labels, keep, clean, P, n, n, 255),
                 'vcdr_error': lambda: [(infer2d.calc_vcdr(gt[i]) - infer2d.calc_vcdr(pred[i])).abs() for i in range(P)],
                 'torch_vcdr_error': lambda: [(torch_vcdr(gt[i]) - torch_vcdr(pred[i])).abs().cpu() for i in range(P)]}
        ms = {k: [] for k in forms}
        for i in range(a.warmup + a.reps):
            for k, fn in forms.items():
                t = timed(fn)
                if i >= a.warmup:
                    ms[k].append(t)
        host = []
        for i in range(1 + a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = host_remove(seg, 255, label)
            torch.cuda.synchronize()
            if i:
                host.append((time.perf_counter() - t0) * 1e3)
        ours = infer2d.remove_fragmentary_segs(seg, 255)
        same_vcdr = all(torch.equal(x.cpu(), y) for x, y in zip(forms['vcdr_error'](), forms['torch_vcdr_error']()))
        out['cases'][name] = {'median_ms': {k: round(statistics.median(v), 4) for k, v in ms.items()}, 'min_ms': {k: round(min(v), 4) for k, v in ms.items()},
                              'host_remove_median_ms': round(statistics.median(host), 3), 'host_remove_min_ms': round(min(host), 3),
                              'equals_host_result': bool(torch.equal(ours, ref)), 'vcdr_equals_torch': bool(same_vcdr),
                              'components': int((sizes > 0).sum()), 'pixels_removed': int((ours != seg).sum())}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
