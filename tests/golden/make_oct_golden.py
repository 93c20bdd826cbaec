"""Golden fixtures of the OCT task (10 one-hot classes) from the REAL reference: oct2d.npz and seg2d_oct_train.npz.

Runs only where the reference checkout exists (as make_golden.py, whose helpers it uses).  The reference's own functions are executed -- index_to_onehot,
onehot_inv_map, harden_segmap2d (dataloaders/datasets2d.py), calc_batch_metric / calc_dice (test_util2d.py), the weight statements of train2d.py and the
reference Segtran2d -- and only their inputs and outputs are stored.
Usage:  python tests/golden/make_oct_golden.py [oct2d] [train]
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402
from make_golden import R, O                               # noqa: E402
from segtran_amd.synth import load_synth, sample, synth_oct_mask   # noqa: E402

NUM_CLASSES = 10


class _CpuTensor(torch.Tensor):
    """train2d.py moves its weight tensors with .cuda(); here they stay where they are"""

    def cuda(self, *a, **kw):
        return self


class _Torch:
    def __getattr__(self, k):
        return getattr(torch, k)

    def tensor(self, *a, **kw):
        return torch.tensor(*a, **kw).as_subclass(_CpuTensor)

    def ones(self, *a, **kw):
        return torch.ones(*a, **kw).as_subclass(_CpuTensor)


def ref_oct_bce_weight():
    """the 'bce_weight' entry of the 'oct' task in train2d.py's table of defaults (a literal: evaluated, not copied)"""
    src = open('/root/reference/code/train2d.py').read()
    a = src.index("'bce_weight':", src.index("'oct':"))
    a = src.index('[', a)
    return ast.literal_eval(src[a:src.index(']', a) + 1])


def ref_weights(bce_weight, focus_class):
    """train2d.py:813-814 and :1123-1127, the reference's own statements"""
    import argparse
    args = argparse.Namespace(bce_weight=list(bce_weight), num_classes=len(bce_weight), focus_class=focus_class)
    ns = dict(args=args, torch=_Torch())
    exec(compile(mg._ref_loop_block('    args.bce_weight = torch.tensor(args.bce_weight).cuda()', 'args.bce_weight.sum()\n'), 'train2d.py:813-814', 'exec'), ns)
    exec(compile(mg._ref_loop_block('    class_weights = torch.ones(args.num_classes).cuda()', '    class_weights /= class_weights.sum()\n'), 'train2d.py:1123-1127', 'exec'), ns)
    return args.bce_weight.as_subclass(torch.Tensor).float(), ns['class_weights'].as_subclass(torch.Tensor).float()


def _eighths(g, *shape):
    """uniform draws rounded to multiples of 1/8: exact in float32, so values exactly at T = 0.5 are frequent"""
    return torch.round(torch.rand(*shape, generator=g) * 8) / 8


def case_oct2d():
    d2 = mg._ref_functions('dataloaders/datasets2d.py', ['index_to_onehot', 'onehot_inv_map', 'harden_segmap2d'])
    t2 = mg._ref_functions('test_util2d.py', ['calc_batch_metric', 'calc_dice'], dict(harden_segmap2d=d2['harden_segmap2d']))
    to_onehot, inv_map, harden = d2['index_to_onehot'], d2['onehot_inv_map'], d2['harden_segmap2d']
    g = torch.Generator().manual_seed(41)
    arrs = {}
    # index_to_onehot: the three input forms, at 10 and at 16 classes
    ix4 = torch.randint(0, NUM_CLASSES, (2, 1, 1, 257), generator=g).to(torch.uint8)
    ix2 = torch.randint(0, NUM_CLASSES, (3, 85), generator=g).to(torch.uint8)
    ix16 = torch.randint(0, 16, (2, 1, 257), generator=g).to(torch.uint8)
    arrs.update(ix4=ix4, oh4=to_onehot(ix4, NUM_CLASSES).to(torch.uint8), oh3=to_onehot(ix4[:, 0], NUM_CLASSES).to(torch.uint8),
                ix2=ix2, oh2=to_onehot(ix2, NUM_CLASSES).to(torch.uint8), ix16=ix16, oh16=to_onehot(ix16, 16).to(torch.uint8))
    assert arrs['oh4'].shape == (2, 10, 1, 257) and arrs['oh3'].shape == (2, 10, 1, 257) and arrs['oh2'].shape == (10, 3, 85) and arrs['oh16'].shape == (2, 16, 1, 257)
    # onehot_inv_map: n-hot maps with ties (several classes on: the lowest index wins) and a pixel with nothing on (index 0)
    nhot = (torch.rand(2, NUM_CLASSES, 6, 9, generator=g) > 0.8).float()
    nhot[0, :, 0, 0] = 0
    nhot[1, :, 5, 8] = 0
    nhot[0, :, 1, 1] = 1
    colormap = torch.randint(0, 256, (NUM_CLASSES, 3), generator=g).to(torch.uint8)
    assert (nhot.sum(1) > 1).sum() > 10 and (nhot.sum(1) == 0).sum() >= 2
    arrs.update(nhot=nhot.to(torch.uint8), colormap=colormap, inv_rgb=inv_map(nhot, colormap), inv_idx=inv_map(nhot),
                inv_rgb3=inv_map(nhot[1], colormap), inv_idx3=inv_map(nhot[1]))
    assert arrs['inv_rgb'].dtype == torch.uint8 and arrs['inv_idx'].dtype == torch.int64 and arrs['inv_rgb'].shape == (2, 6, 9, 3)
    # harden_segmap2d at 9, 10 and 16 classes, values exactly at T
    for C in (9, 10, 16):
        soft = _eighths(g, 2, C, 5, 7)
        soft[0, 1:, 0, 0] = 0.25                                   # no class on -> background
        soft[0, 1:, 0, 1] = 0.5                                    # every class exactly at T -> all on
        assert (soft == 0.5).sum() > 20
        arrs['soft%d' % C] = soft
        arrs['hard%d' % C] = harden(soft).to(torch.uint8)
        arrs['hard%d_3d' % C] = harden(soft[1]).to(torch.uint8)
    # calc_batch_metric at 10 classes, two instances of different shapes; class 7 is absent from prediction and mask (Dice 1), class 8 from the mask only
    preds, gts, masks = [], [], []
    for shape in ((12, 20), (9, 16)):
        p = _eighths(g, NUM_CLASSES, *shape)
        p[7] = 0.375
        m = torch.randint(0, NUM_CLASSES, shape, generator=g)
        m[(m == 7) | (m == 8)] = 6
        preds.append(p); masks.append(m.to(torch.uint8)); gts.append(to_onehot(m, NUM_CLASSES))
    metric = t2['calc_batch_metric'](preds, gts, NUM_CLASSES)
    assert metric.shape == (2, 9) and (metric[:, 6] == 1).all() and (metric[:, 7] < 1e-6).all() and (metric[:, :6] > 0.05).all()
    for i in range(2):
        arrs['metric_soft%d' % i] = preds[i]; arrs['metric_mask%d' % i] = masks[i]
    arrs['metric'] = metric.astype(np.float64)
    # the oct loss weights, with and without --focus 3
    bw = ref_oct_bce_weight()
    assert len(bw) == NUM_CLASSES
    pw, cw = ref_weights(bw, -1)
    pw3, cw3 = ref_weights(bw, 3)
    assert torch.equal(pw, pw3) and cw3[3] == 2 * cw3[1]
    arrs.update(bce_weight=np.array(bw, dtype=np.float32), pos_weight=pw, class_w=cw, class_w_focus3=cw3)
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
    path = os.path.join(mg.OUT_DIR, 'oct2d.npz')
    np.savez_compressed(path, **out)                               # not mg.save: `metric` stays float64, as the reference returns it
    print('  wrote oct2d (%.0f KB)' % (os.path.getsize(path) / 1024))


def case_train():
    """the reference Segtran2d with 10 classes, 1 layer, 32 attractors on a 2 x 3 x 64 x 96 batch (8 x 12 tokens), train mode, dropout and drop-connect off: logits,
    loss and sampled gradients in the format of make_golden.run_seg2d; the index mask is mapped by the reference's index_to_onehot"""
    A, B, H, W, dims = 32, 2, 64, 96, [1792, 1792]
    net = R.ref_segtran2d(num_classes=NUM_CLASSES, num_attractors=A, num_translayers=1, compress=(1, 1), dropout_prob=0)
    sd = load_synth(net)
    net.train()
    net.backbone._global_params = net.backbone._global_params._replace(drop_connect_rate=0.0)
    g = torch.Generator().manual_seed(16)
    x = torch.randn(B, 3, H, W, generator=g)
    mask = synth_oct_mask(B, H, W, NUM_CLASSES, 1338)
    to_onehot = mg._ref_functions('dataloaders/datasets2d.py', ['index_to_onehot'])['index_to_onehot']
    nhot = to_onehot(mask, NUM_CLASSES)
    assert nhot.shape == (B, NUM_CLASSES, H, W) and (nhot.sum(dim=(0, 2, 3)) > 0).all()
    pw = O.bce_pos_weight(ref_oct_bce_weight())
    assert torch.equal(pw, ref_weights(ref_oct_bce_weight(), -1)[0])
    y = R.quiet(net, x)
    loss = O.seg_loss(y, nhot, pw)[0]                        # composition restated; pinned by make_golden.case_loss
    loss.backward()
    sdg = mg.req(sd)
    yo = O.segtran2d_forward(sdg, x, dims, training=True)
    lo = O.seg_loss(yo, nhot, pw)[0]; lo.backward()
    mg.close(yo, y, 2e-5, 'seg2d_oct_train logits')
    og = mg.oracle_grads(sdg)
    rg = dict(net.named_parameters())
    gscale = max(p.grad.abs().max().item() for p in rg.values() if p.grad is not None)
    arrs = dict(x=x, mask=mask, logits=y, labels=(y > 0), loss=loss.detach(), margin=y.abs().min().detach(), dims=np.array(dims), A=np.array(A),
                train=np.array(1), nhot=nhot.to(torch.uint8))
    for k in mg.GRAD_KEYS_2D:
        if k not in rg:
            continue
        gr = rg[k].grad
        assert (og[k] - gr).abs().max().item() <= 3e-4 * gscale, (k, (og[k] - gr).abs().max().item(), gscale)
        arrs['grad:' + k] = sample(gr)
    arrs['gscale'] = np.array(gscale)
    arrs['unused'] = np.array(sorted(k for k, p in rg.items() if p.grad is None))
    arrs['zero_grad'] = np.array(sorted(k for k, p in rg.items() if p.grad is not None and p.grad.abs().max() == 0))
    mg.save('seg2d_oct_train', **arrs)


CASES = {'oct2d': case_oct2d, 'train': case_train}

if __name__ == '__main__':
    for name in (sys.argv[1:] or list(CASES)):
        print(name)
        CASES[name]()
