"""Segtran2d on the ResNet backbones, timed on one device at the cfg2 shape (512 x 512, batch 6, 3 transformer layers).

  python tools/resnet_bench.py [--steps 10] [--warmup 3] [--reps 20] [--inner 5] [--out profiles/resnet_bench.json]

(a) Per backbone (resnet34, resnet101): the train step (forward, loss, backward, clip + BertAdam; synthetic weights, dropout at the trainer's default) and the eval
    forward under torch.no_grad(), unfolded and with BatchNorm folded.  A figure is the median of `steps` warm calls, each between two HIP events, after `warmup`
    calls; the minimum and the maximum are kept next to it.
(b) The block-closing pass of resnet.hip on the largest block output of resnet101 at that shape (layer1: 6 x 256 x 256 x 256 floats, 403 MB):
      training form   SF.add_relu(z): one read, one write;  its backward: two reads, one write
      folded form     SF.add_relu(z, shortcut, bias, out=z): two reads, one write, in place
    against ATen's relu / relu_ and threshold_backward on the same tensors.  A timing is `inner` launches between two HIP events, a figure the median of `reps`
    timings; bytes/s = the bytes the pass has to move / that time.
Nobody has a parent-commit number for a model that did not exist: the numbers are written down, there is no threshold.  Output: ONE JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
from segtran_amd import engine, functional as SF               # noqa: E402
from sliding_bench import timed                                # noqa: E402

BLOCK_OUT = (6, 256, 256, 256)                                 # layer1 of resnet101 at 512 x 512 with the stride-2 stem and no max-pool (bb_feat_upsize)


def stats(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def model_times(bb, a, dev):
    cfg = engine.CONFIGS['cfg2']
    B = cfg['bs']
    torch.manual_seed(0); SF.manual_seed(0)
    net = engine.build_model(cfg, dev, backbone_type=bb)
    x, raw = engine.synth_batch(cfg, B, dev)
    net.train()
    opt = engine.init_optimizer(net, cfg['task'], t_total=10000, warmup_steps=500)
    step = engine.TrainStep(net, opt, cfg['task'])
    for _ in range(a.warmup):
        step(x, raw)
    torch.cuda.synchronize()
    res = {'train_step': stats([timed(lambda: step(x, raw)) for _ in range(a.steps)]), 'loss_finite': bool(torch.isfinite(step.stats[0]).item())}
    del step, opt
    net.eval()
    with torch.no_grad():
        for name, fold in (('eval_unfolded', False), ('eval_folded', True)):
            if fold:
                net.fold_batchnorm()
            for _ in range(a.warmup):
                y = net(x)
            torch.cuda.synchronize()
            res[name] = stats([timed(lambda: net(x)) for _ in range(a.steps)])
            if fold:
                err = (net(x) - y_unfolded).abs().max().item()
                res['folded_vs_unfolded_max_abs'] = err
                res['logit_absmax'] = y_unfolded.abs().max().item()
            else:
                y_unfolded = y.clone()
    res['parameters'] = sum(p.numel() for p in net.parameters())
    return res


def pass_times(a, dev):
    g = torch.Generator(device='cpu').manual_seed(1)
    n = 1
    for v in BLOCK_OUT:
        n *= v
    z = torch.randn(BLOCK_OUT[0] * BLOCK_OUT[1], 1024, generator=g).repeat(1, n // (BLOCK_OUT[0] * BLOCK_OUT[1] * 1024)).view(BLOCK_OUT).to(dev)
    r = z.flip(1).contiguous()
    dy = z.roll(1, 1).contiguous()
    bias = torch.randn(BLOCK_OUT[1], generator=g).to(dev)
    y = SF.add_relu(z)
    zi = z.clone()
    nbytes = 4 * n
    forms = {
        'add_relu_fwd': (lambda: SF.add_relu(z), 2 * nbytes),
        'aten_relu': (lambda: torch.relu(z), 2 * nbytes),
        'aten_relu_': (lambda: torch.relu_(zi), 2 * nbytes),
        'add_relu_bwd': (lambda: SF._AddRelu.backward(_Ctx(y), dy), 3 * nbytes),
        'aten_threshold_backward': (lambda: torch.ops.aten.threshold_backward(dy, y, 0), 3 * nbytes),
        'add_relu_folded_inplace': (lambda: SF.add_relu(zi, r, bias=bias, out=zi), 3 * nbytes),
        'aten_add_bias_add_relu_': (lambda: torch.relu_(zi.add_(bias.view(1, -1, 1, 1)).add_(r)), 7 * nbytes),
    }
    assert torch.equal(y, torch.relu(z)) and torch.equal(SF._AddRelu.backward(_Ctx(y), dy)[0], torch.ops.aten.threshold_backward(dy, y, 0))
    out = {'shape': list(BLOCK_OUT), 'tensor_mb': round(nbytes / 1e6, 1)}
    with torch.no_grad():
        for fn, _ in forms.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, (fn, _) in forms.items():
                ms[k].append(timed(lambda: [fn() for _ in range(a.inner)]) / a.inner)
    for k, (_, moved) in forms.items():
        med = statistics.median(ms[k])
        out[k] = {'median_ms': round(med, 4), 'min_ms': round(min(ms[k]), 4), 'bytes_moved': moved, 'tb_per_s': round(moved / (med * 1e-3) / 1e12, 3)}
    return out


class _Ctx:
    """what _AddRelu.backward reads from its context: the saved output and the plane geometry"""

    def __init__(self, y):
        self.saved_tensors = (y,)
        self.cfg = (y.shape[0] * y.shape[1], y.numel() // (y.shape[0] * y.shape[1]))
        self.has_resid = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--backbones', default='resnet34,resnet101')
    ap.add_argument('--out', default=os.path.join('profiles', 'resnet_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'resnet_bench times the device: it needs the GPU'
    dev = torch.device('cuda', 0)
    res = {'tool': 'resnet_bench', 'device': torch.cuda.get_device_name(0), 'shape': 'cfg2: 512 x 512, batch 6, 3 transformer layers', 'steps': a.steps,
           'warmup': a.warmup, 'reps': a.reps, 'inner': a.inner, 'add_relu': pass_times(a, dev)}
    for bb in [b for b in a.backbones.split(',') if b]:
        res[bb] = model_times(bb, a, dev)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
