"""Folded eval-mode throughput at the two precisions of the bf16 tile engine: six-term (fp32-equivalent, the default) and three-term (inference_precision('bf16x3')).

  python tools/precision_bench.py [--reps 20] [--warmup 5] [--cfgs cfg1,cfg2,cfg3] [--no-window] [--no-gemm] [--out profiles/precision_infer_bench.json]
  python tools/precision_bench.py --3d [--reps 20] [--warmup 5] [--cfgs cfg4,cfg5] [--no-conv] [--out profiles/precision_infer_bench_3d.json]

One process: for every configuration (its BASELINE batch) the SAME folded model runs the eval forward six-term and three-term in alternation -- `warmup` pairs,
then `reps` pairs, each forward timed with HIP events on the launch stream; medians, quartiles and the ratio are reported, with the launch counters of one
three-term forward (how many bf16 tile-engine launches there are and how many of them ran three-term).  Then the fused sliding-window evaluation of a 576 x 576
image with the cfg1 model, the same way, and the five GEMM shapes of the cfg2 forward with the most time, each alone at both precisions (tools/gemm_bench.py
style rows).  The six-term forward is the path every earlier commit ran, so the ratio needs no second box.  Writes the JSON to --out and prints it as one line.

--3d: the eval forwards of the 3-D configurations (cfg4 112 x 112 x 96, cfg5 128^3, batch 4; BatchNorm3d is not folded) the same way, and the five
forward convolutions of each forward with the most time, each alone at both precisions on operands of the same geometry and strides.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from segtran_amd import engine, infer2d, segx                  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {'median_ms': round(statistics.median(ms), 4), 'q1_ms': round(q[0], 4), 'q3_ms': round(q[2], 4), 'min_ms': round(min(ms), 4)}


def alternate(run, reps, warmup):
    """-> {'fp32': [...ms], 'bf16x3': [...ms]}: the two precisions take turns, so drift of the box hits both alike"""
    ms = {'fp32': [], 'bf16x3': []}
    with torch.no_grad():
        for i in range(warmup + reps):
            for prec in ('fp32', 'bf16x3'):
                with infer2d.inference_precision(prec):
                    t = timed(run)
                if i >= warmup:
                    ms[prec].append(t)
    return ms


def row(ms, extra):
    six, three = stats(ms['fp32']), stats(ms['bf16x3'])
    return dict(extra, six_term=six, three_term=three, three_over_six=round(three['median_ms'] / six['median_ms'], 4))


def counters(run):
    L = segx.lib()
    with torch.no_grad(), infer2d.inference_precision('bf16x3'):
        L.x6_launches(); L.x3_launches()
        run()
        torch.cuda.synchronize()
        return {'bf16_engine_launches': L.x6_launches(), 'three_term_launches': L.x3_launches()}


def gemm_shapes(net, x, top):
    """the `top` GEMM shapes of one six-term forward with the most time: [(total ms, calls, (M, N, K, nb, A k-contiguous, B k-contiguous, splitk, tile))]"""
    L = segx.lib()
    with torch.no_grad():
        net(x)
        L.gemm_prof = []
        net(x)
        torch.cuda.synchronize()
        prof, L.gemm_prof = L.gemm_prof, None
    by = {}
    for e0, e1, _, tag, on_x6 in prof:
        if on_x6 and len(tag) == 8:
            t = by.setdefault(tag, [0.0, 0])
            t[0] += e0.elapsed_time(e1); t[1] += 1
    return sorted(((v[0], v[1], k) for k, v in by.items()), reverse=True)[:top]


def gemm_row(tag, reps, warmup, dev):
    M, N, K, nb, akc, bkc, sk, tile = tag
    L = segx.lib()
    A = torch.randn(nb, M, K, device=dev) if akc else torch.randn(nb, K, M, device=dev)
    B = torch.randn(nb, N, K, device=dev) if bkc else torch.randn(nb, K, N, device=dev)
    C = torch.empty(nb, M, N, device=dev)
    a_str = (0, M * K, K, 1) if akc else (0, M * K, 1, M)
    b_str = (0, N * K, K, 1) if bkc else (0, N * K, 1, N)
    ws = torch.empty(sk * nb * M * N, device=dev) if sk > 1 else None

    def run():
        L.gemm(A, B, C, M, N, K, a_str, b_str, (0, M * N, N), nb=(1, nb), splitk=sk, workspace=ws, tile=tile)
    with L.tuned(x6_terms=3):
        route = L.gemm_route(A, B, M, N, K, a_str, b_str, nb=(1, nb), splitk=sk, tile=tile)
    r = row(alternate(run, reps, warmup), {'M': M, 'N': N, 'K': K, 'nb': nb, 'a_kcontig': akc, 'b_kcontig': bkc, 'splitk': sk, 'family': route[0], 'tile': route[1],
                                           'terms_at_3': route[2]})
    flop = 2.0 * M * N * K * nb
    r['six_term_tflops'] = round(flop / r['six_term']['median_ms'] / 1e9, 1)
    r['three_term_tflops'] = round(flop / r['three_term']['median_ms'] / 1e9, 1)
    return r


class conv_recorder:
    """for one block: every conv3d_halo_fwd / conv3d_fwd call of the library object with HIP events around it and what is needed to repeat it alone"""

    def __init__(self):
        self.L, self.calls = segx.lib(), []

    def _wrap(self, kind, orig):
        def f(X, W, Y, B, Cout, geom, *a, **k):
            if kind == 'halo':
                key = (kind, B, Cout, tuple(int(v) for v in geom), 1, True, int(k.get('x_bs', 0)), int(k.get('y_bs', 0)))
            else:
                splitk = a[0] if a else k.get('splitk', 1)
                key = (kind, B, Cout, tuple(int(v) for v in geom), int(splitk), bool(k.get('packed', False)), int(k.get('x_bs', 0)), int(k.get('y_bs', 0)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(X, W, Y, B, Cout, geom, *a, **k)
            e1.record()
            self.calls.append((key, e0, e1))
            return out
        return f

    def __enter__(self):
        halo, fwd = self.L.conv3d_halo_fwd, self.L.conv3d_fwd
        self.L.conv3d_halo_fwd, self.L.conv3d_fwd = self._wrap('halo', halo), self._wrap('igemm', fwd)
        return self

    def __exit__(self, *exc):
        del self.L.conv3d_halo_fwd, self.L.conv3d_fwd


def conv_shapes(net, x, top):
    """the `top` forward convolutions of one six-term forward with the most time: [(total ms, calls, key)]"""
    with torch.no_grad():
        net(x)
        with conv_recorder() as rec:
            net(x)
        torch.cuda.synchronize()
    by = {}
    for key, e0, e1 in rec.calls:
        t = by.setdefault(key, [0.0, 0])
        t[0] += e0.elapsed_time(e1); t[1] += 1
    return sorted(((v[0], v[1], k) for k, v in by.items()), reverse=True)[:top]


def conv_row(key, reps, warmup, dev):
    """one convolution alone, six-term and three-term in alternation, on random operands of the recorded geometry and sample strides"""
    kind, B, Cout, geom, splitk, packed, x_bs, y_bs = key
    L = segx.lib()
    Cin, P, KV = geom[0], geom[4] * geom[5] * geom[6], geom[7] * geom[8] * geom[9]
    isz = geom[1] * geom[2] * geom[3]
    X = torch.randn((B - 1) * (x_bs or Cin * isz) + Cin * isz, device=dev)
    Y = torch.empty((B - 1) * (y_bs or Cout * P) + Cout * P, device=dev)
    W = torch.randn(Cout, Cin, geom[7], geom[8], geom[9], device=dev) * 0.05
    if kind == 'halo':
        Wq = L.conv3d_halo_pack(W, Cout, Cin, 0)
        run = lambda: L.conv3d_halo_fwd(X, Wq, Y, B, Cout, geom, x_bs=x_bs, y_bs=y_bs)        # noqa: E731
    else:
        ws = torch.empty(splitk * B * Cout * P, device=dev) if splitk > 1 else None
        run = lambda: L.conv3d_fwd(X, W, Y, B, Cout, geom, splitk, ws, packed=packed, x_bs=x_bs, y_bs=y_bs)      # noqa: E731
    L.x6_launches(); L.x3_launches()
    with L.tuned(x6_terms=3):
        run()
        torch.cuda.synchronize()
        n6, n3 = L.x6_launches(), L.x3_launches()
    r = row(alternate(run, reps, warmup), {'kernel': kind, 'B': B, 'Cout': Cout, 'geom': list(geom), 'splitk': splitk, 'packed': packed, 'x_bs': x_bs, 'y_bs': y_bs,
                                           'bf16_engine_launches_at_3': n6, 'three_term_launches_at_3': n3})
    flop = 2.0 * B * Cout * P * Cin * KV
    r['six_term_tflops'] = round(flop / r['six_term']['median_ms'] / 1e9, 1)
    r['three_term_tflops'] = round(flop / r['three_term']['median_ms'] / 1e9, 1)
    return r


def main_3d(a):
    dev = torch.device('cuda', 0)
    out = {'tool': 'precision_bench --3d', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'configs': {}}
    for name in (a.cfgs or 'cfg4,cfg5').split(','):
        c = engine.CONFIGS[name]
        net = engine.build_model(name, dev, dropout_prob=0.0).eval()
        x, _ = engine.synth_batch(name, c['bs'], dev)
        run = lambda: net(x)                                   # noqa: E731
        out['configs'][name] = row(alternate(run, a.reps, a.warmup), dict(counters(run), batch=c['bs'], size=list(c['size'])))
        if not a.no_conv:
            out[name + '_convs'] = [dict(conv_row(key, a.reps, a.warmup, dev), forward_ms=round(ms, 4), calls=n) for ms, n, key in conv_shapes(net, x, 5)]
        del net, run
        torch.cuda.empty_cache()
    line = json.dumps(out)
    with open(a.out or os.path.join(ROOT, 'profiles', 'precision_infer_bench_3d.json'), 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--3d', dest='three_d', action='store_true', help='the 3-D configurations (cfg4, cfg5) and their convolutions')
    ap.add_argument('--no-conv', action='store_true')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cfgs', default=None)
    ap.add_argument('--no-window', action='store_true')
    ap.add_argument('--no-gemm', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.reps >= 20, 'the median is taken over at least 20 repetitions'
    if a.three_d:
        return main_3d(a)
    a.cfgs, a.out = a.cfgs or 'cfg1,cfg2,cfg3', a.out or os.path.join(ROOT, 'profiles', 'precision_infer_bench.json')
    dev = torch.device('cuda', 0)
    out = {'tool': 'precision_bench', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'configs': {}}
    for name in a.cfgs.split(','):
        c = engine.CONFIGS[name]
        net = engine.build_model(name, dev, dropout_prob=0.0).eval()
        net.fold_batchnorm()
        x, _ = engine.synth_batch(name, c['bs'], dev)
        run = lambda: net(x)                                   # noqa: E731
        out['configs'][name] = row(alternate(run, a.reps, a.warmup), dict(counters(run), batch=c['bs'], size=list(c['size'])))
        if name == 'cfg2' and not a.no_gemm:
            out['cfg2_gemms'] = [dict(gemm_row(tag, a.reps, a.warmup, dev), forward_ms=round(ms, 4), calls=n) for ms, n, tag in gemm_shapes(net, x, 5)]
        del net, run
        torch.cuda.empty_cache()
    if not a.no_window:
        c = engine.CONFIGS['cfg1']
        net = engine.build_model('cfg1', dev, dropout_prob=0.0).eval()
        net.fold_batchnorm()
        img, _ = engine.synth_batch(dict(c, size=(576, 576)), 1, dev)
        S = c['size'][0]
        run_w = lambda: infer2d.test_single_batch(net, img, (S, S), (S, S), (S // 2, S // 2), c['task'], c['num_classes'], fused=True)      # noqa: E731
        out['test_single_batch_576'] = row(alternate(run_w, a.reps, a.warmup), dict(counters(run_w), model='cfg1', window=[S, S], stride=[S // 2, S // 2], fused=True))
    line = json.dumps(out)
    with open(a.out, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
