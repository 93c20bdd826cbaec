"""The evaluation tail of the n-hot 2-D tasks in one launch (metrics.hip: segx_nhot_case_tail; SF.nhot_case_tail, infer2d.vcdr_from_extents) on the fiber emulator
(CPU) and on the GPU (-m gpu).  Referees: the project's composed path on the same backend -- SF.interp_linear -> SF.harden_segmap(mode 0) -> integer sums ->
SF.row_extent -> SF.nhot_to_values -- and, where the source size is the destination's or exactly half of it (the 2x up-sampling has the weights 1/4 and 3/4, so on
multiples of 1/8 no operation rounds and torch on the CPU is exact too), a torch restatement on the CPU.  Integers, 0 / 1 maps and single rounded float32
operations: every comparison is for EQUALITY, no pixel is left out.

Destination sizes, with T = SEGX_CASE_TAIL_THREADS (a workgroup covers 4 T destination pixels per trip): 1 x 1, 1 x 3, 3 x 5 (one thread, cut quads, the byte path),
31 x 33 = 4 T - 1, 32 x 32 = 4 T, 25 x 41 = 4 T + 1 (the last thread of a workgroup cut, full, one pixel into a second workgroup; 32 x 32 is the only one on the
16-byte path), 41 x 50 = 8 T + 2 (two workgroups and a cut quad; rows that straddle quads) and, GPU only, 1450 x 1450 > 4 T MAX_BLOCKS (the capped grid takes a
second trip).  Source sizes: the destination's (no resampling), half of it where it is even, and 5 x 7 -> 9 x 13 (up, non-integer), 16 x 24 -> 7 x 5 (down),
8 x 40 -> 25 x 41 (anisotropic).

Data: soft is uniform, rounded to multiples of 1/8 (exact in float32; p == T is frequent), with a few NaN cells; the ground truth is a union of random rectangles.
Image i of a case is one of five kinds in turn: random, no disc (class 1 empty in prediction and ground truth), no cup (class 2), class 1 only in row 0, the last
class only in the last row -- both special values of the vCDR and both edges of the extents occur."""
import functools
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from segtran_amd import functional as SF
from segtran_amd import infer2d, segx
from segtran_amd.dataloaders.datasets2d import fundus_map_mask, polyp_map_mask

T, MAXB = segx.SegxLib.CASE_TAIL_THREADS, segx.SegxLib.CASE_TAIL_MAX_BLOCKS
DESTS = [(1, 1), (1, 3), (3, 5), (31, 33), (32, 32), (25, 41), (41, 50)]
GEOMETRIES = [(d, d) for d in DESTS] + [((16, 16), (32, 32)), ((5, 7), (9, 13)), ((16, 24), (7, 5)), ((8, 40), (25, 41))]      # (source, destination)
BIG = (1450, 1450)
KINDS = ['random', 'no-disc', 'no-cup', 'row0', 'last-row']
VALUES = {2: (0, 255), 3: (255, 128, 0), 10: tuple(range(7, 250, 25))}
CPU = torch.device('cpu')


def test_constants_match_the_header_and_place_the_sizes():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'segx.h')).read()
    assert int(re.search(r'#define SEGX_CASE_TAIL_THREADS (\d+)', hdr).group(1)) == T
    assert int(re.search(r'#define SEGX_CASE_TAIL_MAX_BLOCKS (\d+)', hdr).group(1)) == MAXB
    assert T % 64 == 0
    assert [h * w for h, w in DESTS[3:]] == [4 * T - 1, 4 * T, 4 * T + 1, 8 * T + 2]
    assert BIG[0] * BIG[1] > 4 * T * MAXB and BIG[0] * BIG[1] % 4 == 0
    assert [s for s in DESTS if s[0] * s[1] % 4 == 0] == [(32, 32)]


def blobs(g, n, H, W):
    """[n, H, W] 0 / 1 floats: per plane the union of two random rectangles"""
    out = torch.zeros(n, H, W, device=CPU)
    for p in range(n):
        for _ in range(2):
            y = torch.randint(0, H, (2,), generator=g, device=CPU).sort()[0].tolist()
            x = torch.randint(0, W, (2,), generator=g, device=CPU).sort()[0].tolist()
            out[p, y[0]:y[1] + 1, x[0]:x[1] + 1] = 1.0
    return out


@functools.lru_cache(None)
def case(B, C, src, dst, kind0=0):
    """CPU tensors (soft [B, C, h, w], gt n-hot float [B, C, H, W]); image i is of kind KINDS[(kind0 + i) % 5]"""
    (h, w), (H, W) = src, dst
    g = torch.Generator().manual_seed(7 + 1000 * B + 100 * C + 13 * h + 17 * w + 19 * H + 23 * W + kind0)
    soft = torch.round(torch.rand(B, C, h, w, generator=g, device=CPU) * 8) / 8
    gt = blobs(g, B * C, H, W).view(B, C, H, W)
    last = C - 1
    for i in range(B):
        kind = KINDS[(kind0 + i) % 5]
        if kind == 'no-disc':
            gt[i, 1] = 0; soft[i, 1] = 0.25
        elif kind == 'no-cup' and C > 2:
            gt[i, 2] = 0; soft[i, 2] = 0.25
        elif kind == 'row0':
            gt[i, 1] = 0; gt[i, 1, 0] = 1; soft[i, 1] = 0.125; soft[i, 1, 0] = 0.875
        elif kind == 'last-row':
            gt[i, last] = 0; gt[i, last, -1] = 1; soft[i, last] = 0.125; soft[i, last, -1] = 0.875
    flat = soft.view(-1)
    flat[torch.randperm(flat.numel(), generator=g, device=CPU)[:flat.numel() // 40]] = float('nan')
    return soft, gt


def stack_extents(hard, gt, C):
    """int32 [B, 2, 2, 2] from SF.row_extent of classes 1 and 2 of the hardened and the ground-truth maps; the class-2 entries of a 2-class task are empty"""
    B, _, H, W = hard.shape

    def half(m):
        e = torch.empty(B, 2, 2, dtype=torch.int32, device=m.device)
        e[..., 0], e[..., 1] = H, -1
        k = min(C, 3) - 1
        e[:, :k] = SF.row_extent(m[:, 1:1 + k].reshape(B * k, H, W).contiguous(), 0.5).view(B, k, 2)
        return e
    return torch.stack([half(hard), half(gt)], dim=1)


def composed(soft, gt, size, values, Tv=0.5):
    """(counts, ext, labels, hard) through the product's separate calls, on the tensors' device"""
    x = soft if tuple(soft.shape[2:]) == tuple(size) else SF.interp_linear(soft, size)
    hard = SF.harden_segmap(x.contiguous(), None, mode=0, T=Tv, want_soft=False)[1]
    p, g = hard[:, 1:] != 0, gt[:, 1:] >= 0.5
    counts = torch.stack([(p & g).sum(dim=(2, 3)), p.sum(dim=(2, 3)), g.sum(dim=(2, 3))], dim=-1).to(torch.int32)
    return counts, stack_extents(hard, gt, soft.shape[1]), SF.nhot_to_values(hard, values), hard


def torch_cpu(soft, gt, size, values, Tv=0.5):
    """the same four results restated with torch on the CPU: F.interpolate, threshold, sums, a loop over the rows"""
    soft, gt = soft.to(CPU), gt.to(CPU)
    B, C = soft.shape[:2]
    H, W = size
    x = soft if tuple(soft.shape[2:]) == (H, W) else F.interpolate(soft, size=(H, W), mode='bilinear', align_corners=False)
    on = x >= Tv
    on[:, 0] = ~on[:, 1:].any(dim=1)
    g = gt >= 0.5
    counts = torch.stack([(on & g).sum(dim=(2, 3)), on.sum(dim=(2, 3)), g.sum(dim=(2, 3))], dim=-1)[:, 1:].to(torch.int32)
    ext = torch.empty(B, 2, 2, 2, dtype=torch.int32, device=CPU)
    ext[..., 0], ext[..., 1] = H, -1
    for which, m in enumerate((on, g)):
        for b in range(B):
            for c in range(1, min(C, 3)):
                rows = m[b, c].any(dim=1).nonzero().view(-1)
                if rows.numel():
                    ext[b, which, c - 1, 0], ext[b, which, c - 1, 1] = int(rows[0]), int(rows[-1])
    labels = torch.zeros(B, H, W, dtype=torch.uint8, device=CPU)
    for c in range(C):
        labels[on[:, c]] = values[c]
    return counts, ext, labels, on.float()


def same(got, want):
    assert len(got) == len(want)
    for name, a, b in zip(('counts', 'ext', 'labels', 'hard'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a.cpu(), b.cpu()), name


def check(dev, B, C, src, dst, kind0):
    soft, gt = (t.to(dev) for t in case(B, C, src, dst, kind0))
    got = SF.nhot_case_tail(soft, gt, values=VALUES[C], want_extents=True, want_hard=True)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.uint8 and got[3].dtype == torch.float32
    assert tuple(got[0].shape) == (B, C - 1, 3) and tuple(got[1].shape) == (B, 2, 2, 2) and tuple(got[2].shape) == (B,) + dst and tuple(got[3].shape) == (B, C) + dst
    same(got, composed(soft, gt, dst, VALUES[C]))
    if src == dst or (2 * src[0], 2 * src[1]) == dst:
        same(got, torch_cpu(soft, gt, dst, VALUES[C]))
    return got


@pytest.mark.parametrize('C', [2, 3])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('k', range(len(GEOMETRIES)), ids=['%dx%d-to-%dx%d' % (s + d) for s, d in GEOMETRIES])
def test_all_outputs_equal_the_composed_path(backend, k, B, C):
    src, dst = GEOMETRIES[k]
    check(backend.dev, B, C, src, dst, (k + B) % 5)


def test_the_data_hits_thresholds_nans_and_every_special_image():
    """the inputs of the size tests: p == T and NaN occur, and over the kinds an empty disc, an empty cup, a class only in row 0 and only in the last row"""
    soft, gt = case(3, 3, (41, 50), (41, 50), 1)                                  # images: no-disc, no-cup, row0
    assert int((soft == 0.5).sum()) > 50 and int(soft.isnan().sum()) > 50
    _, ext, _, _ = torch_cpu(soft, gt, (41, 50), VALUES[3])
    assert ext[0, :, 0].tolist() == [[41, -1], [41, -1]] and ext[1, :, 1].tolist() == [[41, -1], [41, -1]] and ext[2, 1, 0].tolist() == [0, 0]
    soft, gt = case(3, 3, (41, 50), (41, 50), 3)                                  # images: row0, last-row, random
    _, ext, _, _ = torch_cpu(soft, gt, (41, 50), VALUES[3])
    assert ext[1, 1, 1].tolist() == [40, 40] and ext[1, 0, 1, 1] == 40 and ext[0, 0, 0, 0] == 0


@pytest.mark.parametrize('src', [(41, 50), (20, 25)])
def test_ten_classes_counts_only(backend, src):
    """C = 10 runs harden_cell<16>; only the counts are asked for"""
    dst = (41, 50)
    soft, gt = (t.to(backend.dev) for t in case(3, 10, src, dst, 0))
    counts, ext, labels, hard = SF.nhot_case_tail(soft, gt)
    assert ext is None and labels is None and hard is None
    assert torch.equal(counts.cpu(), composed(soft, gt, dst, VALUES[10])[0].cpu())
    assert int(counts[:, 3:, 0].min()) > 0                                        # the classes no special image empties: every one intersects its ground truth


@pytest.mark.gpu
@pytest.mark.parametrize('src', [BIG, (725, 725)])
def test_second_trip_of_the_grid_stride_loop(src):
    """H * W above 4 T MAX_BLOCKS: the grid is capped and the first workgroups take a second trip; without and with the resampling gather.  GPU only: 2.1 M pixels
    take tens of seconds on the fiber emulator, and the stride arithmetic is the one the small sizes run."""
    segx.use_library(None)
    check(torch.device('cuda', 0), 1, 3, src, BIG, 0)


def raw_mask(B, H, W, seed):
    """uint8 [B, 3, H, W] with values 0 / 1 / 128 / 255: channel 0 and channel 1 are independent blobs, so the exclusive form differs from the plain one"""
    g = torch.Generator().manual_seed(seed)
    m = blobs(g, B * 3, H, W).view(B, 3, H, W)
    level = torch.tensor([1, 128, 255], device=CPU)[torch.randint(0, 3, (B, 3, H, W), generator=g, device=CPU)]
    return (m * level).to(torch.uint8)


@pytest.mark.parametrize('src,dst', [((3, 5), (3, 5)), ((32, 32), (32, 32)), ((8, 40), (25, 41)), ((16, 16), (32, 32))])
@pytest.mark.parametrize('gt_map', ['fundus', 'fundus_exclusive', 'polyp'])
def test_raw_masks_equal_the_mapped_form(backend, gt_map, src, dst):
    C = 2 if gt_map == 'polyp' else 3
    soft = case(3, C, src, dst, 2)[0].to(backend.dev)
    mask = raw_mask(3, dst[0], dst[1], 5 + dst[0]).to(backend.dev)
    mapped = polyp_map_mask(mask) if gt_map == 'polyp' else fundus_map_mask(mask, exclusive=gt_map == 'fundus_exclusive')
    assert tuple(mapped.shape) == (3, C) + dst
    want = SF.nhot_case_tail(soft, mapped, values=VALUES[C], want_extents=True, want_hard=True)
    same(SF.nhot_case_tail(soft, mask, gt_map=gt_map, values=VALUES[C], want_extents=True, want_hard=True), want)
    same(want, composed(soft, mapped, dst, VALUES[C]))
    if gt_map != 'polyp':                                                         # two channels suffice for fundus, one for polyp
        same(SF.nhot_case_tail(soft, mask[:, :2].contiguous(), gt_map=gt_map, values=VALUES[C], want_extents=True, want_hard=True), want)
    else:
        same(SF.nhot_case_tail(soft, mask[:, :1].contiguous(), gt_map=gt_map, values=VALUES[C], want_extents=True, want_hard=True), want)
    if gt_map == 'fundus_exclusive' and dst[0] * dst[1] > 100:
        plain = SF.nhot_case_tail(soft, mask, gt_map='fundus')[0]
        assert not torch.equal(plain.cpu(), want[0].cpu())                        # the exclusive disc is smaller


@pytest.mark.parametrize('kind0', [1, 3])
@pytest.mark.parametrize('src,dst', [((41, 50), (41, 50)), ((8, 40), (25, 41))])
def test_vcdr_from_extents_equals_calc_vcdr_of_each_map(backend, src, dst, kind0):
    soft, gt = (t.to(backend.dev) for t in case(3, 3, src, dst, kind0))
    _, ext, _, hard = SF.nhot_case_tail(soft, gt, want_extents=True, want_hard=True)
    vp, vg = infer2d.vcdr_from_extents(ext)
    assert vp.dtype == torch.float32 and vg.dtype == torch.float32 and tuple(vp.shape) == (3,) and tuple(vg.shape) == (3,)
    assert torch.equal(infer2d.vcdr_from_extents(ext[:, 1]), vg)
    for i in range(3):
        assert torch.equal(vp[i], infer2d.calc_vcdr(hard[i])) and torch.equal(vg[i], infer2d.calc_vcdr(gt[i]))
    if kind0 == 1:                                                                # no-disc, no-cup, row0
        assert vg[0] == -1. and vg[1] == 0. and vp[0] == -1. and vp[1] == 0.
    with pytest.raises(ValueError, match='row extents'):
        infer2d.vcdr_from_extents(ext[0, 0, 0])


@pytest.mark.parametrize('src,dst', [((32, 32), (32, 32)), ((16, 24), (7, 5)), ((41, 50), (41, 50))])
def test_a_subset_of_the_outputs_has_the_same_values(backend, src, dst):
    B, C = 3, 3
    soft, gt = (t.to(backend.dev) for t in case(B, C, src, dst, 4))
    full = SF.nhot_case_tail(soft, gt, values=VALUES[C], want_extents=True, want_hard=True)
    counts, ext, labels, hard = SF.nhot_case_tail(soft, gt)
    assert (ext, labels, hard) == (None, None, None) and torch.equal(counts, full[0])
    counts, ext, labels, hard = SF.nhot_case_tail(soft, size=dst, values=VALUES[C])
    assert (counts, ext, hard) == (None, None, None) and torch.equal(labels, full[2])
    counts, ext, labels, hard = SF.nhot_case_tail(soft, size=dst, want_hard=True)
    assert (counts, ext, labels) == (None, None, None) and torch.equal(hard, full[3])
    # the library's own call: the extents alone, and the counts alone
    L, table = backend.L, torch.tensor(VALUES[C], dtype=torch.int32)
    e = torch.full((B, 2, 2, 2), 77, dtype=torch.int32)
    L.nhot_case_tail(soft, gt, 0, C, None, None, e, None, None, B, C, src[0], src[1], dst[0], dst[1])
    assert torch.equal(e, full[1])
    c, l = torch.full((B, C - 1, 3), 77, dtype=torch.int32), torch.full((B,) + dst, 77, dtype=torch.uint8)
    L.nhot_case_tail(soft, gt, 0, C, table, c, None, l, None, B, C, src[0], src[1], dst[0], dst[1])
    assert torch.equal(c, full[0]) and torch.equal(l, full[2])


def test_preallocated_outputs_are_written_and_initialised_by_every_call(backend):
    B, C, src, dst = 3, 3, (8, 40), (25, 41)
    soft, gt = (t.to(backend.dev) for t in case(B, C, src, dst, 0))
    counts, ext = torch.full((B, C - 1, 3), 12345, dtype=torch.int32), torch.full((B, 2, 2, 2), 12345, dtype=torch.int32)
    labels, hard = torch.full((B,) + dst, 9, dtype=torch.uint8), torch.full((B, C) + dst, 9.0)
    got = SF.nhot_case_tail(soft, gt, values=VALUES[C], counts=counts, ext=ext, labels=labels, hard=hard)
    assert got[0] is counts and got[1] is ext and got[2] is labels and got[3] is hard
    same(got, composed(soft, gt, dst, VALUES[C]))
    soft2, gt2 = (t.to(backend.dev) for t in case(B, C, src, dst, 2))              # other data into the same buffers: nothing of the first call is left
    SF.nhot_case_tail(soft2, gt2, values=VALUES[C], counts=counts, ext=ext, labels=labels, hard=hard)
    same((counts, ext, labels, hard), composed(soft2, gt2, dst, VALUES[C]))
    SF.nhot_case_tail(torch.zeros_like(soft), torch.zeros_like(gt), counts=counts, ext=ext)
    assert not counts.any() and ext[..., 0].eq(dst[0]).all() and ext[..., 1].eq(-1).all()


def test_another_threshold(backend):
    src, dst = (5, 7), (9, 13)
    soft, gt = (t.to(backend.dev) for t in case(3, 3, src, dst, 0))
    got = SF.nhot_case_tail(soft, gt, values=VALUES[3], T=0.625, want_extents=True, want_hard=True)
    same(got, composed(soft, gt, dst, VALUES[3], 0.625))
    assert not torch.equal(got[3], SF.nhot_case_tail(soft, gt, want_hard=True)[3])


def test_refusals(backend):
    L = backend.L
    B, C, (h, w), (H, W) = 2, 3, (4, 6), (5, 7)
    soft, gt = torch.rand(B, C, h, w), torch.zeros(B, C, H, W)
    mask = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    table = torch.tensor(VALUES[3], dtype=torch.int32)
    counts, ext = torch.zeros(B, C - 1, 3, dtype=torch.int32), torch.zeros(B, 2, 2, 2, dtype=torch.int32)
    labels, hard = torch.zeros(B, H, W, dtype=torch.uint8), torch.zeros(B, C, H, W)

    def call(soft=soft, gt=gt, gt_map=0, Cm=C, table=table, counts=counts, ext=ext, labels=labels, hard=hard, B=B, C=C, h=h, w=w, H=H, W=W):
        L.nhot_case_tail(soft, gt, gt_map, Cm, table, counts, ext, labels, hard, B, C, h, w, H, W)
    call()
    for kw, msg in [(dict(soft=None), 'null soft'), (dict(counts=None, ext=None, labels=None, hard=None), 'none of counts, ext, labels and hard'),
                    (dict(gt=None, ext=None), 'counts need the ground truth'), (dict(gt=None, counts=None), 'extents need the ground truth'),
                    (dict(table=None), 'labels need the value table'), (dict(B=0), 'B = 0'), (dict(B=65536), 'B = 65536'), (dict(C=1), 'C = 1'),
                    (dict(C=segx.SegxLib.MAX_CLASSES + 1), 'C = %d' % (segx.SegxLib.MAX_CLASSES + 1)), (dict(h=0), 'source size'), (dict(w=-1), 'source size'),
                    (dict(H=0), 'H \\* W'), (dict(W=0), 'H \\* W'), (dict(H=1 << 16, W=1 << 15), 'H \\* W'), (dict(gt_map=4), 'gt_map 4'), (dict(gt_map=-1), 'gt_map -1'),
                    (dict(gt=mask, gt_map=1, Cm=1), 'fundus mask'), (dict(gt=mask, gt_map=2, Cm=3, C=2), 'fundus mask'), (dict(gt=mask, gt_map=3, Cm=3), 'polyp mask'),
                    (dict(gt=mask, gt_map=3, Cm=0, C=2), 'polyp mask')]:
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    # the wrapper's own
    for kw, exc, msg in [(dict(gt=gt[:, :2]), ValueError, 'n-hot gt'), (dict(gt=gt[:1]), ValueError, 'is no \\['), (dict(gt=gt, size=(H, W + 1)), ValueError, 'is no \\['),
                         (dict(gt=mask, gt_map='polyp'), ValueError, 'raw polyp mask'), (dict(gt=gt, gt_map='fundus'), ValueError, 'raw fundus mask'),
                         (dict(gt=gt, gt_map='retina'), ValueError, 'gt_map'), (dict(), ValueError, 'no gt and no size'), (dict(size=(H, W)), ValueError, 'nothing to compute'),
                         (dict(size=(H, W), want_extents=True), ValueError, 'need gt'), (dict(size=(H, W), counts=counts), ValueError, 'need gt'),
                         (dict(size=(H, W), labels=labels), ValueError, 'labels need values'), (dict(gt=gt, values=(0, 255)), ValueError, '2 values for 3'),
                         (dict(gt=gt, values=(0, 1, 256)), ValueError, 'uint8 value'), (dict(gt=gt, counts=counts.view(-1)), ValueError, 'counts is a contiguous int32'),
                         (dict(gt=gt, values=VALUES[3], labels=labels.int()), ValueError, 'labels is a contiguous uint8'),
                         (dict(gt=gt, hard=hard[:, :, :-1]), ValueError, 'hard is a contiguous float32')]:
        with pytest.raises(exc, match=msg):
            SF.nhot_case_tail(soft, **kw)
    with pytest.raises(ValueError, match='float32 \\[B, C, h, w\\]'):
        SF.nhot_case_tail(soft[0], gt)
    with pytest.raises(ValueError, match='float32 \\[B, C, h, w\\]'):
        SF.nhot_case_tail(soft.double(), gt)
    with pytest.raises(ValueError, match='classes'):
        SF.nhot_case_tail(soft[:, :1], gt[:, :1])
    with torch.enable_grad(), pytest.raises(RuntimeError, match='forward-only'):
        SF.nhot_case_tail(soft.clone().requires_grad_(True), gt)
