"""The tail of the 2-D evaluation (components.hip: segx_ccl2d, segx_frag_keep2, segx_frag_apply, segx_row_extent, segx_nhot_to_values; infer2d.remove_fragmentary_segs /
calc_vcdr / calc_batch_metric, datasets2d.*_inv_map_mask, infer2d.export_masks) on the fiber emulator (CPU) and on the GPU (-m gpu), against

  * tests/golden/fragments2d.npz -- what the reference's own functions return (tests/golden/make_fragments_golden.py; cv2.connectedComponents served by
    scipy.ndimage.label there, scipy is not imported here), and
  * a torch referee written independently of both (tests/fragments_referee.py): labels start as 1 + raster index on set pixels and take the minimum over the set 3 x 3 neighbourhood until
    nothing changes; sizes by bincount; the two labels to keep by sorting (count descending, label ascending).

Everything is integers (or the reference's own float32 scalar arithmetic) and must be EQUAL; only the Dice columns carry a tolerance (that of test_oracle_golden)."""
import functools
import os

import numpy as np
import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer2d, segx
from segtran_amd import test_util2d as T2
from segtran_amd.dataloaders import datasets2d as D2
from fragments_referee import ref_keep, ref_labels, ref_remove

TH, TW = segx.SegxLib.CCL_TILE
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fragments2d.npz'))
FRAG_CASES = ('fundus', 'polyp', 'twofg', 'small')


def gold(key, dev=None):
    t = torch.from_numpy(GOLD[key])
    return t if dev is None else t.to(dev)


# ---- patterns: the smallest shapes at which each mechanism can fail --------------------------------------------------------------------------------------------
def seam_planes():
    """uint8 [12, 2 TH + 1, 2 TW + 2]: four tile rows / columns with a seam of each kind, a last tile row of one row and a last tile column of two columns"""
    H, W = 2 * TH + 1, 2 * TW + 2
    g = torch.Generator().manual_seed(7)
    z = lambda: torch.zeros(H, W, dtype=torch.uint8, device='cpu')
    planes = []
    a = z(); a[10, TW - 5:TW + 5] = 1; a[12, 2 * TW - 1:2 * TW + 2] = 1; a[20, 3:9] = 1; planes.append(a)               # joined only across a vertical seam (both seams)
    a = z(); a[TH - 4:TH + 4, 10] = 1; a[2 * TH - 2:2 * TH + 1, 70] = 1; a[5:9, 40] = 1; planes.append(a)               # only across a horizontal seam (both seams)
    a = z()                                                                                                          # only through the NW-SE corner diagonal
    for k in range(3):
        a[TH - 1 - k, TW - 1 - k] = 1; a[TH + k, TW + k] = 1
    a[2 * TH - 1, 2 * TW - 1] = 1; a[2 * TH, 2 * TW] = 1; planes.append(a)
    a = z()                                                                                                          # only through the NE-SW corner diagonal
    for k in range(3):
        a[TH - 1 - k, TW + k] = 1; a[TH + k, TW - 1 - k] = 1
    a[2 * TH - 1, 2 * TW] = 1; a[2 * TH, 2 * TW - 1] = 1; planes.append(a)
    a = z()                                                                                                          # a rectangular spiral inside tile (0, 0)
    y0, x0, y1, x1 = 0, 0, TH - 1, TW - 1
    while y1 - y0 >= 2 and x1 - x0 >= 2:
        a[y0, x0:x1 + 1] = 1; a[y0:y1 + 1, x1] = 1; a[y1, x0 + 2:x1 + 1] = 1; a[y0 + 2:y1 + 1, x0 + 2] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        if y1 > y0:
            a[y0, x0] = 1
    planes.append(a)
    a = z(); a[1:TH - 1, TW + 1:2 * TW - 1:2] = 1; a[TH - 2, TW + 1:2 * TW - 1] = 1; planes.append(a)                   # a comb inside tile (0, 1): teeth joined at the bottom
    a = z()                                                                                                          # a snake over the first vertical seam, five crossings
    rows = [2, 6, 10, 14, 18]
    for i, r in enumerate(rows):
        a[r, TW - 4:TW + 4] = 1
        if i + 1 < len(rows):
            a[r:rows[i + 1] + 1, TW + 3 if i % 2 == 0 else TW - 4] = 1
    planes.append(a)
    yy, xx = torch.meshgrid(torch.arange(H, device='cpu'), torch.arange(W, device='cpu'), indexing='ij')
    planes.append(((yy + xx) % 2 == 0).to(torch.uint8))                                                              # checkerboard: one 8-connected component
    planes.append(torch.ones(H, W, dtype=torch.uint8, device='cpu'))
    planes.append(z())
    planes.append((torch.rand(H, W, generator=g, device='cpu') < 0.3).to(torch.uint8))                               # 30 % speckle
    planes.append((torch.rand(H, W, generator=g, device='cpu') < 0.55).to(torch.uint8))                              # denser: components that wander over all tiles
    return torch.stack(planes)


def small_planes(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    return torch.stack([(torch.rand(H, W, generator=g, device='cpu') < 0.5).to(torch.uint8), torch.ones(H, W, dtype=torch.uint8, device='cpu'),
                        torch.zeros(H, W, dtype=torch.uint8, device='cpu')])


SHAPES = {'1x1': (1, 1), 'row': (1, TW + 6), 'column': (TH + 6, 1), 'tile-1': (TH - 1, TW - 1), 'tile': (TH, TW), 'seams': None}


@functools.lru_cache(None)
def case(name):
    """(planes uint8 [P, H, W], referee labels, referee sizes) on the CPU, computed once and shared"""
    with torch.device('cpu'):
        m = seam_planes() if name == 'seams' else small_planes(*SHAPES[name])
        return (m,) + ref_labels(m != 0)


def test_referee_and_fixture_agree():
    """the scipy stand-in behind the fixture and the referee say the same on every fragment case; and the referee knows a component when it sees one"""
    with torch.device('cpu'):
        for c in FRAG_CASES:
            seg, bg = gold('frag_%s_in' % c), int(GOLD['frag_%s_bg' % c])
            assert torch.equal(ref_remove(seg[None], bg)[0], gold('frag_%s_out' % c)), c
        m, labels, sizes = case('seams')
        ncomp = [int((sizes[p] > 0).sum()) for p in range(m.shape[0])]
        assert ncomp[:10] == [3, 3, 2, 2, 1, 1, 1, 1, 1, 0] and int(sizes[8].max()) == m.shape[1] * m.shape[2]


# ---- labelling ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SHAPES))
def test_label_components(backend, name):
    m, labels_ref, sizes_ref = case(name)
    labels, sizes = SF.label_components(m.to(backend.dev))
    assert labels.dtype == sizes.dtype == torch.int32 and labels.shape == sizes.shape == m.shape
    assert torch.equal(labels.cpu(), labels_ref)
    assert torch.equal(sizes.cpu(), sizes_ref)
    first = labels_ref == torch.arange(1, m[0].numel() + 1, dtype=torch.int32, device='cpu').view(1, *m.shape[1:])
    assert not sizes.cpu()[~first].any()                                               # counts sit on first pixels only
    for p in (0, m.shape[0] - 1):                                                       # a plane alone gives what it gives inside the stack
        l1, s1 = SF.label_components(m[p].to(backend.dev))
        assert l1.shape == m.shape[1:] and torch.equal(l1.cpu(), labels_ref[p]) and torch.equal(s1.cpu(), sizes_ref[p])
    lb, sb = SF.label_components((m != 0).to(backend.dev))                              # bool masks; another background value
    assert torch.equal(lb.cpu(), labels_ref) and torch.equal(sb.cpu(), sizes_ref)
    l7, _ = SF.label_components(torch.where(m != 0, 3, 7).to(torch.uint8).to(backend.dev), bg_value=7)
    assert torch.equal(l7.cpu(), labels_ref)


def test_keep_rule(backend):
    """segx_frag_keep2 against the sorted candidates, on planes with many components, with ties, with one candidate and with none but the background"""
    m, _, sizes_ref = case('seams')
    L = backend.L
    keep = torch.empty(m.shape[0], 2, dtype=torch.int32, device=backend.dev)
    L.frag_keep2(sizes_ref.to(backend.dev), keep, m.shape[0], m.shape[1], m.shape[2])
    assert torch.equal(keep.cpu(), ref_keep(sizes_ref))
    assert keep.cpu()[8].tolist() == [1, -1] and keep.cpu()[9].tolist() == [0, -1]      # all set: the one component; empty: the background alone
    sz = torch.zeros(1, 2, 5, dtype=torch.int32, device=backend.dev)                  # 10 pixels: components of 3 (label 9), 3 (label 2) and 2; background 2
    sz[0, 1, 3], sz[0, 0, 1], sz[0, 0, 4] = 3, 3, 2
    k1 = torch.empty(1, 2, dtype=torch.int32, device=backend.dev)
    L.frag_keep2(sz, k1, 1, 2, 5)
    assert k1.cpu().tolist() == [[2, 9]]                                                # equal counts: the lower label first
    sz[0, 1, 3] = 2                                                                     # now 3, 2, 2: the background holds 10 - 7 = 3 and ties with label 2
    L.frag_keep2(sz, k1, 1, 2, 5)
    assert k1.cpu().tolist() == [[0, 2]]                                                # a tie between the background and a component: the background first


# ---- fragment removal -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', FRAG_CASES)
def test_remove_fragmentary_segs_fixture(backend, c):
    seg, bg = gold('frag_%s_in' % c, backend.dev), int(GOLD['frag_%s_bg' % c])
    before = seg.clone()
    out = infer2d.remove_fragmentary_segs(seg, bg)
    assert out.dtype == torch.uint8 and out.shape == seg.shape and out.device == seg.device
    assert torch.equal(out.cpu(), gold('frag_%s_out' % c))                             # the real reference
    assert torch.equal(seg, before) and out.data_ptr() != seg.data_ptr()               # a new tensor; the input is not modified
    out3 = infer2d.remove_fragmentary_segs(seg[None], bg)                                   # [H, W] versus [1, H, W]
    assert out3.shape == (1,) + tuple(seg.shape) and torch.equal(out3[0], out)


def test_remove_fragments_outside_the_reference_domain(backend):
    dev = backend.dev
    H, W = TH + 3, TW + 5
    allbg = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    assert torch.equal(infer2d.remove_fragmentary_segs(allbg, 255), allbg)                  # all background: unchanged
    allfg = torch.full((H, W), 128, dtype=torch.uint8, device=dev); allfg[TH:, :] = 0
    assert torch.equal(infer2d.remove_fragmentary_segs(allfg, 255), allfg)                  # all foreground (one component of two values): unchanged
    tie = torch.zeros(6, TW + 8, dtype=torch.uint8, device=dev)                        # background 0 is the largest; two components of 4 pixels tie for the second place
    tie[1, TW - 2:TW + 2] = 9; tie[4, 2:6] = 5; tie[3, TW + 6] = 9
    want = tie.clone(); want[4, 2:6] = 0; want[3, TW + 6] = 0                          # the one that starts first in raster order stays
    assert torch.equal(infer2d.remove_fragmentary_segs(tie, 0), want)
    stack = torch.stack([tie, want, torch.zeros_like(tie)])                            # planes are cleaned on their own
    out = infer2d.remove_fragmentary_segs(stack, 0)
    assert torch.equal(out, torch.stack([want, want, torch.zeros_like(tie)]))
    with torch.device('cpu'):
        assert torch.equal(out.cpu(), ref_remove(stack.cpu(), 0))
    m = case('seams')[0]                                                               # and the referee on every pattern plane, with label values 1 -> 200
    seg = (m * 200).to(dev)
    with torch.device('cpu'):
        want = ref_remove(seg.cpu(), 0)
    assert torch.equal(infer2d.remove_fragmentary_segs(seg, 0).cpu(), want)


# ---- row extents and vCDR -------------------------------------------------------------------------------------------------------------------------------------
def test_row_extent(backend):
    dev = backend.dev
    H, W = 2 * 32 + 5, 64 + 7                                                          # three row groups of a workgroup; a second, partial sweep of the row
    m = torch.zeros(6, H, W, device=dev)
    m[0, 3, W - 1] = 0.5; m[0, 40, 0] = 0.7; m[0, 50, 5] = 0.49                        # >= thres counts, below does not
    m[1, H - 1, 64] = 1.0                                                              # the last row, a column of the second sweep
    m[2, 0, 0] = 2.0
    m[3] = 1.0
    m[4, 10, 10] = float('nan')                                                        # a NaN is below every threshold
    ext = SF.row_extent(m, 0.5)
    assert ext.dtype == torch.int32 and ext.cpu().tolist() == [[3, 40], [H - 1, H - 1], [0, 0], [0, H - 1], [H, -1], [H, -1]]
    assert SF.row_extent(m[0], 0.5).cpu().tolist() == [3, 40]
    assert SF.row_extent(m, 0.49).cpu()[0].tolist() == [3, 50]
    rows = SF.row_extent(m[0].reshape(H, 1, W), 0.5).cpu()                             # planes of one row: (0, 0) occupied, (1, -1) not
    assert rows[:, 1].eq(0).nonzero().view(-1).tolist() == [3, 40]
    want = (m.cpu() >= 0.5).any(dim=2)
    for p in range(6):
        occ = want[p].nonzero().view(-1)
        assert ext.cpu()[p].tolist() == ([int(occ.min()), int(occ.max())] if occ.numel() else [H, -1])


@pytest.mark.parametrize('name', ['normal', 'hard', 'nodisc', 'nocup', 'lastrow', 'batch'])
def test_calc_vcdr(backend, name):
    m = gold('vcdr_%s_in' % name, backend.dev)
    for delta in (0, 1):
        v = infer2d.calc_vcdr(m, delta=delta)
        want = gold('vcdr_%s_d%d' % (name, delta))
        assert v.dtype == want.dtype == torch.float32 and v.shape == want.shape
        assert torch.equal(v.cpu(), want), (name, delta, v, want)
    if name == 'hard':
        assert abs(infer2d.calc_vcdr(m).cpu().item() - 0.3) < 1e-4                              # disc rows 3..14, cup rows 6..10: tensor(0.3000)
    if name == 'batch':
        assert GOLD['vcdr_batch_d1'].shape == (5,)
        assert torch.equal(infer2d.calc_vcdr(m, thres=0.75).cpu(), infer2d.calc_vcdr((m >= 0.75).float()).cpu())


def _metric_inputs(dev):
    return [gold('metric_pred%d' % i, dev) for i in range(2)], [gold('metric_gt%d' % i, dev) for i in range(2)]


def test_calc_batch_metric_vcdr_column(backend):
    preds, gts = _metric_inputs(backend.dev)
    table = GOLD['metric_table']
    got = infer2d.calc_batch_metric(preds, gts, 3, do_calc_vcdr_error=True)
    assert got.shape == (2, 3) and got.dtype == np.float64
    assert np.abs(got[:, :2] - table[:, :2]).max() <= 1e-6 * np.abs(table[:, :2]).max()      # the bar test_oracle_golden holds calc_dice to
    assert np.array_equal(got[:, 2], table[:, 2])                                            # exact
    plain = infer2d.calc_batch_metric(preds, gts, 3)                                              # the default call: what it returned before the column existed
    want = np.zeros((2, 2))
    for i in range(2):
        hard = D2.harden_segmap2d(preds[i])
        want[i] = SF.dice_scores(hard[1:].float().reshape(2, -1), gts[i][1:].float().reshape(2, -1)).cpu().numpy()
    assert plain.shape == (2, 2) and np.array_equal(plain, want) and np.array_equal(plain, got[:, :2])
    assert np.array_equal(plain, T2.calc_batch_metric(preds, gts, 3))                        # test_util2d's function is the default, as it was


class _FixedNet:
    """stands for a network: the scores whose sigmoid is the fixture's soft prediction, whatever the patch"""

    def __init__(self, soft):
        self.scores = torch.logit(soft.clamp(1e-4, 1 - 1e-4))[None]

    def __call__(self, patch):
        return self.scores


def test_all_cases_vcdr_flag(backend):
    preds, gts = _metric_inputs(backend.dev)
    shape = tuple(preds[0].shape[1:])
    net = _FixedNet(preds[0])
    batches = [(torch.zeros(1, 3, *shape, device=backend.dev), gts[0][None])]
    for mod in (T2, infer2d):
        avg0, n0 = mod.test_all_cases(net, batches, 'fundus', 3, shape, shape, shape)
        assert avg0.shape == (2,) and n0 == 1                                              # the default: untouched
    avg, n = infer2d.test_all_cases(net, batches, 'fundus', 3, shape, shape, shape, do_calc_vcdr_error=True)
    assert avg.shape == (3,) and np.array_equal(n, np.ones(3))                              # vectors of num_classes entries, as the reference
    assert np.array_equal(avg[:2], avg0) and avg[2] == GOLD['metric_table'][0, 2]


# ---- inverse maps and export ------------------------------------------------------------------------------------------------------------------------------------
def test_inverse_maps(backend):
    dev = backend.dev
    f = D2.fundus_inv_map_mask(gold('inv_fundus_in', dev))
    assert f.dtype == torch.uint8 and torch.equal(f.cpu(), gold('inv_fundus_out'))
    assert f.cpu()[0, 0, :4].tolist() == [128, 0, 0, 0]                                 # bg + disc -> disc; bg + cup -> cup; nothing on -> 0; all on -> cup
    f3 = D2.fundus_inv_map_mask(gold('inv_fundus3_in', dev))
    assert f3.dtype == torch.uint8 and torch.equal(f3.cpu(), gold('inv_fundus3_out'))
    p = D2.polyp_inv_map_mask(gold('inv_polyp_in', dev))
    assert p.dtype == torch.uint8 and torch.equal(p.cpu(), gold('inv_polyp_out'))
    assert torch.equal(D2.polyp_inv_map_mask(gold('inv_polyp_in', dev)[1]).cpu(), gold('inv_polyp_out')[1])
    assert torch.equal(D2.fundus_inv_map_mask(gold('inv_fundus_in', dev).int()).cpu(), gold('inv_fundus_out'))      # hardened maps are int32
    v = SF.nhot_to_values(gold('inv_fundus_in', dev), (1, 2, 3))
    assert sorted(v.unique().cpu().tolist()) == [0, 1, 2, 3]


def test_export_masks(backend):
    dev = backend.dev
    preds, _ = _metric_inputs(dev)
    sizes = [(2 * TH + 3, TW + 9), tuple(preds[1].shape[1:])]                          # one resampled over tile seams, one at its own size
    for inv, bg in ((D2.fundus_inv_map_mask, 255), (D2.polyp_inv_map_mask, 0)):
        soft = [p if inv is D2.fundus_inv_map_mask else p[:2] for p in preds]
        plain = infer2d.export_masks(soft, sizes, inv)
        clean = infer2d.export_masks(soft, sizes, inv, remove_frag=True, bg_value=bg)
        for i in range(2):
            s = soft[i][None].contiguous()
            if tuple(s.shape[2:]) != sizes[i]:
                s = SF.interp_linear(s, sizes[i])
            want = inv(D2.harden_segmap2d(s[0]))
            assert plain[i].dtype == torch.uint8 and tuple(plain[i].shape) == sizes[i] and torch.equal(plain[i], want)
            assert torch.equal(clean[i], infer2d.remove_fragmentary_segs(want, bg))
    with pytest.raises(ValueError, match='sizes'):
        infer2d.export_masks(preds, sizes[:1], D2.fundus_inv_map_mask)


def test_constants_match_header():
    """the tile the seam patterns (and the fixture generator) are laid out by, and the plane limit the wrappers refuse at, are the header's"""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'segx.h')).read()
    d = {k: int(v, 0) for k, v in re.findall(r'#define\s+(SEGX_CCL_\w+)\s+(\w+)', hdr)}
    assert (d['SEGX_CCL_TILE_H'], d['SEGX_CCL_TILE_W']) == tuple(segx.SegxLib.CCL_TILE) == (TH, TW)
    assert d['SEGX_CCL_MAX_PLANE'] == segx.SegxLib.CCL_MAX_PLANE == 1 << 30


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    dev, L = backend.dev, backend.L
    seg = torch.zeros(4, 5, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match='uint8'):
        infer2d.remove_fragmentary_segs(seg.int(), 0)
    with pytest.raises(TypeError, match='uint8'):
        infer2d.remove_fragmentary_segs(seg.cpu().numpy(), 0)
    with pytest.raises(TypeError):
        SF.label_components(seg.float())
    with pytest.raises(TypeError):
        SF.row_extent(seg, 0.5)
    with pytest.raises(ValueError, match='rank'):
        SF.remove_fragments(seg[None, None], 0)
    with pytest.raises(ValueError, match='uint8 value'):
        SF.remove_fragments(seg, 256)
    side = 1 << 15                                                                     # H * W = 2^30: the first plane size refused; nothing of that size is allocated
    huge = torch.zeros(1, dtype=torch.uint8, device=dev).expand(side, side)
    with pytest.raises(ValueError, match='2\\^30'):
        SF.remove_fragments(huge, 0)
    with pytest.raises(ValueError, match='2\\^30'):
        SF.label_components(huge)
    i32 = torch.zeros(4, 5, dtype=torch.int32, device=dev)
    keep = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match='2\\^30'):
        L.ccl2d(seg, 0, i32, i32.clone(), 1, side, side)
    with pytest.raises(RuntimeError, match='2\\^30'):
        L.frag_keep2(i32, keep, 1, side, side)
    with pytest.raises(RuntimeError, match='2\\^30'):
        L.frag_apply(seg, i32, keep, seg.clone(), 1, side, side, 0)
    with pytest.raises(RuntimeError, match='2\\^30'):
        L.row_extent(seg.float(), keep, 1, side, side, 0.5)
    L.ccl2d(seg, 0, i32, i32.clone(), 1, 4, 5)                                          # the same call inside the bound goes through
    with pytest.raises(RuntimeError, match='one grid'):                                # HIP takes at most 2^32 threads per grid axis: 2^24 tiles of 256 threads
        L.ccl2d(seg, 0, i32, i32.clone(), 1 << 24, 1, 1)
    with pytest.raises(RuntimeError, match='one grid'):                                # ... and 2^22 planes of 1024 threads
        L.frag_keep2(i32, keep, 1 << 22, 1, 1)
    with pytest.raises(RuntimeError, match='positive'):
        L.ccl2d(seg, 0, i32, i32.clone(), 1, 0, 5)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.frag_keep2(None, keep, 1, 4, 5)
    with pytest.raises(ValueError, match='values for'):
        SF.nhot_to_values(torch.zeros(1, 3, 2, 2, device=dev), (1, 2))
    with pytest.raises(ValueError, match='n-hot maps'):
        D2.fundus_inv_map_mask(torch.zeros(2, 4, 4, device=dev))
    with pytest.raises(ValueError, match='rank'):
        infer2d.calc_vcdr(torch.zeros(4, 4, device=dev))
    g = torch.zeros(1, 4, 5, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match='forward-only'):
        SF.row_extent(g, 0.5)


def test_product_library_refuses_cpu_tensors():
    from segtran_amd.build import build
    segx.use_library(segx.SegxLib(build()))
    try:
        seg = torch.zeros(4, 5, dtype=torch.uint8, device='cpu')
        for call in (lambda: infer2d.remove_fragmentary_segs(seg, 0), lambda: SF.label_components(seg), lambda: SF.row_extent(seg.float(), 0.5),
                     lambda: infer2d.calc_vcdr(torch.zeros(3, 4, 5, device='cpu')), lambda: D2.polyp_inv_map_mask(torch.zeros(2, 4, 5, device='cpu'))):
            with pytest.raises(RuntimeError, match='CPU tensor'):
                call()
    finally:
        segx.use_library(None)
