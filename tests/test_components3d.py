"""Connected-component post-processing of 3-D predictions (components.hip: segx_ccl3d, segx_cc3d_keep, segx_mask_apply, segx_brats_postprocess, segx_brats_relabel;
SF.label_components3d / keep_components3d / remove_small_components3d / brats_postprocess / brats_relabel; infer3d.connected_components / remove_small_components /
postprocess_brats and the `postprocess=` argument) on the fiber emulator (CPU) and on the GPU (-m gpu), against the torch referee of tests/components3d_referee.py,
which is written independently of the kernels.  Everything is integers or 0 / 1 floats and must be EQUAL.

The volumes are a few tiles: T = (TX, TY, TZ) = SEGX_CCL3_TILE_X / _Y / _Z, and every pattern is placed by them."""
import functools
import os
import re

import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer3d, segx
from components3d_referee import ref_brats, ref_keep3d, ref_labels3d, ref_remove3d

TX, TY, TZ = segx.SegxLib.CCL3_TILE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def zeros(*shape):
    return torch.zeros(*shape, dtype=torch.uint8, device='cpu')


# ---- patterns -------------------------------------------------------------------------------------------------------------------------------------------------
def corner_stack(shape):
    """[8, *shape]: a single voxel at each of the 8 corners"""
    X, Y, Z = shape
    m = zeros(8, X, Y, Z)
    for v in range(8):
        m[v, (X - 1) * (v >> 2 & 1), (Y - 1) * (v >> 1 & 1), (Z - 1) * (v & 1)] = 1
    return m


def pair_stack():
    """[3 + 6 + 4, 2 TX, 2 TY, 2 TZ]: two voxels that touch only across a seam -- a FACE in each of the three directions, a tile EDGE in both diagonals of each of the
    three orientations, and the tile CORNER in its four space diagonals.  (faces, edges, corners) index ranges"""
    c = (TX, TY, TZ)                                          # the first coordinate behind each seam
    vols = []
    for ax in range(3):                                       # face: straight across the seam of axis ax, away from the other seams
        a = [2, 3, 5]; b = list(a)
        a[ax], b[ax] = c[ax] - 1, c[ax]
        vols.append((a, b))
    for ax in range(3):                                       # edge running along ax: the pair differs in the two other coordinates
        o = [k for k in range(3) if k != ax]
        for flip in (0, 1):
            a = [1, 1, 1]; b = [1, 1, 1]
            a[o[0]], b[o[0]] = c[o[0]] - 1, c[o[0]]
            a[o[1]], b[o[1]] = (c[o[1]] - 1, c[o[1]]) if not flip else (c[o[1]], c[o[1]] - 1)
            vols.append((a, b))
    for f in range(4):                                        # corner: the four space diagonals through the point where the three seams meet
        a = [c[0] - 1, c[1] - 1 + (f & 1), c[2] - 1 + (f >> 1)]
        b = [c[0], c[1] - (f & 1), c[2] - (f >> 1)]
        vols.append((a, b))
    m = zeros(len(vols), 2 * TX, 2 * TY, 2 * TZ)
    for v, (a, b) in enumerate(vols):
        m[v][tuple(a)] = 1; m[v][tuple(b)] = 1
    return m, (range(0, 3), range(3, 9), range(9, 13))


def serpentine(axis):
    """one volume whose single component crosses the first seam of `axis` seven times: rods along `axis` over the seam, joined alternately at their ends"""
    ext = [2 * TX, 3, 3]
    if axis == 2:
        ext = [3, 3, 2 * TZ]
    other = 1 if axis == 2 else 2                             # the rods lie side by side along this axis, two apart
    ext[other] = 14
    m = zeros(1, *ext)
    seam = (TX, TY, TZ)[axis]
    for i in range(7):
        for t in range(seam - 3, seam + 3):
            p = [0, 0, 0]; p[axis] = t; p[other] = 2 * i
            m[0][tuple(p)] = 1
        if i < 6:
            p = [0, 0, 0]; p[axis] = seam + 2 if i % 2 == 0 else seam - 3; p[other] = 2 * i + 1
            m[0][tuple(p)] = 1
    return m


def spiral_plane(H, W):
    """the cells of a one-cell-wide rectangular spiral that fills an H x W plane without touching itself, not even diagonally: (path from the outside in)"""
    path, seen = [(0, 0)], {(0, 0)}
    dirs, d = [(0, 1), (1, 0), (0, -1), (-1, 0)], 0

    def free(c):
        if not (0 <= c[0] < H and 0 <= c[1] < W) or c in seen:
            return False
        near = {(c[0] + dy, c[1] + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)} & seen
        return near <= set(path[-2:])
    while True:
        for turn in (0, 1):
            dd = dirs[(d + turn) % 4]
            c = (path[-1][0] + dd[0], path[-1][1] + dd[1])
            if free(c):
                d = (d + turn) % 4
                path.append(c); seen.add(c)
                break
        else:
            return path


def spiral_tile():
    """[1, TX, TY, TZ]: the plane spiral in the (y, z) planes x = 0, 2, 4, ..., joined alternately at their inner and outer ends through the planes between: ONE
    one-voxel-wide path through the whole tile"""
    path = spiral_plane(TY, TZ)
    m = zeros(1, TX, TY, TZ)
    for x in range(0, TX, 2):
        for y, z in path:
            m[0, x, y, z] = 1
        if x + 2 < TX:
            y, z = path[-1] if (x // 2) % 2 == 0 else path[0]
            m[0, x + 1, y, z] = 1
    return m, len(path)


def random_stack(density, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(2, 2 * TX, 2 * TY, 2 * TZ, generator=g, device='cpu') < density).to(torch.uint8)


def touching_stack():
    """[2, TX + 1, 3, TZ + 2]: a component of the first volume ends on its last voxel, one of the second starts on its first: neighbours in memory, not in space"""
    m = zeros(2, TX + 1, 3, TZ + 2)
    m[0, TX, 2, TZ - 1:] = 1
    m[1, 0, 0, :4] = 1
    return m


PARTIAL = (TX + 3, 2 * TY + 1, TZ + 5)                        # every axis has a partial last tile
CASES = {
    'empty': lambda: zeros(1, *PARTIAL),
    'full': lambda: zeros(1, *PARTIAL) + 1,
    'corners': lambda: corner_stack(PARTIAL),
    'partial-random': lambda: (torch.rand(2, *PARTIAL, generator=torch.Generator().manual_seed(5), device='cpu') < 0.35).to(torch.uint8),
    'one-voxel': lambda: zeros(1, 1, 1, 1) + 1,
    'stack': touching_stack,
    'pairs': lambda: pair_stack()[0],
    'serpentine-x': lambda: serpentine(0),
    'serpentine-z': lambda: serpentine(2),
    'spiral': lambda: spiral_tile()[0],
    'random-0.1': lambda: random_stack(0.1, 1),
    'random-0.3': lambda: random_stack(0.3, 2),             # near the 26-connected percolation threshold: components that wander over all tiles
    'random-0.6': lambda: random_stack(0.6, 3),
}


@functools.lru_cache(None)
def case(name, connectivity):
    """(mask uint8 [V, X, Y, Z], referee labels, referee sizes) on the CPU, computed once and shared"""
    with torch.device('cpu'):
        m = CASES[name]()
        return (m,) + ref_labels3d(m != 0, connectivity)


def ncomp(sizes):
    return [int((s > 0).sum()) for s in sizes]


# ---- the referee and the patterns themselves --------------------------------------------------------------------------------------------------------------------
def test_patterns_are_what_they_claim():
    faces, edges, corners = pair_stack()[1]
    _, _, s26 = case('pairs', 26)
    _, _, s6 = case('pairs', 6)
    assert ncomp(s26) == [1] * 13 and all(int(s.max()) == 2 for s in s26)
    assert ncomp(s6) == [1] * 3 + [2] * 10                   # only the face pairs are 6-connected
    m, _, _ = case('pairs', 26)
    for v in range(13):                                       # the two voxels lie in different tiles
        a, b = m[v].nonzero().tolist()
        tiles = [(p[0] // TX, p[1] // TY, p[2] // TZ) for p in (a, b)]
        differ = sum(x != y for x, y in zip(*tiles))
        assert differ == (1 if v in faces else 2 if v in edges else 3), v
    for name in ('serpentine-x', 'serpentine-z'):
        m, _, s = case(name, 6)
        assert ncomp(s) == [1] and int(s.max()) == int(m.sum()) == 7 * 6 + 6
    m, n = spiral_tile()
    assert n > TY * TZ // 3                                   # the plane spiral fills its plane
    for conn in (6, 26):
        assert ncomp(case('spiral', conn)[2]) == [1] and int(case('spiral', conn)[2].max()) == int(m.sum()) == n * (TX // 2) + TX // 2 - 1
    assert ncomp(case('stack', 26)[2]) == [1, 1] and ncomp(case('corners', 26)[2]) == [1] * 8
    assert ncomp(case('full', 6)[2]) == [1] and ncomp(case('empty', 26)[2]) == [0]
    assert ncomp(case('random-0.3', 26)[2])[0] > 5 and ncomp(case('random-0.3', 6)[2])[0] > ncomp(case('random-0.3', 26)[2])[0]


def test_referee_agrees_with_scipy():
    """the referee's partition against scipy.ndimage.label with both structuring elements (labels differ by a renaming: compare first-voxel labels)"""
    ndimage = pytest.importorskip('scipy.ndimage')
    import numpy as np
    for name in ('random-0.3', 'partial-random', 'pairs', 'spiral'):
        for conn in (6, 26):
            m, labels, sizes = case(name, conn)
            for v in range(m.shape[0]):
                lab, n = ndimage.label(m[v].numpy(), structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
                assert n == int((sizes[v] > 0).sum())
                flat, mine = lab.reshape(-1), labels[v].reshape(-1).numpy()
                first = np.full(n + 1, flat.size, dtype=np.int64)
                np.minimum.at(first, flat, np.arange(flat.size))
                want = np.where(flat > 0, first[flat] + 1, 0)
                assert np.array_equal(want, mine), (name, conn, v)


# ---- labelling ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [26, 6])
@pytest.mark.parametrize('name', list(CASES))
def test_label_components3d(backend, name, connectivity):
    m, labels_ref, sizes_ref = case(name, connectivity)
    before = m.clone()
    labels, sizes = SF.label_components3d(m.to(backend.dev), connectivity)
    assert labels.dtype == sizes.dtype == torch.int32 and labels.shape == sizes.shape == m.shape
    assert torch.equal(labels.cpu(), labels_ref)
    assert torch.equal(sizes.cpu(), sizes_ref)
    first = labels_ref == torch.arange(1, m[0].numel() + 1, dtype=torch.int32, device='cpu').view(1, *m.shape[1:])
    assert not sizes.cpu()[~first].any()                      # counts sit on first voxels only
    assert torch.equal(m, before)


@pytest.mark.parametrize('name', ['partial-random', 'stack', 'pairs'])
def test_label_components3d_input_types(backend, name):
    """the float channel is read as it is (voxel != 0), bool and other float types too; a volume alone gives what it gives inside the stack"""
    m, labels_ref, sizes_ref = case(name, 26)
    dev = backend.dev
    for t in (m.float() * 1.0, m != 0, m.double(), m * 7):
        labels, sizes = SF.label_components3d(t.to(dev))
        assert torch.equal(labels.cpu(), labels_ref) and torch.equal(sizes.cpu(), sizes_ref), t.dtype
    for v in (0, m.shape[0] - 1):
        l1, s1 = SF.label_components3d(m[v].float().to(dev))
        assert l1.shape == m.shape[1:] and torch.equal(l1.cpu(), labels_ref[v]) and torch.equal(s1.cpu(), sizes_ref[v])
    ch = torch.stack([torch.zeros_like(m[0]), m[0]]).float().to(dev)         # one channel of a [C, H, W, D] prediction: a view at an offset
    l1, _ = SF.label_components3d(ch[1])
    assert torch.equal(l1.cpu(), labels_ref[0])


def test_other_float_types_are_set_where_they_are_not_zero(backend):
    """float64 / half / bfloat16 masks: set iff not 0 in the type itself -- a float64 below the float32 range is set --, and the cleaned mask keeps dtype and values"""
    m, labels_ref, sizes_ref = case('partial-random', 26)
    with torch.device('cpu'):
        want = ref_remove3d(m, min_voxels=3)
    for dtype, value in ((torch.float64, 1e-300), (torch.float16, 1e-7), (torch.bfloat16, 0.5), (torch.float64, -2.5)):
        t = (m.to(dtype) * value).to(backend.dev)
        assert int((t != 0).sum()) == int(m.sum()) and (dtype != torch.float64 or value < 0 or not t.float().any())
        labels, sizes = SF.label_components3d(t)
        assert torch.equal(labels.cpu(), labels_ref) and torch.equal(sizes.cpu(), sizes_ref), dtype
        out = SF.remove_small_components3d(t, min_voxels=3)
        assert out.dtype == dtype and out.shape == t.shape and torch.equal(out.cpu(), (want.to(dtype) * value)), dtype


# ---- keep rule ------------------------------------------------------------------------------------------------------------------------------------------------
def keep_stack():
    """[4, 3, 4, TZ + 8]: (0) components of 5, 5, 3 and 1 voxels, the two of 5 tie for largest; (1) 4 and 6 voxels, the later one is larger and crosses the z seam;
    (2) no foreground; (3) one voxel"""
    m = zeros(4, 3, 4, TZ + 8)
    m[0, 0, 0, 2:7] = 1; m[0, 2, 3, 10:15] = 1; m[0, 1, 2, 20:23] = 1; m[0, 2, 0, 0] = 1
    m[1, 0, 0, 0:4] = 1; m[1, 2, 2, TZ - 3:TZ + 3] = 1
    m[3, 1, 1, 1] = 1
    return m


@pytest.mark.parametrize('min_voxels,largest_only', [(0, False), (5, False), (6, False), (3, False), (4, False), (0, True), (5, True), (6, True), (7, True),
                                                     (1, True), (2, False)])
def test_keep_rule(backend, min_voxels, largest_only):
    m = keep_stack()
    with torch.device('cpu'):
        labels, sizes = ref_labels3d(m != 0, 26)
        want = ref_keep3d(labels, sizes, min_voxels, largest_only)
    keep = SF.keep_components3d(labels.to(backend.dev), sizes.to(backend.dev), min_voxels, largest_only)
    assert keep.dtype == torch.uint8 and torch.equal(keep.cpu(), want)
    kept = [sorted(set(labels[v][keep.cpu()[v] != 0].tolist())) for v in range(4)]
    five_a, five_b, three, one = int(labels[0, 0, 0, 2]), int(labels[0, 2, 3, 10]), int(labels[0, 1, 2, 20]), int(labels[0, 2, 0, 0])
    four, six = int(labels[1, 0, 0, 0]), int(labels[1, 2, 2, TZ])
    assert five_a < five_b and kept[2] == []                                  # a volume without foreground keeps nothing
    if largest_only:
        assert kept[0] == ([five_a] if min_voxels <= 5 else [])               # the tie: the earlier of the two equal components; above the largest size: nothing
        assert kept[1] == ([six] if min_voxels <= 6 else [])
        assert kept[3] == ([int(labels[3, 1, 1, 1])] if min_voxels <= 1 else [])
    else:
        assert kept[0] == sorted(l for l, n in ((five_a, 5), (five_b, 5), (three, 3), (one, 1)) if n >= min_voxels)    # size == min_voxels stays, one more goes
        assert kept[1] == sorted(l for l, n in ((four, 4), (six, 6)) if n >= min_voxels)
    out = SF.remove_small_components3d(m.to(backend.dev), min_voxels, largest_only)
    assert out.dtype == m.dtype and torch.equal(out.cpu(), m * want)
    with torch.device('cpu'):
        assert torch.equal(out.cpu(), ref_remove3d(m, min_voxels, largest_only))


@pytest.mark.parametrize('connectivity', [26, 6])
def test_remove_small_components3d(backend, connectivity):
    """on a random stack with many components, for every input type; a new tensor of the input's shape and dtype, the input untouched"""
    m, labels_ref, sizes_ref = case('random-0.1', connectivity)
    dev = backend.dev
    for t, kw in ((m, dict(min_voxels=3)), (m != 0, dict(largest_only=True)), (m.float(), dict(min_voxels=2, largest_only=True)), (m[1], dict(min_voxels=4))):
        x = t.to(dev)
        before = x.clone()
        out = SF.remove_small_components3d(x, connectivity=connectivity, **kw)
        with torch.device('cpu'):
            want = ref_remove3d(t if t.dim() == 4 else t[None], connectivity=connectivity, **kw)
        assert out.dtype == t.dtype and out.shape == t.shape and out.data_ptr() != x.data_ptr()
        assert torch.equal(out.cpu(), want if t.dim() == 4 else want[0]) and torch.equal(x, before)
        assert 0 < int((out != 0).sum()) < int((x != 0).sum())


# ---- BraTS rule -----------------------------------------------------------------------------------------------------------------------------------------------
SHAPE_B = (TX + 4, TY + 4, TZ + 8)
N_ET_MAIN, N_ET_SAT, N_SAT_A, N_SAT_B = 2 * 2 * 3, 2, 2 * 2 * 2, 3 * 2 * 3


def brats_case():
    """(hard float [4, *SHAPE_B], labels uint8): nested ET < TC < WT blobs over the tile seams, satellite A (WT alone, 8 voxels) and satellite B (18 voxels of WT, 2 of
    them ET and TC as well); the label volume a tail would write (4 = ET, 1 = TC, 2 = WT) with a few stray labels outside WT"""
    et, wt, tc = zeros(*SHAPE_B), zeros(*SHAPE_B), zeros(*SHAPE_B)
    wt[2:TX + 2, 2:TY + 2, TZ - 8:TZ + 4] = 1
    tc[4:TX, 4:TY, TZ - 4:TZ + 2] = 1
    et[5:7, 5:7, TZ - 1:TZ + 2] = 1
    wt[0:2, 0:2, 0:2] = 1                                                      # satellite A
    wt[TX + 1:TX + 4, 0:2, TZ + 5:TZ + 8] = 1                                  # satellite B
    et[TX + 2, 0, TZ + 5:TZ + 7] = 1; tc[TX + 2, 0, TZ + 5:TZ + 7] = 1
    tc[0, TY + 3, 0] = 1                                                       # a TC voxel outside WT: cut by rule 2
    assert int(et.sum()) == N_ET_MAIN + N_ET_SAT and int((et * wt).sum()) == int(et.sum())
    bg = ((et + wt + tc) == 0).to(torch.uint8)
    labels = torch.where(et != 0, 4, torch.where(tc != 0, 1, torch.where(wt != 0, 2, 0))).to(torch.uint8)
    labels[1, TY + 2, 3] = 2; labels[TX + 3, TY + 3, 0] = 4                    # the soft map's argmax need not agree with hard: labels outside WT
    return torch.stack([bg, et, wt, tc]).float(), labels


N_WT_MAIN = TX * TY * 12
BRATS_OPTIONS = [
    dict(),
    dict(wt_min_voxels=N_SAT_A),                    # satellite A is exactly that large: everything stays
    dict(wt_min_voxels=N_SAT_A + 1),                # A goes
    dict(wt_min_voxels=N_SAT_B + 1),                # A and B go, and the ET of B with it
    dict(wt_largest_only=True),
    dict(et_min_voxels=N_ET_MAIN + N_ET_SAT),       # exactly the count: kept
    dict(et_min_voxels=N_ET_MAIN + N_ET_SAT + 1),   # one more: dropped
    dict(connectivity=6),
    dict(wt_largest_only=True, et_min_voxels=N_ET_MAIN),                       # B's ET left with B: exactly N_ET_MAIN remain, kept
    dict(wt_largest_only=True, et_min_voxels=N_ET_MAIN + 1),                   # one fewer than asked: dropped, TC unchanged, labels 4 -> 1
    dict(wt_min_voxels=N_SAT_A + 1, wt_largest_only=True, et_min_voxels=N_ET_MAIN + 1, connectivity=6),
    dict(wt_min_voxels=N_WT_MAIN + 1, wt_largest_only=True),                   # above the largest size: no WT at all
]


@pytest.mark.parametrize('opts', BRATS_OPTIONS, ids=lambda o: ','.join('%s=%s' % kv for kv in o.items()) or 'defaults')
def test_brats_rule(backend, opts):
    hard, labels = brats_case()
    with torch.device('cpu'):
        want, want_labels, dropped = ref_brats(hard, labels, **opts)
    x, l = hard.to(backend.dev), labels.to(backend.dev)
    x0, l0 = x.clone(), l.clone()
    out, flag = SF.brats_postprocess(x, **opts)
    assert out.dtype == torch.float32 and out.shape == hard.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(out.cpu(), want)
    assert flag.cpu().tolist() == [int((hard[1] * want[2] != 0).sum()), int(dropped)]            # the count and the decision, on the device
    new = SF.brats_relabel(l, out, flag)
    assert torch.equal(new.cpu(), want_labels)
    assert torch.equal(x, x0) and torch.equal(l, l0)                                            # the inputs are not modified
    o = out.cpu()
    assert torch.equal(o[0], ((o[1] + o[2] + o[3]) == 0).float())                               # the background channel recomputed
    assert not new.cpu()[o[2] == 0].any()                                                       # labels' zero outside WT'
    assert not o[1][o[2] == 0].any() and not o[3][o[2] == 0].any()
    if dropped:
        assert not o[1].any() and torch.equal(o[3], hard[3] * o[2]) and not (new == 4).any()    # ET gone, TC unchanged, 4 -> 1
        assert torch.equal(new.cpu()[(labels == 4) & (o[2] != 0)], torch.ones(int(((labels == 4) & (o[2] != 0)).sum()), dtype=torch.uint8, device='cpu'))
    inplace = SF.brats_relabel(l, out, flag, out=l)                                             # a captured sequence rewrites its static volume
    assert inplace is l and torch.equal(l.cpu(), want_labels)


def test_brats_rule_expected_outcomes():
    """the referee's own results on the synthetic case are the ones the options were chosen for"""
    hard, labels = brats_case()
    with torch.device('cpu'):
        res = [ref_brats(hard, labels, **o) for o in BRATS_OPTIONS]
    wt = [int(r[0][2].sum()) for r in res]
    everything = N_WT_MAIN + N_SAT_A + N_SAT_B
    assert wt == [everything, everything, everything - N_SAT_A, N_WT_MAIN, N_WT_MAIN, everything, everything, everything, N_WT_MAIN, N_WT_MAIN, N_WT_MAIN, 0]
    assert [r[2] for r in res] == [False, False, False, False, False, False, True, False, False, True, True, False]
    assert [int(r[0][1].sum()) for r in res] == [14, 14, 14, 12, 12, 14, 0, 14, 12, 0, 0, 0]


def test_public_functions(backend):
    """infer3d's entry points on the backend's device (the emulated library takes host tensors, so the host-tensor refusal is patched out there)"""
    hard, labels = brats_case()
    opts = dict(wt_largest_only=True, et_min_voxels=N_ET_MAIN + 1, connectivity=6)
    with torch.device('cpu'):
        want, want_labels, _ = ref_brats(hard, labels, **opts)
        lab_ref, sizes_ref = ref_labels3d(hard[2:3] != 0, 6)
    x, l = hard.to(backend.dev), labels.to(backend.dev)
    orig = infer3d._device_operand
    if backend.name == 'emu':
        infer3d._device_operand = lambda what, t: None
    try:
        assert torch.equal(infer3d.postprocess_brats(x, **opts).cpu(), want)
        out, new = infer3d.postprocess_brats(x, l, **opts)
        assert torch.equal(out.cpu(), want) and torch.equal(new.cpu(), want_labels)
        lab, sizes = infer3d.connected_components(x[2], connectivity=6)
        assert torch.equal(lab.cpu(), lab_ref[0]) and torch.equal(sizes.cpu(), sizes_ref[0])
        clean = infer3d.remove_small_components(x[2] != 0, min_voxels=N_SAT_A + 1)
        assert clean.dtype == torch.bool and int(clean.sum()) == N_WT_MAIN + N_SAT_B
    finally:
        infer3d._device_operand = orig


def test_nan_in_preds_soft_does_not_matter(backend, monkeypatch):
    """the rule reads preds_hard alone: with a preds_soft full of NaN behind the merge, test_single_case(fused=True, postprocess=) still gives the referee's hard' and
    hands the same preds_soft back (a constructed prediction in place of the forwards: _Plan3d.run is patched)"""
    hard, _ = brats_case()
    opts = dict(wt_min_voxels=N_SAT_A + 1, et_min_voxels=N_ET_MAIN + N_ET_SAT + 1)
    with torch.device('cpu'):
        want, _, dropped = ref_brats(hard, None, **opts)
    assert dropped
    x = hard.to(backend.dev)
    soft = torch.full_like(x, float('nan'))
    monkeypatch.setattr(infer3d._Plan3d, 'run', lambda self, net, image: (x, soft))

    class Net:
        batchnorm_folded = False
    image = torch.zeros(4, *SHAPE_B, device=backend.dev)
    got_hard, got_soft = infer3d.test_single_case(Net(), image, (8, 8, 8), (8, 8, 8), 2, 4, 4, 'brats', fused=True, postprocess=opts)
    assert torch.equal(got_hard.cpu(), want) and got_soft is soft and bool(torch.isnan(got_soft).all())
    assert torch.equal(x.cpu(), hard)


# ---- host side: no kernel runs ----------------------------------------------------------------------------------------------------------------------------------
def test_header_constants():
    hdr = open(os.path.join(ROOT, 'include', 'segx.h')).read()
    d = {k: int(v, 0) for k, v in re.findall(r'#define\s+(SEGX_CCL3_\w+)\s+(\w+)', hdr)}
    assert (d['SEGX_CCL3_TILE_X'], d['SEGX_CCL3_TILE_Y'], d['SEGX_CCL3_TILE_Z']) == tuple(segx.SegxLib.CCL3_TILE)


def test_argument_refusals():
    """ValueError before anything is launched: no library is installed here, so a launch would fail differently"""
    host = torch.zeros(4, 4, 4, 4, device='cpu')
    with pytest.raises(ValueError, match='host tensor'):
        infer3d.connected_components(host[0])
    with pytest.raises(ValueError, match='host tensor'):
        infer3d.remove_small_components(host[0], 3)
    with pytest.raises(ValueError, match='host tensor'):
        infer3d.postprocess_brats(host)
    for conn in (18, 8, 0, None, '26', True):
        with pytest.raises(ValueError, match='connectivity'):
            infer3d.connected_components(host[0], connectivity=conn)
        with pytest.raises(ValueError, match='connectivity'):
            infer3d.remove_small_components(host[0], connectivity=conn)
        with pytest.raises(ValueError, match='connectivity'):
            infer3d.postprocess_brats(host, connectivity=conn)
        with pytest.raises(ValueError, match='connectivity'):
            infer3d.check_postprocess(dict(connectivity=conn))
    with pytest.raises(ValueError, match='min_voxels'):
        infer3d.remove_small_components(host[0], min_voxels=-1)
    for key in ('wt_min_voxels', 'et_min_voxels'):
        with pytest.raises(ValueError, match=key):
            infer3d.postprocess_brats(host, **{key: -1})
        with pytest.raises(ValueError, match=key):
            infer3d.check_postprocess({key: -3})
        with pytest.raises(ValueError, match=key):
            infer3d.check_postprocess({key: 2.5})
    for odd in (None, 'many', float('inf'), float('nan'), [3], True):
        with pytest.raises(ValueError, match='not a non-negative voxel count'):
            infer3d.remove_small_components(host[0], min_voxels=odd)
        with pytest.raises(ValueError, match='not a non-negative voxel count'):
            infer3d.check_postprocess(dict(et_min_voxels=odd))
    with pytest.raises(ValueError, match='unknown keys'):
        infer3d.check_postprocess(dict(min_voxels=3))
    with pytest.raises(ValueError, match='dict'):
        infer3d.check_postprocess('largest')
    with pytest.raises(ValueError, match='num_classes'):
        infer3d.check_postprocess(dict(), num_classes=3)
    with pytest.raises(ValueError, match='num_classes'):
        infer3d.postprocess_brats(torch.zeros(3, 4, 4, 4, device='cpu'))
    assert infer3d.check_postprocess(None) is None and infer3d.check_postprocess(None, num_classes=2) is None
    assert infer3d.check_postprocess(dict(et_min_voxels=5)) == dict(wt_min_voxels=0, wt_largest_only=False, et_min_voxels=5, connectivity=26)
    # the evaluation entry points refuse before they touch the net (there is none) or the data
    bad = dict(wt_min_voxels=-1)
    with pytest.raises(ValueError, match='wt_min_voxels'):
        infer3d.test_single_case(None, host, (4, 4, 4), (4, 4, 4), 1, 2, 2, 'brats', fused=True, postprocess=bad)
    with pytest.raises(ValueError, match='num_classes'):
        infer3d.test_single_case(None, host, (4, 4, 4), (4, 4, 4), 1, 2, 2, 'brats', num_classes=2, postprocess=dict())
    with pytest.raises(ValueError, match='unknown keys'):
        infer3d.test_all_cases(None, [], postprocess=dict(largest=True))
    with pytest.raises(ValueError, match='num_classes'):
        infer3d.test_all_cases(None, [], num_classes=3, postprocess=dict())
    with pytest.raises(ValueError, match='connectivity'):
        infer3d.GraphedSlidingWindow3d(None, (4, 8, 8, 8), (4, 4, 4), (4, 4, 4), 1, 2, 2, postprocess=dict(connectivity=18))


def test_postprocess_none_takes_todays_path(monkeypatch):
    """postprocess=None builds the same plan object as a call without the argument and never reaches the rule"""
    plans = []

    def run(self, net, image):
        plans.append(self)
        return 'hard', 'soft'

    def refuse(*a, **k):
        raise AssertionError('the rule ran')
    monkeypatch.setattr(infer3d._Plan3d, 'run', run)
    monkeypatch.setattr(SF, 'brats_postprocess', refuse)

    class Net:
        batchnorm_folded = False
    image = torch.zeros(4, 20, 24, 16, device='cpu')
    args = (Net(), image, (16, 16, 16), (16, 16, 16), 2, 8, 8, 'brats')
    assert infer3d.test_single_case(*args, fused=True) == ('hard', 'soft')
    assert infer3d.test_single_case(*args, fused=True, postprocess=None) == ('hard', 'soft')
    a, b = plans
    assert type(a) is type(b) and set(vars(a)) == set(vars(b))
    for k, v in vars(a).items():
        if k == 'table':
            assert type(v) is type(b.table) and v.origins == b.table.origins and torch.equal(v.dev, b.table.dev)
        else:
            assert v == getattr(b, k), k
    with pytest.raises(AssertionError, match='the rule ran'):
        infer3d.test_single_case(*args, fused=True, postprocess=dict())
