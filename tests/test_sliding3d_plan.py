"""CPU: infer3d.sliding_windows -- pads, padded extent, window origins and the eager loop's grouping of the windows into net() calls -- against a transcription of the
loops of test_util3d.test_single_case (reference test_util3d.py:93-166) that records what the loop crops and when it flushes."""
import math

import pytest

import segtran_amd
from segtran_amd import infer3d


def eager_loops(H, W, D, patch, stride_xy, stride_z, batch_size):
    """the loops of test_util3d.test_single_case as they stand, with the crop origins and the flushed batches recorded"""
    dx, dy, dz = patch
    pads = [max(dx - H, 0), max(dy - W, 0), max(dz - D, 0)]
    lp = [p // 2 for p in pads]
    H2, W2, D2 = H + pads[0], W + pads[1], D + pads[2]
    sx = math.ceil((H2 - dx) / stride_xy) + 1
    sy = math.ceil((W2 - dy) / stride_xy) + 1
    sz = math.ceil((D2 - dz) / stride_z) + 1
    visited, batches = [], []
    for x in range(sx):
        xs = min(stride_xy * x, H2 - dx)
        patches = []
        for y in range(sy):
            ys = min(stride_xy * y, W2 - dy)
            for z in range(sz):
                zs = min(stride_z * z, D2 - dz)
                patches.append((xs, ys, zs))
                visited.append((xs, ys, zs))
                if len(patches) == batch_size or (y == sy - 1 and z == sz - 1):
                    batches.append(patches)
                    patches = []
        assert not patches
    return tuple(lp), (H2, W2, D2), visited, batches, (sx, sy, sz)


# (H, W, D), window, stride_xy, stride_z, (sx, sy, sz), what the case is there for
SHAPES = [
    ((120, 224, 16), (112, 112, 16), 56, 16, (2, 3, 1), 'sy * sz = 3; x clamped to 8'),
    ((125, 130, 40), (112, 112, 16), 56, 10, (2, 2, 4), 'the last origin of EVERY axis clamped (13, 18, 24)'),
    ((112, 168, 12), (112, 112, 16), 56, 16, (1, 2, 1), 'depth smaller than the window: padded by 4, left pad 2'),
    ((100, 112, 16), (112, 112, 16), 56, 16, (1, 1, 1), 'sy * sz = 1: one window, H padded by 12'),
    ((240, 240, 155), (112, 112, 96), 56, 48, (4, 4, 3), 'the BraTS case: 48 windows'),
    ((112, 224, 33), (112, 112, 16), 56, 16, (1, 3, 3), 'one x row; z clamped to 17 (sy * sz = 9)'),
    ((170, 168, 32), (112, 112, 16), 56, 16, (3, 2, 2), 'three x rows of sy * sz = 4'),
    ((113, 224, 32), (112, 112, 16), 56, 16, (2, 3, 2), 'sy * sz = 6; second x origin clamped to 1'),
]


@pytest.mark.parametrize('batch_size', [1, 2, 3, 100])
@pytest.mark.parametrize('shape,patch,sxy,sz,counts,why', SHAPES)
def test_geometry_and_chunks_are_the_eager_loops(shape, patch, sxy, sz, counts, why, batch_size):
    lp, canvas, visited, batches, n = eager_loops(*shape, patch, sxy, sz, batch_size)
    assert n == counts, why                                                    # the case is the one the list says it is
    pads, extent, origins, chunks = infer3d.sliding_windows(*shape, patch, sxy, sz, batch_size)
    assert tuple(pads) == lp and tuple(extent) == canvas
    assert [tuple(o) for o in origins] == visited
    assert [origins[a:b] for a, b in chunks] == batches
    # every window exactly once, in order, and no chunk across an x row
    row = n[1] * n[2]
    assert [k for a, b in chunks for k in range(a, b)] == list(range(len(origins)))
    for a, b in chunks:
        assert 0 < b - a <= batch_size and a // row == (b - 1) // row
        assert len({origins[k][0] for k in range(a, b)}) == 1
    # the last origin of each axis reaches the end of the padded extent
    for ax in range(3):
        assert max(o[ax] for o in origins) == extent[ax] - patch[ax] and min(o[ax] for o in origins) == 0


def test_the_list_covers_the_chunk_forms():
    """sy * sz = 1, 3 and 6 against batch sizes 1, 2, 3 and 100: full chunks only, a short last chunk, and a chunk that never fills"""
    rows = {c[4][1] * c[4][2] for c in SHAPES}
    assert {1, 3, 6} <= rows
    _, _, _, chunks = infer3d.sliding_windows(120, 224, 16, (112, 112, 16), 56, 16, 2)
    assert chunks == [(0, 2), (2, 3), (3, 5), (5, 6)]                           # 2 + 1 per row
    _, _, _, chunks = infer3d.sliding_windows(120, 224, 16, (112, 112, 16), 56, 16, 100)
    assert chunks == [(0, 3), (3, 6)]                                           # never fills: the flush at the end of the row
    _, _, _, chunks = infer3d.sliding_windows(113, 224, 32, (112, 112, 16), 56, 16, 3)
    assert chunks == [(0, 3), (3, 6), (6, 9), (9, 12)]                          # full chunks only
    assert all(c[4][0] * c[4][1] * c[4][2] == 48 for c in SHAPES if c[0] == (240, 240, 155))


@pytest.mark.parametrize('sxy,sz', [(0, 16), (56, 0), (-1, 16), (113, 16), (56, 17)])
def test_a_stride_outside_the_window_is_refused(sxy, sz):
    with pytest.raises(ValueError, match='stride'):
        infer3d.sliding_windows(224, 224, 32, (112, 112, 16), sxy, sz, 2)


def test_a_stride_above_the_smaller_in_plane_extent_is_refused():
    with pytest.raises(ValueError, match='stride'):
        infer3d.sliding_windows(224, 224, 32, (128, 112, 16), 120, 16, 2)
    infer3d.sliding_windows(224, 224, 32, (128, 112, 16), 112, 16, 2)


def test_batch_size_below_one_is_refused():
    with pytest.raises(ValueError, match='batch_size'):
        infer3d.sliding_windows(224, 224, 32, (112, 112, 16), 56, 16, 0)


def test_lazy_export():
    assert segtran_amd.GraphedSlidingWindow3d is infer3d.GraphedSlidingWindow3d
