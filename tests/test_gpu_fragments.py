"""GPU only: component labelling, fragment removal and vCDR at a size where thousands of workgroups on all XCDs unite one component at the same time, and the whole
evaluation tail captured into a graph (a capture fails on a synchronisation or a copy to the host, so a replay that matches proves there is none)."""
import functools

import pytest
import torch

from segtran_amd import functional as SF
from segtran_amd import infer2d, segx
from fragments_referee import ref_labels, ref_remove

pytestmark = pytest.mark.gpu
N = 1024
TH, TW = segx.SegxLib.CCL_TILE


def fundus_plane(dev, shift=0):
    """uint8 [N, N] by formula: background 255, a disc (128) of radius 300 with a cup (0) of radius 120 inside, 200 specks of 1 to 4 pixels outside the disc, and two
    4 x 4 squares that touch only diagonally, at a corner where four tiles meet"""
    y, x = torch.meshgrid(torch.arange(N, device=dev), torch.arange(N, device=dev), indexing='ij')
    cy, cx = 500 + shift, 520 - shift
    seg = torch.full((N, N), 255, dtype=torch.uint8, device=dev)
    seg[(y - cy) ** 2 + (x - cx) ** 2 <= 300 * 300] = 128
    seg[(y - cy - 20) ** 2 + (x - cx + 10) ** 2 <= 120 * 120] = 0
    k = torch.arange(200, device=dev)
    sy, sx = (k * 389 + 17) % N, (k * 683 + 5) % N
    far = (sy - cy) ** 2 + (sx - cx) ** 2 > 330 * 330
    for d in range(4):
        on = far & (k % 4 >= d)
        seg[sy[on], (sx[on] + d) % N] = 128
    cyt, cxt = 2 * TH, TW                                                               # tiles meet at (64, 64)
    seg[cyt - 4:cyt, cxt - 4:cxt] = 0
    seg[cyt:cyt + 4, cxt:cxt + 4] = 0
    return seg


def nhot_of(seg):
    return torch.stack([seg == 255, seg <= 128, seg == 0]).float()


@functools.lru_cache(None)
def referee(shift=0):
    dev = torch.device('cuda', 0)
    seg = fundus_plane(dev, shift)
    labels, sizes = ref_labels((seg != 255)[None], check_every=32)
    return seg, labels[0], sizes[0], ref_remove(seg[None], 255, check_every=32)[0]


def test_large_plane_against_the_referee():
    segx.use_library(None)
    seg, labels_ref, sizes_ref, clean_ref = referee()
    labels, sizes = SF.label_components(seg, bg_value=255)
    assert torch.equal(labels, labels_ref) and torch.equal(sizes, sizes_ref)
    corner = labels[2 * TH - 1, TW - 1]
    assert int(corner) == 1 + (2 * TH - 4) * N + TW - 4 and int(labels[2 * TH, TW]) == int(corner)       # the diagonal bridge across the tile corner holds
    assert int(sizes[2 * TH - 4, TW - 4]) == 32
    assert int((sizes > 0).sum()) > 100                                                 # the disc, the squares and the specks
    clean = infer2d.remove_fragmentary_segs(seg, 255)
    assert torch.equal(clean, clean_ref)
    assert int((clean != 255).sum()) == int(sizes.max()) and int((clean != seg).sum()) > 200             # only the disc (with its cup) is left
    assert torch.equal(SF.label_components(seg, bg_value=255)[0], labels)               # and again: the same bits


def test_evaluation_tail_is_capturable():
    segx.use_library(None)
    dev = torch.device('cuda', 0)
    seg0, _, _, clean0 = referee()
    seg1 = fundus_plane(dev, shift=37)
    static_seg, static_nhot = seg0.clone(), nhot_of(seg0)

    def tail():
        return infer2d.remove_fragmentary_segs(static_seg, 255), infer2d.calc_vcdr(static_nhot), infer2d.calc_vcdr(static_nhot[None])

    eager = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():                                      # warm-up off the capture: allocator pools, the value tables
        for key, seg in ((0, seg0), (1, seg1)):
            static_seg.copy_(seg); static_nhot.copy_(nhot_of(seg))
            eager[key] = [t.clone() for t in tail()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(eager[0][0], clean0) and not torch.equal(eager[0][0], eager[1][0])
    for key, seg in ((0, seg0), (1, seg1)):                                             # the ratio by plain row reductions
        rows = [(nhot_of(seg)[c] >= 0.5).any(dim=1).nonzero().view(-1) for c in (1, 2)]
        disc_len, cup_len = (r.max() - r.min() - 1 for r in rows)
        assert torch.equal(eager[key][1], cup_len / (disc_len + 0.0001)) and eager[key][2].shape == (1,)
    graph = torch.cuda.CUDAGraph()
    static_seg.copy_(seg0); static_nhot.copy_(nhot_of(seg0))
    torch.cuda.synchronize()
    with torch.no_grad(), torch.cuda.graph(graph):
        outs = tail()
    for key, seg in ((0, seg0), (1, seg1)):                                             # two replays, on different images
        static_seg.copy_(seg); static_nhot.copy_(nhot_of(seg))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[key]):
            assert got.dtype == want.dtype and torch.equal(got, want)
