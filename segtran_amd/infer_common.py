"""What the 2-D and the 3-D evaluation (infer2d.py, infer3d.py) share on the host: the precision switch, the fold-for-a-block context manager, the chunk runner of
the fused sliding-window sequence and the captured-evaluation core (GraphedEvaluation).  A task supplies its plan, its `_sequence()` and its buffers."""
import contextlib

import torch

PRECISIONS = {'fp32': 6, 'bf16x3': 3}           # name -> Knob.X6_TERMS: bf16 products per block of the bf16 tile engine


@contextlib.contextmanager
def inference_precision(name):
    """with inference_precision('bf16x3'): the GEMMs and the forward 3-D convolutions of the bf16 tile engine run the three-term product (hi.mid + mid.hi + hi.hi on
    two bf16 planes per operand) on the routes that have such a kernel -- accurate to (2^-15 + 2^-16) |A|.|B| per element instead of fp32-equivalent; 'fp32' is the default behaviour.
    The setting is process-wide for the duration of the block (segx_tune knob X6_TERMS) and the value it held comes back at the end, also after an exception.
    Inference only: the training parity bar rules the mode out, so entering with gradients enabled raises RuntimeError; an unknown name raises ValueError."""
    if name not in PRECISIONS:
        raise ValueError('inference_precision: %r is not one of %s' % (name, sorted(PRECISIONS)))
    if torch.is_grad_enabled():
        raise RuntimeError("inference_precision(%r) is for inference: enter it under torch.no_grad()" % (name,))
    from . import segx
    with segx.lib().tuned(x6_terms=PRECISIONS[name]):
        yield


@contextlib.contextmanager
def _precision(precision):
    """the `precision` argument of the evaluation entry points: 'fp32' leaves everything as the caller has it, 'bf16x3' runs the block without gradients inside
    inference_precision('bf16x3')"""
    if precision not in PRECISIONS:
        raise ValueError('precision: %r is not one of %s' % (precision, sorted(PRECISIONS)))
    if precision == 'fp32':
        yield
    else:
        with torch.no_grad(), inference_precision(precision):
            yield


@contextlib.contextmanager
def folded(net, fold_bn, fold, unfold):
    """fold_bn of the evaluation entry points: fold(net) for the block if asked and net.batchnorm_folded is not set already, unfold(net) at its end, also after an
    exception; a net the caller folded stays folded"""
    here = bool(fold_bn) and not net.batchnorm_folded
    if here:
        fold(net)
    try:
        yield
    finally:
        if here:
            unfold(net)


def run_chunks(net, patches, chunks):
    """net() on the row ranges `chunks` = [(row0, row1)] of patches, in order; the scores side by side in one buffer, as window_merge reads them.  One chunk: net()'s
    own result, no buffer.  The caller holds torch.no_grad()."""
    if len(chunks) == 1:
        r0, r1 = chunks[0]
        return net(patches[r0:r1])
    scores = None
    for r0, r1 in chunks:
        part = net(patches[r0:r1])
        if scores is None:
            scores = part.new_empty((patches.shape[0],) + tuple(part.shape[1:]))
        scores[r0:r1] = part                                     # plumbing
    return scores


def view_chunks(chunks, rows_per_view, V):
    """the row ranges `chunks` of one view's patches repeated for V views, view after view: a net() call never mixes views, so the forwards keep the shapes (and the
    bits) they have without test-time augmentation"""
    return [(v * rows_per_view + r0, v * rows_per_view + r1) for v in range(V) for r0, r1 in chunks]


def composed_tta(evaluate, image, views, first_axis, mode):
    """Flip test-time augmentation as a host loop over an existing evaluation -- the definition the fused form (SF.window_gather / SF.window_merge with views=) is
    held to, bit for bit.  evaluate(image) -> (preds_hard, preds_soft) of one image or batch; views: check_views()' tuples of spatial axes, spatial
    axis a being dimension first_axis + a of both the image and preds_soft.  Per view, in order: torch.flip the image, evaluate, flip preds_soft back;
    preds_soft = (((soft_0 + soft_1) + soft_2) + ...) / float(V) in fp32 -- the divisor is a device tensor, so the division is a division and not ATen's product
    with a reciprocal --, then SF.harden_segmap(mode) on the mean.  Returns (hard, soft) as harden_segmap leaves them (float 0 / 1 hard)."""
    from . import functional as SF
    with torch.no_grad():
        total = None
        for view in views:
            dims = tuple(first_axis + a for a in view)
            _, soft = evaluate(torch.flip(image, dims) if dims else image)
            soft = torch.flip(soft, dims) if dims else soft
            total = soft if total is None else total + soft
        mean = total / total.new_full((), float(len(views)))
        batched = mean if first_axis == 2 else mean.unsqueeze(0)
        soft, hard = SF.harden_segmap(batched, mode=mode)
        return (hard, soft) if first_axis == 2 else (hard[0], soft[0])


class GraphedEvaluation:
    """The captured-evaluation core: one evaluation sequence of one input shape, warmed up, captured into a hipGraph and replayed.  A subclass supplies
    `_build(device, *args)` (self.plan, whose .shape is the input's, and its own static buffers; self.image is made here), `_sequence()` -> (preds_hard, preds_soft)
    (the launches to capture; reads self.image), `_check_classes()` and, where the fold is not the net's own method, `_fold` / `_unfold`.  Its __call__ is
    `_check(image)`, its own guards and copies, `_replay(image)` and its own tuple of static results."""

    @staticmethod
    def _fold(net):
        net.fold_batchnorm()

    @staticmethod
    def _unfold(net):
        net.unfold_batchnorm()

    def __init__(self, net, num_classes, fold_bn, warmup, precision, *plan_args):
        from . import segx
        name = type(self).__name__
        if net.training:
            raise RuntimeError('%s is for inference: call net.eval() first' % name)
        if precision not in PRECISIONS:
            raise ValueError('precision: %r is not one of %s' % (precision, sorted(PRECISIONS)))
        self.precision = precision
        assert segx.lib().gemm_prof is None, 'per-launch event profiling cannot run inside a captured evaluation'
        device = next(net.parameters()).device
        self.net, self.num_classes = net, num_classes
        self._folded_here = bool(fold_bn) and not net.batchnorm_folded
        if self._folded_here:
            self._fold(net)
        try:
            self.folded = net.batchnorm_folded
            self._build(device, *plan_args)                         # the window table: built before capture
            self.image = torch.zeros(self.plan.shape, dtype=torch.float32, device=device)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad(), _precision(precision):   # eager warm-up: GEMM plans, derived operands, allocator pools
                for _ in range(warmup):
                    self._sequence()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), _precision(precision), torch.cuda.graph(self.graph):
                self.preds_hard, self.preds_soft = self._sequence()
            self._check_classes()
        except BaseException:                                   # leave the net as it was found
            self.graph = None
            if self._folded_here and net.batchnorm_folded:
                self._unfold(net)
            raise
        self.replays = 0

    def _check(self, image):
        """the replay guards every captured evaluation shares"""
        name = type(self).__name__
        if self.graph is None:
            raise RuntimeError('%s: closed' % name)
        if self.net.training:
            raise RuntimeError('%s: the net is in train mode; the captured evaluation is the eval-mode forward' % name)
        if self.net.batchnorm_folded != self.folded:
            raise RuntimeError('%s: the BatchNorm fold of the net changed since capture (train(), load_state_dict() or an in-place edit); build a new %s' % (name, name))
        if tuple(image.shape) != self.plan.shape:
            raise ValueError('%s: captured for images %r, got %r' % (name, self.plan.shape, tuple(image.shape)))

    def _replay(self, image):
        """copy the (checked) image into its static buffer and replay"""
        if image is not self.image:
            self.image.copy_(image, non_blocking=True)
        self.graph.replay()
        self.replays += 1

    def close(self):
        """drop the graph and its static tensors; unfold the net if the constructor folded it"""
        self.graph = self.preds_hard = self.preds_soft = None
        if self._folded_here and self.net.batchnorm_folded:
            self._unfold(self.net)
        self._folded_here = False
