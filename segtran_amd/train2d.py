"""`python -m segtran_amd.train2d --task fundus --net segtran --bb eff-b4 --translayers 3 --layercompress 1,1,2,2 --bs 6 ...`
Mirror of the reference's code/train2d.py for the `--net segtran` path (flags train2d.py:58-243)."""
import argparse
from . import train_common as tc

NUM_CLASSES = {'fundus': 3, 'polyp': 2, 'oct': 10}                        # train2d.py:286-384
DEFAULT_SIZE = {'fundus': (576, 576), 'polyp': (320, 320), 'oct': (288, 512)}   # orig_input_size defaults (oct: the 'duke' scans); --patch defaults to it


def parse_size(text, flag='--patch'):
    """'320' -> (320, 320); '288,512' -> (288, 512).  The backbone's finest feature map is 1/8 of the input (the stem and two strided stages), and the output
    pyramid doubles its way back, so both extents must be positive multiples of 8."""
    try:
        vals = [int(v) for v in str(text).split(',')]
    except ValueError:
        raise SystemExit('%s %s: a size S or H,W in pixels' % (flag, text))
    if len(vals) not in (1, 2):
        raise SystemExit('%s %s: a size S or H,W in pixels' % (flag, text))
    H, W = vals[0], vals[-1]
    if H <= 0 or W <= 0 or H % 8 or W % 8:
        raise SystemExit('%s %s: height and width must be positive multiples of 8 (the network works on 1/8-resolution tokens)' % (flag, text))
    return H, W


def parse_args(argv=None):
    """the finalised argument namespace and the run's config (size, classes) -- everything main() decides before a device is touched"""
    p = tc.common_flags(argparse.ArgumentParser(description=__doc__), 2)
    p.add_argument('--insize', dest='orig_input_size', type=str, default=None, help='S or H,W')
    p.add_argument('--patch', dest='patch_size', type=str, default=None, help='S or H,W (default: --insize)')
    p.add_argument('--exclusive', dest='use_exclusive_masks', action='store_true')
    p.add_argument('--focus', dest='focus_class', type=int, default=-1, help='The class that is particularly predicted (with higher loss weight)')
    args = tc.finalize_args(p.parse_args(argv), 2)
    if args.use_exclusive_masks and args.task_name != 'fundus':
        raise SystemExit('--exclusive only changes the fundus label map (datasets2d.py:110-111)')
    if args.task_name not in NUM_CLASSES:
        raise SystemExit("--task %s: only 'fundus', 'polyp' and 'oct' are wired" % args.task_name)
    if not args.backbone_type.startswith('eff-b') and args.backbone_type not in ('resnet34', 'resnet50', 'resnet101'):
        raise SystemExit('--bb %s: only EfficientNet-V1 (eff-b*) and resnet34 / resnet50 / resnet101 backbones are built' % args.backbone_type)
    if args.tune_bn_only and not args.backbone_type.startswith('eff'):    # train2d.py:1089-1100: --tunebn walks the EfficientNet blocks
        raise SystemExit("Backbone '%s' not supported by --tunebn." % args.backbone_type)
    nc = NUM_CLASSES[args.task_name]
    if args.focus_class != -1 and not 0 <= args.focus_class < nc:
        raise SystemExit('--focus %d: the %s task has classes 0 .. %d' % (args.focus_class, args.task_name, nc - 1))
    if args.patch_size is not None:
        size = parse_size(args.patch_size, '--patch')
    elif args.orig_input_size is not None:
        size = parse_size(args.orig_input_size, '--insize')
    else:
        size = DEFAULT_SIZE[args.task_name]
    return args, tc.make_cfg(args, 2, size, nc)


def main(argv=None):
    args, cfg = parse_args(argv)
    return tc.run(args, cfg)


if __name__ == '__main__':
    main()
