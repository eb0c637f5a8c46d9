"""COCO's instance JSON -> the instance-annotation pickles of a data directory (miscc/coco_prep.py):

    python prepare_data.py --data_dir ../data/coco --split train|test --what gt|shape|both [--cpu] [--BATCH 64]

Reads `<data_dir>/insanns/instances_<train|val>2014.json` (`test` reads val2014), `<data_dir>/<split>/filenames.pickle`
and `<data_dir>/categories.txt`; writes `<split>_gt_insanns.pickle` (image generator) and / or
`<split>_shape_insanns.pickle` (shape generator) as the reference's loaders write them (`pickle.dump([dict], f,
protocol=2)`).  The masks are rasterised and resized on the GPU in batches of --BATCH images; --cpu (or a machine
without a GPU) takes the numpy + scipy route, which gives the same bits.  A missing file is answered with one line on
stderr and exit status 2 before anything touches the device."""
import argparse
import os
import pickle
import sys

dir_path = os.path.abspath(os.path.dirname(os.path.realpath(__file__)))
if dir_path not in sys.path:
    sys.path.append(dir_path)


def build_parser():
    p = argparse.ArgumentParser(description='Build the instance-annotation pickles from the COCO instance JSON')
    p.add_argument('--data_dir', required=True)
    p.add_argument('--split', required=True, choices=('train', 'test'))
    p.add_argument('--what', default='both', choices=('gt', 'shape', 'both'))
    p.add_argument('--cpu', action='store_true', help='numpy + scipy route even when a GPU is present')
    p.add_argument('--BATCH', type=int, default=64, help='images per device call')
    p.add_argument('--gpu', type=int, default=0)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from miscc import coco_prep, load
    from miscc.config import cfg
    files = {"annotation file": coco_prep.annotation_file(args.data_dir, args.split),
             "key list": os.path.join(args.data_dir, args.split, 'filenames.pickle'),
             "category list": os.path.join(args.data_dir, 'categories.txt')}
    for role, path in files.items():
        if not os.path.isfile(path):
            print("prepare_data.py: %s not found: %s" % (role, path), file=sys.stderr)
            return 2
    if args.BATCH < 1:
        print("prepare_data.py: --BATCH must be at least 1", file=sys.stderr)
        return 2
    filenames = load.load_filenames(args.data_dir, args.split)
    cats_index_dict = {int(line.split(',', 1)[0]): i for i, line in enumerate(load._category_lines(args.data_dir))}
    device = None
    if not args.cpu:
        import torch
        if torch.cuda.is_available():
            device = torch.device("cuda", args.gpu)
            torch.cuda.set_device(device)
    imsize = [cfg.TREE.BASE_SIZE * (2 ** b) for b in range(cfg.TREE.BRANCH_NUM)]
    jobs = []
    if args.what in ('gt', 'both'):
        jobs.append(('%s_gt_insanns.pickle' % args.split, coco_prep.build_gt_insanns, imsize))
    if args.what in ('shape', 'both'):
        jobs.append(('%s_shape_insanns.pickle' % args.split, coco_prep.build_shape_insanns, imsize[0]))
    for leaf, builder, size in jobs:
        try:
            insanns = builder(args.data_dir, filenames, args.split, size, cfg.ROI.FM_SIZE, cats_index_dict,
                              device=device, batch=args.BATCH)
        except (KeyError, ValueError) as e:
            print("prepare_data.py: %s" % (e.args[0] if e.args else e), file=sys.stderr)
            return 2
        path = os.path.join(args.data_dir, leaf)
        with open(path, 'wb') as f:
            pickle.dump([insanns], f, protocol=2)
        print("prepare_data.py: %d images in %s (%s route)" % (len(insanns), path, "host" if device is None else "device"))
    return 0


if __name__ == '__main__':
    sys.exit(main())
