"""Caption file -> images, in one process (pipeline.TextToImage):

    python generate.py --captions captions.txt --data_dir ../data/coco --NET_G <netG checkpoint> \\
        --box_ckpt <box generator checkpoint directory> --output_dir OUT [--BATCH_SIZE 16] [--seed S] [--save_layout]

One caption per line of the file (empty lines are skipped; line numbers count every line, from 1).  Writes
`OUT/Image/<line>_<k>.jpg` (k numbers the samples of a caption: 0) and, with --save_layout, `OUT/<line>/boxes.txt` in the format of
`sample.py --is_training 0`.  Read besides the two checkpoints, all under --data_dir unless given: the DAMSM text
encoder (--NET_E, also the box generator's caption encoder unless --box_encoder names another), the shape generator
(--NET_SHP_G), captions.pickle, captions_glove.pickle, categories.txt, the box generator's mean/std file (--mean_std)
and gaussian_dict.npy (--gaussian_dict).  A missing file is answered with one line on stderr and exit status 2 before
anything touches the device."""
import argparse
import os
import sys

dir_path = os.path.abspath(os.path.dirname(os.path.realpath(__file__)))
if dir_path not in sys.path:
    sys.path.append(dir_path)


def build_parser():
    p = argparse.ArgumentParser(description='Generate images from a file of captions')
    p.add_argument('--captions', required=True, help='text file, one caption per line')
    p.add_argument('--data_dir', required=True)
    p.add_argument('--NET_G', required=True, help='image generator checkpoint')
    p.add_argument('--box_ckpt', required=True, help='checkpoint directory of the box generator')
    p.add_argument('--output_dir', required=True)
    p.add_argument('--BATCH_SIZE', type=int, default=16)
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--save_layout', action='store_true')
    p.add_argument('--NET_E', default=None, help='DAMSM text encoder (default: <data_dir>/pretrained/text_encoder100.pth)')
    p.add_argument('--NET_SHP_G', default=None, help='shape generator (default: <data_dir>/pretrained/shape_ckpt/shape_gen.pth)')
    p.add_argument('--box_encoder', default=None, help="the box generator's caption encoder (default: --NET_E)")
    p.add_argument('--mean_std', default=None, help='default: <data_dir>/box_label/mean_std_train2014.txt')
    p.add_argument('--gaussian_dict', default=None, help='default: <data_dir>/box_label/gaussian_dict.npy')
    p.add_argument('--early_stop_len', type=int, default=10)
    p.add_argument('--gpu', type=int, default=0)
    return p


def read_captions(path):
    """-> [(line number, text)] of the non-empty lines"""
    with open(path) as f:
        return [(i, ln.strip()) for i, ln in enumerate(f.read().splitlines(), 1) if ln.strip()]


def main(argv=None):
    args = build_parser().parse_args(argv)
    import pipeline
    files = dict(pipeline.required_files(args.data_dir, args.NET_G, args.box_ckpt, args.NET_E, args.NET_SHP_G,
                                         args.box_encoder, args.mean_std, args.gaussian_dict))
    files["captions file"] = args.captions
    for role, path in files.items():
        if not os.path.isfile(path):
            print("generate.py: %s not found: %s" % (role, path), file=sys.stderr)
            return 2
    lines = read_captions(args.captions)
    if not lines:
        print("generate.py: no caption in %s" % args.captions, file=sys.stderr)
        return 2
    import torch
    if not torch.cuda.is_available():
        print("generate.py: the pipeline runs on the GPU kernels; no device found", file=sys.stderr)
        return 3
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    t2i = pipeline.TextToImage.from_files(args.data_dir, args.NET_G, args.box_ckpt, device, net_e=args.NET_E,
                                          net_shp_g=args.NET_SHP_G, box_encoder=args.box_encoder, mean_std=args.mean_std,
                                          gaussian_dict=args.gaussian_dict, early_stop_len=args.early_stop_len,
                                          batch_size=args.BATCH_SIZE, output_dir=args.output_dir)
    try:
        t2i.encode([text for _, text in lines], lines=[n for n, _ in lines])        # refusals before any image is made
    except ValueError as e:
        print("generate.py: %s" % e, file=sys.stderr)
        return 2
    numbers = [n for n, _ in lines]
    B = t2i.batch_size
    for k, start in enumerate(range(0, len(lines), B)):
        part = lines[start:start + B]
        images, layouts, _ = t2i.generate([text for _, text in part],
                                          seed=None if args.seed is None else args.seed + k,
                                          lines=[n for n, _ in part], notice=False)
        t2i.imager.save_singleimages(images, [n for n, _ in part], [0] * len(part))
        if args.save_layout:
            for (n, _), rows in zip(part, layouts):
                os.makedirs(os.path.join(args.output_dir, str(n)), exist_ok=True)
                with open(os.path.join(args.output_dir, str(n), 'boxes.txt'), 'w') as f:
                    f.write(pipeline.boxes_txt(rows))
    print("generate.py: %d images in %s" % (len(numbers), os.path.join(args.output_dir, 'Image')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
