"""Command line of the shape generator: the reference's `shape_generation/main.py` (main.py:24-111).

    python shape_main.py --FLAG --data_dir ../data/coco --output_dir ..          train
    python shape_main.py --NET_G <Model/netG_epoch_N.pth> --data_dir ../data/coco    one mask PNG per test image

Same arguments, same defaults (--PCP_LAMBDA 10: the perceptual term on the frozen VGG-19-bn, whose torchvision weights
are read from <data_dir>/pretrained/vgg19_bn-c79401a0.pth).  Training writes Model/ (checkpoints), Score/scores_<epoch>.txt
and, every --DISPLAY_INTERVAL iterations (default 5, the reference's config value; 0: never), the four grids
Image/{G,D,G2,D2}_average_<iter>.png.  Without --FLAG the test split is sampled with seed 100, unshuffled, into
<NET_G without .pth>/valid/single/<key>_<category word>.png (the first box of every image; --ALL_BOXES, an extension:
every box, <key>_<r>_<word>.png).  Refused, loudly and before any work: a non-zero --PCP_LAMBDA when the VGG file is
missing (`--PCP_LAMBDA 0` trains without the term), sampling without --NET_G, and a --NET_G that is not a file.  The
run happens on the GPU: `--gpu` names the device (default 0; the reference's `-1` CPU mode does not exist here).
"""
import argparse
import datetime
import os
import pprint
import random
import sys
import time

import numpy as np


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Train a shape generation network')
    parser.add_argument('--gpu', dest='gpu_ids', type=str, default='0')
    parser.add_argument('--data_dir', dest='data_dir', type=str, default='../data/coco')
    parser.add_argument('--manualSeed', type=int, help='manual seed')
    parser.add_argument('--output_dir', type=str, default='..')
    parser.add_argument('--MAX_EPOCH', type=int, default=60)
    parser.add_argument('--WORKERS', type=int, default=0)
    parser.add_argument('--NET_G', type=str, default='')
    parser.add_argument('--DISCRIMINATOR_LR', type=float, default=0.0002)
    parser.add_argument('--GENERATOR_LR', type=float, default=0.0002)
    parser.add_argument('--INS_LAMBDA', type=float, default=1.0)
    parser.add_argument('--GLB_LAMBDA', type=float, default=1.0)
    parser.add_argument('--PCP_LAMBDA', type=float, default=10.0)
    parser.add_argument('--R_NUM', type=int, default=1)
    parser.add_argument('--BATCH_SIZE', type=int, default=40)
    parser.add_argument('--FLAG', dest='FLAG', action='store_true')
    parser.add_argument('--DISPLAY_INTERVAL', type=int, default=5, help='iterations between grids; 0: none')
    parser.add_argument('--ALL_BOXES', action='store_true', help='sampling: one PNG per box, not only the first')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not args.FLAG:
        # before any device or data work
        if args.NET_G == '':
            sys.exit("shape_main.py: sampling (no --FLAG) needs --NET_G <checkpoint>; pass --FLAG to train")
        if not os.path.isfile(args.NET_G):
            print("shape_main.py: --NET_G %s is not a file" % args.NET_G, file=sys.stderr)
            sys.exit(2)
    else:
        from miscc.shape_losses import check_pcp_lambda
        # before any work: no silent fall-back to a loss without the term
        check_pcp_lambda(args.PCP_LAMBDA, os.path.join(args.data_dir, 'pretrained', 'vgg19_bn-c79401a0.pth'))

    if args.gpu_ids not in ('', '-1'):
        os.environ.setdefault("CUDA_VISIBLE_DEVICES", args.gpu_ids)
    import torch
    from miscc.config import cfg
    import shapeDataset
    from shape_trainer import condGANTrainer

    if args.data_dir != '':
        cfg.DATA_DIR = args.data_dir
    cfg.TRAIN.NET_G = args.NET_G
    cfg.TRAIN.MAX_EPOCH = args.MAX_EPOCH
    cfg.WORKERS = args.WORKERS
    cfg.TRAIN.DISCRIMINATOR_LR = args.DISCRIMINATOR_LR
    cfg.TRAIN.GENERATOR_LR = args.GENERATOR_LR
    cfg.TRAIN.RNN_GRAD_CLIP = 0.25
    cfg.TRAIN.PRINT_INTERVAL = 5
    cfg.TRAIN.DISPLAY_INTERVAL = args.DISPLAY_INTERVAL
    cfg.TRAIN.SMOOTH.INS_LAMBDA = args.INS_LAMBDA
    cfg.TRAIN.SMOOTH.GLB_LAMBDA = args.GLB_LAMBDA
    cfg.TRAIN.SMOOTH.PCP_LAMBDA = args.PCP_LAMBDA
    cfg.GAN.R_NUM = args.R_NUM
    cfg.TRAIN.BATCH_SIZE = args.BATCH_SIZE
    cfg.TRAIN.FLAG = bool(args.FLAG)
    cfg.GPU_IDS = [0]
    cfg.CUDA = True
    print('Using config:')
    pprint.pprint(cfg)

    if not args.FLAG:
        args.manualSeed = 100
    elif args.manualSeed is None:
        args.manualSeed = random.randint(1, 10000)
    random.seed(args.manualSeed)
    np.random.seed(args.manualSeed)
    torch.manual_seed(args.manualSeed)
    torch.cuda.manual_seed_all(args.manualSeed)

    timestamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    output_dir = '{0}/output_shape_gen/{1}_{2}'.format(args.output_dir, cfg.DATASET_NAME, timestamp)

    split_dir = 'train' if args.FLAG else 'test'
    dataset = shapeDataset.TextDataset(cfg.DATA_DIR, split_dir, base_size=cfg.TREE.BASE_SIZE)
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True,
                                             shuffle=bool(args.FLAG), num_workers=int(cfg.WORKERS))
    algo = condGANTrainer(output_dir, dataloader, dataset)
    start_t = time.time()
    if args.FLAG:
        algo.train()
        print('Total time for training:', time.time() - start_t)
        print('Model directory:', algo.model_dir)
    else:
        algo.sampling(split_dir, all_boxes=args.ALL_BOXES)
        print('Total time for sampling:', time.time() - start_t)


if __name__ == "__main__":
    main()
