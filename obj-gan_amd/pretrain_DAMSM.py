"""Command line of the DAMSM pretraining (AttnGAN's pretrain_DAMSM.py, where the reference's download of
`pretrained/text_encoder100.pth` / `image_encoder100.pth` comes from):

    python pretrain_DAMSM.py --gpu 0 --data_dir ../data/coco --output_dir ..

trains the caption encoder and the image encoder's two projections on the prepared data directory the other commands
read (prepare_data.py builds it) and writes `<output_dir>/output_damsm/<dataset>_<time>/Model/text_encoder<epoch>.pth`
and `image_encoder<epoch>.pth` every --SNAPSHOT_INTERVAL epochs and at the end: plain state dicts with the reference's
keys, the pair cfg.TRAIN.NET_E names (copy them to <data_dir>/pretrained/text_encoder100.pth and image_encoder100.pth,
or edit NET_E).  The frozen Inception-v3 trunk starts from torchvision's ImageNet weights, read from
<data_dir>/pretrained/inception_v3_google-1a9a5a14.pth or --NET_INCEPTION; `--NET_E <text_encoder*.pth>` resumes from
a pair instead.  The published recipe is the default of every flag.  One GPU: the loss couples all pairs of a batch.

Refused with one line on stderr and exit status 2, before any work: a missing data directory, a missing Inception
weights file, a missing resume pair, no device.
"""
import argparse
import datetime
import os
import pprint
import random
import sys
import time

import numpy as np

dir_path = os.path.abspath(os.path.dirname(os.path.realpath(__file__)))
if dir_path not in sys.path:
    sys.path.append(dir_path)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Pretrain the DAMSM text and image encoders')
    parser.add_argument('--gpu', dest='gpu_ids', type=str, default='0')
    parser.add_argument('--data_dir', dest='data_dir', type=str, default='../data/coco')
    parser.add_argument('--manualSeed', type=int, help='manual seed')
    parser.add_argument('--output_dir', type=str, default='..')
    parser.add_argument('--WORKERS', type=int, default=0)
    parser.add_argument('--BATCH_SIZE', type=int, default=48)
    parser.add_argument('--ENCODER_LR', type=float, default=0.002)
    parser.add_argument('--RNN_GRAD_CLIP', type=float, default=0.25)
    parser.add_argument('--MAX_EPOCH', type=int, default=600)
    parser.add_argument('--SNAPSHOT_INTERVAL', type=int, default=5)
    parser.add_argument('--PRINT_INTERVAL', type=int, default=200, help='steps between progress lines; 0: none')
    parser.add_argument('--NET_E', type=str, default='', help='resume from this text_encoder*.pth and its image_encoder*.pth')
    parser.add_argument('--NET_INCEPTION', type=str, default='',
                        help="torchvision's Inception-v3 ImageNet state dict (default: <data_dir>/pretrained/...)")
    return parser.parse_args(argv)


def refuse(msg):
    print("pretrain_DAMSM.py: " + msg, file=sys.stderr)
    sys.exit(2)


def has_test_split(data_dir):
    return all(os.path.isfile(os.path.join(data_dir, f))
               for f in ('test/filenames.pickle', 'test_imgs.bigfile', 'test_gt_insanns.pickle'))


def main(argv=None):
    args = parse_args(argv)
    import damsm_trainer
    net_inception = args.NET_INCEPTION or os.path.join(args.data_dir, 'pretrained', damsm_trainer.INCEPTION_FILE)
    try:
        damsm_trainer.check_files(args.data_dir, args.NET_E, net_inception)
    except damsm_trainer.Refusal as e:
        refuse(str(e))
    if args.gpu_ids not in ('', '-1'):
        os.environ.setdefault("CUDA_VISIBLE_DEVICES", args.gpu_ids)
    import torch
    if args.gpu_ids in ('', '-1') or not torch.cuda.is_available():
        refuse("no device: the encoders train on the GPU (--gpu <id>)")
    from miscc.config import cfg
    from trainDataset import TrainDataset, build_loader

    cfg.DATA_DIR = args.data_dir
    cfg.TRAIN.BATCH_SIZE = args.BATCH_SIZE
    cfg.TRAIN.MAX_EPOCH = args.MAX_EPOCH
    cfg.TRAIN.SNAPSHOT_INTERVAL = args.SNAPSHOT_INTERVAL
    cfg.TRAIN.PRINT_INTERVAL = args.PRINT_INTERVAL
    cfg.TRAIN.NET_E = args.NET_E
    cfg.TRAIN.FLAG = True
    cfg.WORKERS = args.WORKERS
    cfg.GPU_IDS = [0]
    cfg.CUDA = True
    print('Using config:')
    pprint.pprint(cfg)

    if args.manualSeed is None:
        args.manualSeed = random.randint(1, 10000)
    random.seed(args.manualSeed)
    np.random.seed(args.manualSeed)
    torch.manual_seed(args.manualSeed)
    torch.cuda.manual_seed_all(args.manualSeed)

    device = torch.device("cuda", 0)
    timestamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    output_dir = '{0}/output_damsm/{1}_{2}'.format(args.output_dir, cfg.DATASET_NAME, timestamp)

    dataset = TrainDataset(cfg.DATA_DIR, 'train', base_size=cfg.TREE.BASE_SIZE, device_hmaps=True)
    dataloader = build_loader(dataset, cfg.TRAIN.BATCH_SIZE, workers=int(cfg.WORKERS), seed=args.manualSeed, shuffle=True)
    val_loader = None
    if has_test_split(cfg.DATA_DIR):
        val_set = TrainDataset(cfg.DATA_DIR, 'test', base_size=cfg.TREE.BASE_SIZE, device_hmaps=True)
        val_loader = build_loader(val_set, cfg.TRAIN.BATCH_SIZE, workers=int(cfg.WORKERS), shuffle=False)
    text_encoder, image_encoder, start_epoch = damsm_trainer.build_encoders(dataset.n_words, args.NET_E, net_inception,
                                                                            device)
    algo = damsm_trainer.DAMSMTrainer(output_dir, dataloader, dataset, device, text_encoder, image_encoder,
                                      start_epoch=start_epoch, encoder_lr=args.ENCODER_LR,
                                      rnn_grad_clip=args.RNN_GRAD_CLIP, max_epoch=args.MAX_EPOCH,
                                      snapshot_interval=args.SNAPSHOT_INTERVAL, print_interval=args.PRINT_INTERVAL,
                                      val_loader=val_loader)
    start_t = time.time()
    algo.train()
    print('Total time for training:', time.time() - start_t)
    print('Model directory:', algo.model_dir)
    return algo


if __name__ == "__main__":
    main()
