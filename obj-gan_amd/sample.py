"""Box generator, sampling: captions -> layouts (reference box_generation/sample.py, the --is_training 0 branch).

    python sample.py --is_training 0 --dev_path .../input_val2014.txt --dev_filename_path .../filenames_val2014.txt \\
        --mean_std_path .../mean_std_train2014.txt --gaussian_dict_path .../gaussian_dict.npy \\
        --expt_dir EXPT --load_checkpoint NAME --encoder_path .../text_encoder100.pth --box_saving_folder .../gen_masks

writes `<box_saving_folder>_<NAME>/<key>/<i>/boxes.txt`, one file per caption.  Same flags and defaults as the
reference; `--batch_size` is the number of captions per device batch, `--seed` (new) fixes the two random streams (the
decoder's noise and the per-category count thresholds).  Training (--is_training 1, the reference's default) is not
built here."""
import argparse
import logging
import os
import sys

import numpy as np
import torch


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--train_path', default='../data/coco/box_label/input_train2014.txt', help='Path to train data')
    parser.add_argument('--dev_path', default='../data/coco/box_label/input_val2014.txt', help='Path to dev data')
    parser.add_argument('--train_filename_path', default='../data/coco/box_label/filenames_train2014.txt',
                        help='Path to train filename data')
    parser.add_argument('--dev_filename_path', default='../data/coco/box_label/filenames_val2014.txt',
                        help='Path to dev filename data')
    parser.add_argument('--mean_std_path', default='../data/coco/box_label/mean_std_train2014.txt',
                        help='Path to the means and stds of the box values')
    parser.add_argument('--gaussian_dict_path', default='../data/coco/box_label/gaussian_dict.npy',
                        help='Path to gaussian dict')
    parser.add_argument('--vocab_path', default='../data/coco/captions.pickle', help='Path to the vocab path')
    parser.add_argument('--box_saving_folder', default='../data/coco/gen_masks', help='Path to box saving folder')
    parser.add_argument('--expt_dir', default='experiment', help='Path to experiment directory')
    parser.add_argument('--load_checkpoint', default='../data/pretrained/coco/box_ckpt',
                        help='The name of the checkpoint to load, usually an encoded time string')
    parser.add_argument('--resume', action='store_true', default=False)
    parser.add_argument('--log-level', dest='log_level', default='info', help='Logging level.')
    parser.add_argument('--batch_size', type=int, default=1, help='Captions per device batch.')
    parser.add_argument('--gmm_comp_num', type=int, default=5, help='The number of GMM components.')
    parser.add_argument('--lamda1', type=float, default=1.0)
    parser.add_argument('--lamda2', type=float, default=1.0)
    parser.add_argument('--count_smooth', type=float, default=1e5)
    parser.add_argument('--is_training', type=int, default=1, help='The state for training or test')
    parser.add_argument('--max_len', type=int, default=150, help='The max length for sequences')
    parser.add_argument('--min_len', type=int, default=1, help='The min length for sequences')
    parser.add_argument('--early_stop_len', type=int, default=10, help='The early-stop length for generation')
    parser.add_argument('--output_opt', type=int, default=0, help='The output option (0/1)')
    parser.add_argument('--embedding_dim', type=int, default=256, help='The embedding dimension')
    parser.add_argument('--encoder_path', type=str, default='../data/coco/pretrained/text_encoder100.pth',
                        help='encoder path.')
    parser.add_argument('--seed', type=int, default=None, help='Seed of the noise and threshold streams.')
    return parser


def main(argv=None):
    opt = build_parser().parse_args(argv)
    logging.basicConfig(format='%(asctime)s %(name)-12s %(levelname)-8s %(message)s',
                        level=getattr(logging, opt.log_level.upper()))
    if opt.is_training:
        print("sample.py: --is_training 1 (training the box generator) is not built in this project; train it with the "
              "reference and sample here with --is_training 0", file=sys.stderr)
        return 2
    if not torch.cuda.is_available():
        print("sample.py: the sampling path runs on the GPU kernels; no device found", file=sys.stderr)
        return 3

    from seq2seq.models import PreEncoderRNN
    from seq2seq.dataset.prepare_dataset import prepare_test_data, get_class_sta
    from seq2seq.evaluator import Evaluator
    from seq2seq.util.checkpoint import Checkpoint

    box_saving_folder = '%s_%s/' % (opt.box_saving_folder, opt.load_checkpoint)
    checkpoint_path = os.path.join(opt.expt_dir, Checkpoint.CHECKPOINT_DIR_NAME, opt.load_checkpoint)
    logging.info("loading checkpoint from {}".format(checkpoint_path))
    checkpoint = Checkpoint.load(checkpoint_path)
    decoder = checkpoint.model.eval().cuda()

    if not os.path.isfile(opt.gaussian_dict_path):
        print('calculating means and stds of the per-category box counts...')
        get_class_sta(opt.train_path, opt.gaussian_dict_path)
    gaussian_dict = np.load(opt.gaussian_dict_path, allow_pickle=True).item()

    encoder = PreEncoderRNN(len(checkpoint.cap_word2index), nhidden=opt.embedding_dim)
    encoder.load_state_dict(torch.load(opt.encoder_path, map_location='cpu'))
    encoder.eval().cuda()

    dev_cap_lang, dev_label_lang, dev_tuples, x_mean_std, y_mean_std, w_mean_std, r_mean_std, keys = \
        prepare_test_data(opt.dev_path, opt.mean_std_path, opt.max_len, opt.min_len, checkpoint.cap_word2index,
                          checkpoint.cap_index2word, checkpoint.label_word2index, checkpoint.label_index2word,
                          opt.dev_filename_path)
    rng = None
    if opt.seed is not None:
        np.random.seed(opt.seed)                       # the count thresholds of the post-processing
        rng = np.random.RandomState(opt.seed + 1)      # the decoder's noise
    evaluator = Evaluator(opt.batch_size, opt.early_stop_len, opt.expt_dir, dev_cap_lang, dev_label_lang, x_mean_std,
                          y_mean_std, w_mean_std, r_mean_std, gaussian_dict, box_saving_folder, opt.output_opt)
    with torch.no_grad():
        evaluator.evaluate(encoder, decoder, dev_tuples, keys, rng=rng)
    return 0


if __name__ == '__main__':
    sys.exit(main())
