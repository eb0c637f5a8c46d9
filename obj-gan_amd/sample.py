"""Box generator: training (--is_training 1, the reference's default) and sampling captions -> layouts
(--is_training 0); reference box_generation/sample.py.

    python sample.py --is_training 1 --train_path .../input_train2014.txt --dev_path .../input_val2014.txt \\
        --mean_std_path .../mean_std_train2014.txt --vocab_path .../captions.pickle \\
        --encoder_path .../text_encoder100.pth --expt_dir EXPT [--batch_size B] [--resume] [--seed S]

trains the decoder for 10 epochs of len(train) / batch_size steps and writes checkpoints under EXPT/checkpoints/.  A
step is one fused device step over batch_size captions (seq2seq/trainer); batch_size 1 is the reference's schedule.

    python sample.py --is_training 0 --dev_path .../input_val2014.txt --dev_filename_path .../filenames_val2014.txt \\
        --mean_std_path .../mean_std_train2014.txt --gaussian_dict_path .../gaussian_dict.npy \\
        --expt_dir EXPT --load_checkpoint NAME --encoder_path .../text_encoder100.pth --box_saving_folder .../gen_masks

writes `<box_saving_folder>_<NAME>/<key>/<i>/boxes.txt`, one file per caption.  Same flags and defaults as the
reference; `--batch_size` is the number of captions per device batch, `--seed` (new) fixes the two random streams (the
decoder's noise and the per-category count thresholds; in training the init and the batch draws)."""
import argparse
import logging
import math
import os
import pickle
import random
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
    parser.add_argument('--seed', type=int, default=None,
                        help='Seed of the noise and threshold streams (sampling), of the init and batch draws (training).')
    parser.add_argument('--num_epochs', type=int, default=10, help='Training epochs (the reference trains 10).')
    parser.add_argument('--print_every', type=int, default=50, help='Steps between loss read-backs and log lines.')
    parser.add_argument('--checkpoint_every', type=int, default=100, help='Steps between checkpoints.')
    return parser


def label_weights(label_lang, count_smooth):
    """count_smooth / count^0.8 per label seen in training, 1 for the others (reference sample.py:99-105)"""
    weight = torch.ones(len(label_lang.word2index))
    for word, index in label_lang.word2index.items():
        if label_lang.word2count[word] == 0:
            continue
        weight[index] = weight[index] * count_smooth / float(math.pow(label_lang.word2count[word], 0.8))
    return weight


def new_decoder(label_word2index, means, batch_size, max_len, hidden_size, gmm_comp_num, seed=None):
    """the reference's fresh decoder: every parameter uniform(-0.08, 0.08), on the CPU.  With a seed the values come
    from a generator of their own (parameters in module order); torch's global generator is left alone."""
    from seq2seq.models import DecoderRNN
    decoder = DecoderRNN(label_word2index, means[0], means[1], means[2], means[3], batch_size, max_len, hidden_size,
                         gmm_comp_num, dropout_p=0.2, use_attention=False, bidirectional=True)
    generator = None if seed is None else torch.Generator().manual_seed(seed)
    for param in decoder.parameters():
        param.data.uniform_(-0.08, 0.08, generator=generator)
    return decoder


def train(opt):
    """the reference's --is_training 1 branch: vocabulary, label weights, uniform(-0.08, 0.08) init, 10 epochs"""
    missing = [p for p in (opt.train_path, opt.dev_path, opt.mean_std_path, opt.vocab_path, opt.encoder_path)
               if not os.path.isfile(p)]
    if missing or not torch.cuda.is_available():
        why = "missing input %s" % ", ".join(missing) if missing else "the training kernels need a GPU, none found"
        print("sample.py: training the box generator (--is_training 1) cannot start: %s" % why, file=sys.stderr)
        return 2

    from seq2seq.models import PreEncoderRNN
    from seq2seq.dataset.prepare_dataset import prepare_data
    from seq2seq.loss import Perplexity, BBLoss
    from seq2seq.trainer import SupervisedTrainer

    with open(opt.vocab_path, 'rb') as f:
        x = pickle.load(f)
    ixtoword, wordtoix = x[2], x[3]
    del x
    train_cap_lang, train_label_lang, train_tuples, dev_cap_lang, dev_label_lang, dev_tuples, \
        x_mean_std, y_mean_std, w_mean_std, r_mean_std = prepare_data(opt.train_path, opt.dev_path, opt.mean_std_path,
                                                                      opt.max_len, opt.min_len, ixtoword, wordtoix)
    rng = None
    if opt.seed is not None:
        random.seed(opt.seed)
        rng = random.Random(opt.seed + 1)              # the batch draws
    decoder = None
    if not opt.resume:
        decoder = new_decoder(train_label_lang.word2index, (x_mean_std[0], y_mean_std[0], w_mean_std[0], r_mean_std[0]),
                              opt.batch_size, opt.max_len, opt.embedding_dim, opt.gmm_comp_num, opt.seed).cuda()
    weight = label_weights(train_label_lang, opt.count_smooth)
    pad = train_label_lang.word2index["<pad>"]
    lloss = Perplexity(weight, pad, opt.lamda1)
    bloss = BBLoss(opt.batch_size, opt.gmm_comp_num, opt.lamda2)       # the fused step takes lamda2 and the name from it
    lloss.cuda()

    encoder = PreEncoderRNN(train_cap_lang.n_words, nhidden=opt.embedding_dim)
    encoder.load_state_dict(torch.load(opt.encoder_path, map_location='cpu'))
    for p in encoder.parameters():
        p.requires_grad = False
    encoder.eval().cuda()

    trainer = SupervisedTrainer(lloss=lloss, bloss=bloss, batch_size=opt.batch_size,
                                checkpoint_every=opt.checkpoint_every, print_every=opt.print_every,
                                expt_dir=opt.expt_dir, train_cap_lang=train_cap_lang,
                                train_label_lang=train_label_lang, x_mean_std=x_mean_std, y_mean_std=y_mean_std,
                                w_mean_std=w_mean_std, r_mean_std=r_mean_std)
    trainer.train(encoder, decoder, train_tuples, num_epochs=opt.num_epochs, resume=opt.resume,
                  is_training=opt.is_training, rng=rng)
    return 0


def main(argv=None):
    opt = build_parser().parse_args(argv)
    logging.basicConfig(format='%(asctime)s %(name)-12s %(levelname)-8s %(message)s',
                        level=getattr(logging, opt.log_level.upper()))
    if opt.is_training:
        return train(opt)
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
