"""Readers of the box generator's text inputs (reference box_generation/seq2seq/dataset/prepare_dataset.py, the parts
the sampling path uses): `input_<split>.txt` (caption, x, y, w, h and label sequences, tab-separated),
`filenames_<split>.txt` (one image key per caption) and `mean_std_<split>.txt` (mean and std of x, y, w, w/h ratio).

Captions are tokenised with re.findall(r'\\w+', ...) in place of nltk's RegexpTokenizer(r'\\w+') (nltk is not a
dependency here); the two are not pinned against each other by a test."""
import collections
import re

import numpy as np


class Lang(object):
    """a vocabulary: word2index / index2word / word2count"""

    def __init__(self, name):
        self.name = name
        self.word2index = {"<pad>": 0, "<sos>": 1, "<eos>": 2, "<unk>": 3}
        self.index2word = {0: "<pad>", 1: "<sos>", 2: "<eos>", 3: "<unk>"}
        self.word2count = {w: 0 for w in self.word2index}
        self.n_words = 4

    def set_word2index(self, word2index):
        self.word2index = word2index
        self.n_words = len(word2index)

    def set_index2word(self, index2word):
        self.index2word = index2word

    def reset_word2count(self):
        self.word2count = {w: 0 for w in self.word2index}


def normalize_string(s):
    """lower-cased \\w+ tokens, non-ASCII characters dropped, empty tokens skipped"""
    tokens = re.findall(r'\w+', s.replace("\ufffd\ufffd", " ").lower())
    tokens = [t.encode('ascii', 'ignore').decode('ascii') for t in tokens]
    return [t for t in tokens if t]


def read_langs(filename):
    """-> (caption Lang, label Lang, [[tokens, xs, ys, ws, hs, labels]] with the five sequences as strings)"""
    with open(filename) as f:
        lines = f.read().strip().split('\n')
    tuples = []
    for line in lines:
        cap, x, y, w, h, label = line.split('\t')
        tuples.append([normalize_string(cap), x, y, w, h, label])
    return Lang('caption'), Lang('label'), tuples


def read_mean_std(filename):
    with open(filename) as f:
        rows = [tuple(float(v) for v in ln.split(' ')) for ln in f.read().strip().split('\n')[:4]]
    return rows[0], rows[1], rows[2], rows[3]


def prepare_test_data(dev_path, mean_std_path, max_len, min_len, train_cap_word2index, train_cap_index2word,
                      train_label_word2index, train_label_index2word, dev_filename_path):
    """the captions of a split with the vocabularies of a checkpoint; like the reference, max_len / min_len are
    accepted and no caption is filtered on the sampling path"""
    with open(dev_filename_path) as f:
        keys = f.read().strip().split('\n')
    x_mean_std, y_mean_std, w_mean_std, r_mean_std = read_mean_std(mean_std_path)
    cap_lang, label_lang, tuples = read_langs(dev_path)
    cap_lang.set_word2index(train_cap_word2index)
    cap_lang.set_index2word(train_cap_index2word)
    cap_lang.reset_word2count()
    label_lang.set_word2index(train_label_word2index)
    label_lang.set_index2word(train_label_index2word)
    label_lang.reset_word2count()
    return cap_lang, label_lang, tuples, x_mean_std, y_mean_std, w_mean_std, r_mean_std, keys


def get_class_sta(train_path, gaussian_dict_path):
    """{category id: (mean, std) of its per-image count} over the training layouts, saved with np.save"""
    counts = {}
    for item in read_langs(train_path)[2]:
        for label, n in collections.Counter(int(v) for v in item[5].split(' ')).items():
            counts.setdefault(label, []).append(n)
    np.save(gaussian_dict_path, {label: (np.mean(np.array(v)), np.std(np.array(v))) for label, v in counts.items()})


def indexes_from_sentence(lang, sentence):
    """ids of the known words, framed by <sos> / <eos> where the vocabulary has them"""
    words = sentence if isinstance(sentence, list) else sentence.split(' ')
    seq = [lang.word2index[w] for w in words if w in lang.word2index]
    if "<sos>" in lang.word2index:
        seq.insert(0, lang.word2index["<sos>"])
    if "<eos>" in lang.word2index:
        seq.append(lang.word2index["<eos>"])
    return seq
