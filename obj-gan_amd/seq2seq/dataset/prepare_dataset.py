"""Readers of the box generator's text inputs and the batch maker of its training (reference
box_generation/seq2seq/dataset/prepare_dataset.py): `input_<split>.txt` (caption, x, y, w, h and label sequences, tab-separated),
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

    # ---- building and counting (training) ----------------------------------------------------------------------
    def index_words(self, sentence):
        """a space-separated label sequence: unseen words get the next free index, every word is counted"""
        for word in sentence.split(' '):
            index = self.word2index.setdefault(word, self.n_words)
            if index == self.n_words:
                self.index2word[index] = word
                self.n_words += 1
            self.word2count[word] = self.word2count.get(word, 0) + 1

    def index_cap_words(self, tokens):
        """a tokenised caption against a FIXED vocabulary: known words are counted, unknown ones ignored"""
        for word in tokens:
            if word in self.word2index:
                self.word2count[word] += 1

    def increase_seos_count(self):
        """one more sequence: <sos> and <eos> frame each of them"""
        for word in ("<sos>", "<eos>"):
            self.word2count[word] += 1

    def copy_dict(self, lang):
        """share another Lang's vocabulary (the same dict objects) and start its counts from zero"""
        self.word2index, self.index2word, self.n_words = lang.word2index, lang.index2word, lang.n_words
        self.reset_word2count()

    def copy_ext_dict(self, ixtoword, wordtoix):
        """take over an external vocabulary (the text encoder's), counts from zero"""
        self.set_word2index(wordtoix)
        self.set_index2word(ixtoword)
        self.reset_word2count()

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


def filter_tuples(tuples, max_len, min_len):
    return [item for item in tuples
            if min_len <= len(item[0]) <= max_len and min_len <= len(item[5]) <= max_len]


def prepare_data(train_path, dev_path, mean_std_path, max_len, min_len, ixtoword, wordtoix):
    """the training and dev captions with the caption vocabulary of the text encoder (ixtoword / wordtoix) and the
    label vocabulary indexed from the training layouts; word2count feeds the label weights.  Like the reference,
    max_len / min_len are accepted and nothing is filtered."""
    x_mean_std, y_mean_std, w_mean_std, r_mean_std = read_mean_std(mean_std_path)
    train_cap_lang, train_label_lang, train_tuples = read_langs(train_path)
    train_cap_lang.copy_ext_dict(ixtoword, wordtoix)
    for item in train_tuples:
        train_cap_lang.index_cap_words(item[0])
        train_label_lang.index_words(item[5])
        train_label_lang.increase_seos_count()
    dev_cap_lang, dev_label_lang, dev_tuples = read_langs(dev_path)
    dev_cap_lang.copy_dict(train_cap_lang)
    dev_label_lang.copy_dict(train_label_lang)
    for item in dev_tuples:
        dev_cap_lang.index_cap_words(item[0])
        dev_label_lang.index_words(item[5])
        dev_label_lang.increase_seos_count()
    return train_cap_lang, train_label_lang, train_tuples, dev_cap_lang, dev_label_lang, dev_tuples, \
        x_mean_std, y_mean_std, w_mean_std, r_mean_std


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


def nums_from_sentence(mean, std, sentence):
    """normalised values framed by a zero for <sos> and one for <eos>"""
    values = [0.0] * (len(sentence.split(' ')) + 2)
    for i, text in enumerate(sentence.split(' ')):
        values[i + 1] = (float(text) - mean) / std
    return values


def pad_seq(seq, max_length, pad_token):
    """extends `seq` in place to max_length with pad_token and returns it (longer sequences are left alone)"""
    seq.extend([pad_token] * (max_length - len(seq)))
    return seq


def random_batch(batch_size, tuples, cap_lang, label_lang, x_mean_std, y_mean_std, w_mean_std, r_mean_std,
                 is_training=0, select_index=None, rng=None, device=None):
    """a batch of (caption ids, caption lengths, labels, label lengths, x, y, w, r), sorted by caption length
    (descending) and zero padded, as tensors on `device` (the GPU when there is one).  is_training=1 draws batch_size
    items with random.choice (or rng.choice, an object with that method), otherwise item `select_index` is taken."""
    import random
    import torch
    if is_training:
        choice = random.choice if rng is None else rng.choice
        items = [choice(tuples) for _ in range(batch_size)]
    else:
        assert select_index is not None
        items = [tuples[select_index]]
    seqs = [(indexes_from_sentence(cap_lang, item[0]), indexes_from_sentence(label_lang, item[5]),
             nums_from_sentence(x_mean_std[0], x_mean_std[1], item[1]),
             nums_from_sentence(y_mean_std[0], y_mean_std[1], item[2]),
             nums_from_sentence(w_mean_std[0], w_mean_std[1], item[3]),
             nums_from_sentence(r_mean_std[0], r_mean_std[1], item[4])) for item in items]
    seqs = sorted(seqs, key=lambda p: len(p[0]), reverse=True)
    cap_seqs, label_seqs, x_seqs, y_seqs, w_seqs, r_seqs = zip(*seqs)
    cap_lengths = [len(s) for s in cap_seqs]
    label_lengths = [len(s) for s in label_seqs]
    n = max(label_lengths)
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    cap_var = torch.tensor([pad_seq(s, max(cap_lengths), 0) for s in cap_seqs], dtype=torch.long, device=device)
    label_var = torch.tensor([pad_seq(s, n, label_lang.word2index["<pad>"]) for s in label_seqs], dtype=torch.long,
                             device=device)
    x_var, y_var, w_var, r_var = (torch.tensor([pad_seq(s, n, 0) for s in q], dtype=torch.float32, device=device)
                                  for q in (x_seqs, y_seqs, w_seqs, r_seqs))
    return cap_var, cap_lengths, label_var, label_lengths, x_var, y_var, w_var, r_var
