import os
import pickle

import torch

from seq2seq.models.DecoderRNN import DecoderRNN


class Checkpoint(object):
    """Reader of a checkpoint directory written by the reference's box-generator training (reference
    box_generation/seq2seq/util/checkpoint.py): `model.pt` is the pickled decoder module, the four vocabulary files are
    dill dumps of plain dicts, which pickle reads.  The pickled module resolves to this package's DecoderRNN (same
    module path), but only its state dict and constructor values are taken: `model` is a freshly built DecoderRNN.
    The optimizer state (`trainer_states.pt`) is not read; saving belongs to training, which is not built here."""

    CHECKPOINT_DIR_NAME = 'checkpoints'
    TRAINER_STATE_NAME = 'trainer_states.pt'
    MODEL_NAME = 'model.pt'
    CAP_WORD2INDEX = 'cap_word2index.pt'
    CAP_INDEX2WORD = 'cap_index2word.pt'
    LABEL_WORD2INDEX = 'label_word2index.pt'
    LABEL_INDEX2WORD = 'label_index2word.pt'

    def __init__(self, model, optimizer, epoch, step, cap_word2index, cap_index2word, label_word2index,
                 label_index2word, path=None):
        self.model = model
        self.optimizer = optimizer
        self.cap_word2index = cap_word2index
        self.cap_index2word = cap_index2word
        self.label_word2index = label_word2index
        self.label_index2word = label_index2word
        self.epoch = epoch
        self.step = step
        self._path = path

    @property
    def path(self):
        if self._path is None:
            raise LookupError("The checkpoint has not been saved.")
        return self._path

    def save(self, experiment_dir):
        raise NotImplementedError("checkpoints are written by box-generator training, which is out of scope here")

    @classmethod
    def load(cls, path):
        vocabs = []
        for name in (cls.CAP_WORD2INDEX, cls.CAP_INDEX2WORD, cls.LABEL_WORD2INDEX, cls.LABEL_INDEX2WORD):
            with open(os.path.join(path, name), 'rb') as fin:
                vocabs.append(pickle.load(fin))
        pickled = torch.load(os.path.join(path, cls.MODEL_NAME), map_location='cpu', weights_only=False)
        state = pickled.state_dict()
        d = pickled.__dict__
        if d.get('use_attention'):
            raise NotImplementedError("this checkpoint holds the attention variant of the decoder")
        model = DecoderRNN(vocabs[2], d['x_mean'], d['y_mean'], d['w_mean'], d['r_mean'], d['batch_size'],
                           d['max_length'], d['hidden_size'], d['gmm_comp_num'],
                           bidirectional=d['bidirectional_encoder'])
        model.load_state_dict(state)
        del pickled
        return Checkpoint(model=model, optimizer=None, epoch=None, step=None, cap_word2index=vocabs[0],
                          cap_index2word=vocabs[1], label_word2index=vocabs[2], label_index2word=vocabs[3], path=path)

    @classmethod
    def get_latest_checkpoint(cls, experiment_path):
        checkpoints_path = os.path.join(experiment_path, cls.CHECKPOINT_DIR_NAME)
        return os.path.join(checkpoints_path, sorted(os.listdir(checkpoints_path), reverse=True)[0])
