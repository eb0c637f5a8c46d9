import os
import pickle

import torch

from seq2seq.models.DecoderRNN import DecoderRNN


class Checkpoint(object):
    """A checkpoint directory of the box generator's training (reference box_generation/seq2seq/util/checkpoint.py):
    `model.pt` is the pickled decoder module, the four vocabulary files are dumps of plain dicts (the reference writes
    them with dill, `save` here with pickle; pickle reads both).  On load the pickled module resolves to this package's
    DecoderRNN (same module path), but only its state dict and constructor values are taken: `model` is a freshly
    built DecoderRNN.  `trainer_states.pt` holds epoch, step and the optimizer (Adam moments and step count); `load`
    restores them from a directory `save` wrote and leaves them None for one the reference wrote."""

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

    def save(self, experiment_dir, name=None):
        """writes <experiment_dir>/checkpoints/<name or the local time as Y_M_D_H_M_S>/ in the reference's layout:
        model.pt (the pickled decoder module, on the CPU), trainer_states.pt {'epoch', 'step', 'optimizer': the
        seq2seq.optim.Optimizer with its Adam moments and step count} and the four vocabulary files.  -> the path"""
        import copy
        import shutil
        import time
        name = time.strftime('%Y_%m_%d_%H_%M_%S', time.localtime()) if name is None else name
        path = self._path = os.path.join(experiment_dir, self.CHECKPOINT_DIR_NAME, name)
        if os.path.exists(path):
            shutil.rmtree(path)
        os.makedirs(path)
        model = self.model
        packed, model._packed = model._packed, None              # the kernel-layout cache is not part of the module
        try:
            cpu_model = copy.deepcopy(model).cpu()
        finally:
            model._packed = packed
        optimizer = None
        if self.optimizer is not None:
            # the optimizer is stored as its state dict (parameters by position) next to its settings: a pickled
            # torch optimizer would drag device tensors and the live parameters along
            inner = self.optimizer.optimizer
            state = copy.deepcopy(inner.state_dict())
            for s in state['state'].values():
                for k, v in s.items():
                    if torch.is_tensor(v):
                        s[k] = v.cpu()
            optimizer = {'class': type(inner).__name__, 'state_dict': state,
                         'max_grad_norm': self.optimizer.max_grad_norm}
        torch.save({'epoch': self.epoch, 'step': self.step, 'optimizer': optimizer},
                   os.path.join(path, self.TRAINER_STATE_NAME))
        torch.save(cpu_model, os.path.join(path, self.MODEL_NAME))
        for fname, vocab in ((self.CAP_WORD2INDEX, self.cap_word2index), (self.CAP_INDEX2WORD, self.cap_index2word),
                             (self.LABEL_WORD2INDEX, self.label_word2index),
                             (self.LABEL_INDEX2WORD, self.label_index2word)):
            with open(os.path.join(path, fname), 'wb') as fout:
                pickle.dump(vocab, fout)
        return path

    @classmethod
    def _load_trainer_state(cls, path, model):
        """-> (optimizer, epoch, step) of trainer_states.pt; (None, None, None) where the file is absent or holds a
        pickled reference optimizer (a directory the reference wrote: sampling needs none of it)"""
        from seq2seq.optim import Optimizer
        fname = os.path.join(path, cls.TRAINER_STATE_NAME)
        if not os.path.isfile(fname):
            return None, None, None
        try:
            st = torch.load(fname, map_location='cpu', weights_only=False)
        except (AttributeError, ImportError, pickle.UnpicklingError):
            # the reference pickles its optimizer OBJECT: classes this package does not have fail to resolve.  Any
            # other failure (a truncated or unreadable file) is an error and is raised.
            return None, None, None
        o = st.get('optimizer')
        optimizer = None
        if o is not None and not isinstance(o, dict):
            return None, None, None                      # a pickled reference optimizer that did resolve: not read
        if o is not None:
            inner = getattr(torch.optim, o['class'])(model.parameters())
            inner.load_state_dict(o['state_dict'])
            optimizer = Optimizer(inner, max_grad_norm=o['max_grad_norm'])
        return optimizer, st.get('epoch'), st.get('step')

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
        optimizer, epoch, step = cls._load_trainer_state(path, model)
        return Checkpoint(model=model, optimizer=optimizer, epoch=epoch, step=step, cap_word2index=vocabs[0],
                          cap_index2word=vocabs[1], label_word2index=vocabs[2], label_index2word=vocabs[3], path=path)

    @classmethod
    def get_latest_checkpoint(cls, experiment_path):
        checkpoints_path = os.path.join(experiment_path, cls.CHECKPOINT_DIR_NAME)
        return os.path.join(checkpoints_path, sorted(os.listdir(checkpoints_path), reverse=True)[0])
