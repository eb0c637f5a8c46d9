from .supervised_trainer import SupervisedTrainer, FusedBoxStep
