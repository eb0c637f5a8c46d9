from .optim import Optimizer
