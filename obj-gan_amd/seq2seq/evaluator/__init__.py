from .evaluator import Evaluator
