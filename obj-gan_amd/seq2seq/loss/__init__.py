from .loss import Perplexity, BBLoss
