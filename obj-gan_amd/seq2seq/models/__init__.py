from .PreEncoderRNN import PreEncoderRNN
from .DecoderRNN import DecoderRNN
