"""medtok_amd -- MI355X-native vector-quantisation hot path of MedTok.

Host side: Python classes mirroring the reference's VQ interfaces
(vector_quantization_soft_one_new.py, norm_ema_quantizer.py, loss.py and the
quantize call sites of tokenizer.py / inference.py).  Device side: hand-written
gfx950 kernels behind the C ABI in include/medtok_vq.h, bound with ctypes.
"""
__version__ = "0.1.0"

__all__ = ["MedTokEmbedding"]


def __getattr__(name):
    # (on first use: importing the package alone stays free of torch)
    if name == "MedTokEmbedding":
        from .embedding import MedTokEmbedding
        return MedTokEmbedding
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
