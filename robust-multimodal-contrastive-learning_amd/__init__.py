"""rmcl_amd: MI355X-native hot path of the RMCL training step behind the reference's
``vilt.modules.ViLTransformerSS`` / ``training_step`` API.  All compute runs in
``lib/librmcl_hip.so`` (hand-written HIP for gfx950, C ABI in ``include/rmcl.h``); PyTorch is
used for device memory, streams and ``torch.distributed`` only.  There is no CPU fallback:
importing :mod:`rmcl_amd.runtime` fails loudly when the HIP library is missing."""
__version__ = "0.1.0"


def __getattr__(name):
    # ``from rmcl_amd import Predictor``: resolved on first use, so that importing the package alone still loads neither torch nor the library
    if name == "Predictor":
        from .predict import Predictor
        return Predictor
    if name == "RobustEval":
        from .robust import RobustEval
        return RobustEval
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
