"""MI355X-native Hierarchical Parallel Co-Attention path (drop-in for the reference's
``--model attention`` hot path, /root/reference/model.py:337-397).

Host side is Python on PyTorch-ROCm (device memory, streams, torch.distributed); the compute
is a C-ABI HIP library (``include/coattn.h``, sources in ``csrc/``) loaded through ctypes.
There is no CPU fallback: using the co-attention op without the HIP library or on CPU
tensors raises.
"""
from . import _lib  # noqa: F401
from ._lib import RangeError, check_range  # noqa: F401
from .coattention import ParallelCoAttention, coattention, native_features  # noqa: F401
from .alternating import AlternatingCoAttention  # noqa: F401
from .loss import CrossEntropyLoss, SoftTargetLoss, cross_entropy, soft_target_loss, vqa_score  # noqa: F401
from .head import answer_head  # noqa: F401
from .optim import HipAdam  # noqa: F401
from .lstm import sentence_lstm  # noqa: F401
from . import gru  # noqa: F401
from .gru import question_gru  # noqa: F401
from . import fusion  # noqa: F401
from .fusion import fusion_head  # noqa: F401
from . import embedding  # noqa: F401
from .embedding import word_embedding  # noqa: F401
from . import dropout  # noqa: F401
from .dropout import DropoutState, feature_dropout, rank_seed  # noqa: F401
from . import features  # noqa: F401
from .features import FeatureTable, gather_features  # noqa: F401
from . import overlay  # noqa: F401
from .overlay import render_attention  # noqa: F401
from . import preprocess  # noqa: F401
from .preprocess import ImagePreprocessor, preprocess_host  # noqa: F401

__all__ = ["word_embedding", "embedding","ParallelCoAttention", "AlternatingCoAttention", "coattention", "native_features", "answer_head", "cross_entropy", "CrossEntropyLoss", "soft_target_loss",
           "SoftTargetLoss", "vqa_score", "HipAdam", "sentence_lstm", "gru", "question_gru", "fusion", "fusion_head", "_lib",
           "check_range", "RangeError", "dropout", "DropoutState", "feature_dropout", "rank_seed",
           "features", "FeatureTable", "gather_features",
           "overlay", "render_attention", "preprocess", "ImagePreprocessor", "preprocess_host"]
