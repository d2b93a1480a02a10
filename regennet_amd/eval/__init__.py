from .auto_regressive import sample_auto_regressive  # noqa: F401
from .fid import calculate_activation_statistics, calculate_fid, calculate_frechet_distance  # noqa: F401
from .metrics import Evaluation, calculate_accuracy, calculate_diversity_multimodality  # noqa: F401
from .stgcn import STGCN, UnconstrainedSTGCN  # noqa: F401
from .gru import MotionDiscriminator, MotionDiscriminatorForFID, load_classifier, load_classifier_for_fid  # noqa: F401
from .t2m import EvaluatorMDMWrapper, MotionEncoderBiGRUCo, MovementConvEncoder, TextEncoderBiGRUCo  # noqa: F401

_A2M = ("A2MEvaluation", "A2MLoader", "calculate_accuracy_a2m")


def __getattr__(name):
    """The names of eval.a2m resolve on first use: `python -m regennet_amd.eval.a2m` must not find its module imported by the package already."""
    if name in _A2M:
        from . import a2m
        return getattr(a2m, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
