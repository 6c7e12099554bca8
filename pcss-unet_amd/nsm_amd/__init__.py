"""nsm_amd — MI355X-native (gfx950) hot path of the PCSS-Unet Neural Shadow
Mapping U-Net: forward, backward, losses and train-step tail on hand-written
HIP kernels (libnsm.so), behind the reference's Python surface.

Importing this package loads libnsm.so and fails loudly if it is missing.
"""
from ._lib import LIB_PATH, NsmError, lib  # noqa: F401  (loads the HIP library)
from .unet import DoubleConv, Unet, reserve_side_stream  # noqa: F401
from .losses import (CustomLoss, EnhancedCustomLoss, L1Loss, PerturbationLoss,  # noqa: F401
                     detail_loss, detail_terms, l1_loss, measure_temporal_instability, ssim,
                     ssim_loss)
from .temporal import (TemporalInstability, reproject,  # noqa: F401
                       temporal_instability_terms)
from .taa import TemporalAA, taa_resolve, temporal_aa  # noqa: F401
from .svgf import SVGF, atrous_filter, svgf, svgf_accumulate, svgf_variance  # noqa: F401
from .optim import (FlatAdam, FlatAdamW, FlatSGD, allreduce_grads, flat_grad,  # noqa: F401
                    make_optimizer)
from .grad_scaler import GradScaler  # noqa: F401
from .infer import GraphedUnet  # noqa: F401
from .features import FeatureRecipe  # noqa: F401
from .extract import ExtractedUnet, FeatureExtractor  # noqa: F401
from .frames import (FramePipeline, compose_features, finish_frames,  # noqa: F401
                     prepare_frames)
from .patches import PatchSampler, patch_draws  # noqa: F401
from .sensitivity import (FeatureSensitivity, SensitivityResult,  # noqa: F401
                          feature_sensitivity)
from .stats import (ChannelStats, StatsResult, channel_stats, dataset_stats,  # noqa: F401
                    save_stats, stats_json)
from .step import GraphedTrainStep  # noqa: F401
from .validation import (ImageMetrics, MetricsResult, ValidationResult,  # noqa: F401
                         Validator, image_metrics, validate)
from .vgg import MultiLayerVGGLoss  # noqa: F401

__version__ = "0.1.0"
