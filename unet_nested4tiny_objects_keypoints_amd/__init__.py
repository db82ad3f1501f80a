"""MI355X-native UNet_Nested (UNet++) forward/backward path.

Drop-in for ``models.UNet_Nested`` of unanan/UNet_Nested4Tiny_Objects_Keypoints
(/root/reference/models/unet.py:204-300; resolved by name as trainer/trainer.py:337 does):

    import unet_nested4tiny_objects_keypoints_amd as models
    net = getattr(models, "UNet_Nested")().to("cuda")

All arithmetic of the path runs in the in-tree HIP library (csrc/ -> libunetpp_hip.so, C ABI in
include/unetpp_hip.h).  There is no CPU or eager-PyTorch fallback: using the model without the
library, or with CPU tensors, raises.
"""
from .unet import UNet, UNet_Nested, count_param  # noqa: F401
from .losses import (FocalLoss_BCE_2d, HeadDistillLoss, PenaltyReducedFocalLoss, TeacherDistillLoss,  # noqa: F401
                     TopKFocalLoss_BCE_2d)
from .step import train_step  # noqa: F401
from .engine import McMaps, pruned_parameters  # noqa: F401
from .targets import create_heatmap  # noqa: F401
from .keypoints import Heatmap  # noqa: F401
from .serving import GraphedForward  # noqa: F401
from .graph import GraphedTrainStep  # noqa: F401
from .optim import AdamW, AdaBound, SGDW, clip_grad_norm_  # noqa: F401
from .validate import validate_outputs, validate_step  # noqa: F401
from .averaging import WeightAverager  # noqa: F401
from .loader import Augment, DeviceLoader, affine_params, warp_batch  # noqa: F401
from .scene import CascadeSceneInference, SceneInference  # noqa: F401
from .detect import DetectionScore, Detections, PeakDetector, classes_from_pattern, evaluate  # noqa: F401
from .crops import ObjectPaste, PasteRows, SceneCrops, false_positive_centres  # noqa: F401
from .ignore import IgnoreMask, IgnoreRegions, IgnoreUnion  # noqa: F401

__all__ = ["UNet_Nested", "UNet", "count_param", "FocalLoss_BCE_2d", "train_step", "create_heatmap", "Heatmap",
           "GraphedForward", "GraphedTrainStep", "AdamW", "AdaBound", "SGDW", "validate_step",
           "validate_outputs", "WeightAverager", "clip_grad_norm_", "DeviceLoader", "Augment", "affine_params",
           "warp_batch", "SceneInference", "CascadeSceneInference", "PeakDetector", "Detections", "DetectionScore",
           "evaluate", "classes_from_pattern", "SceneCrops", "false_positive_centres", "TopKFocalLoss_BCE_2d",
           "pruned_parameters", "PenaltyReducedFocalLoss", "IgnoreRegions", "IgnoreMask", "IgnoreUnion", "McMaps", "ObjectPaste",
           "PasteRows", "HeadDistillLoss", "TeacherDistillLoss"]
