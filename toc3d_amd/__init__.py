"""toc3d_amd -- MI355X (gfx950) implementation of the ToC3D / EVA-02 ViT backbone hot path.

Importing the package registers ``ToC3DEVAViT``, ``EVA_ViT`` (BACKBONES), ``CPFPN`` (NECKS), ``PETRTemporalTransformer`` (TRANSFORMER), ``NMSFreeCoder``
(BBOX_CODERS), ``StreamPETRHead`` and ``FocalHead`` (HEADS) and ``Petr3D`` (DETECTORS) under the reference's type names, like ``projects/mmdet3d_plugin`` does on import (``tools/test.py:133-145``).
"""
from .backbone import EVA_ViT, ToC3DEVAViT, ToC3DViTReturnType
from .neck import CPFPN
from .preprocess import ResizeCropFlipRotImage, prepare_images, resample_tables
from .memory import TemporalMemory
from .head_tokens import HeadTokenEmbedding
from .decoder import PETRTemporalTransformer
from .head_outputs import HeadOutputs, NMSFreeCoder
from .head_queries import HeadQueries
from .head import StreamPETRHead
from .focal_head import FocalHead
from .detector import Petr3D, build_vis_detector
from .token_vis import TokenVis, token_selection_vis
from .box_vis import BoxVis
from .nusc_results import NuScenesResults
from .tracking import HungarianPubTracker, PubTracker, build_tracker
from .registry import (BACKBONES, BBOX_CODERS, DETECTORS, HEADS, NECKS, TRANSFORMER, build_backbone, build_bbox_coder, build_detector, build_head, build_neck,
                       build_transformer, register_all)

register_all()

__all__ = ["ToC3DEVAViT", "EVA_ViT", "CPFPN", "ToC3DViTReturnType", "BACKBONES", "NECKS", "build_backbone", "build_neck", "prepare_images", "ResizeCropFlipRotImage", "resample_tables", "TemporalMemory", "HeadTokenEmbedding",
           "PETRTemporalTransformer", "TRANSFORMER", "build_transformer", "HeadOutputs", "HeadQueries", "NMSFreeCoder", "BBOX_CODERS", "build_bbox_coder",
           "StreamPETRHead", "FocalHead", "HEADS", "build_head", "Petr3D", "DETECTORS", "build_detector", "build_vis_detector",
           "TokenVis", "token_selection_vis", "BoxVis", "NuScenesResults", "PubTracker", "HungarianPubTracker", "build_tracker"]
