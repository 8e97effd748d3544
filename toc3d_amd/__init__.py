"""toc3d_amd -- MI355X (gfx950) implementation of the ToC3D / EVA-02 ViT backbone hot path.

Importing the package registers ``ToC3DEVAViT``, ``EVA_ViT`` (BACKBONES), ``CPFPN`` (NECKS) and ``PETRTemporalTransformer`` (TRANSFORMER) under the
reference's type names, like ``projects/mmdet3d_plugin`` does on import (``tools/test.py:133-145``).
"""
from .backbone import EVA_ViT, ToC3DEVAViT, ToC3DViTReturnType
from .neck import CPFPN
from .preprocess import prepare_images
from .memory import TemporalMemory
from .head_tokens import HeadTokenEmbedding
from .decoder import PETRTemporalTransformer
from .registry import BACKBONES, NECKS, TRANSFORMER, build_backbone, build_neck, build_transformer, register_all

register_all()

__all__ = ["ToC3DEVAViT", "EVA_ViT", "CPFPN", "ToC3DViTReturnType", "BACKBONES", "NECKS", "build_backbone", "build_neck", "prepare_images", "TemporalMemory", "HeadTokenEmbedding",
           "PETRTemporalTransformer", "TRANSFORMER", "build_transformer"]
