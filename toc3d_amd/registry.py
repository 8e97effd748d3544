"""Registry surface: ``ToC3DEVAViT`` / ``EVA_ViT`` on mmdet's BACKBONES, ``CPFPN`` on NECKS, ``PETRTemporalTransformer`` on TRANSFORMER, ``NMSFreeCoder`` on
BBOX_CODERS, ``StreamPETRHead`` and ``FocalHead`` on HEADS (the reference: ``@HEADS.register_module()``, ``dense_heads/streampetr_head.py:32``,
``dense_heads/focal_head.py:20``), ``Petr3D`` on DETECTORS
(``@DETECTORS.register_module()``, ``detectors/petr3d.py:23``).

The reference registers its classes with ``@BACKBONES.register_module()`` (``toc3d_eva_vit.py:25``,
``eva_vit.py:270``), ``@NECKS.register_module()`` (``cp_fpn.py:15``) and ``@TRANSFORMER.register_module()``
(``utils/petr_transformer.py:430``), its box coder with ``@BBOX_CODERS.register_module()`` (``core/bbox/coders/nms_free_coder.py:8``); configs name them
by ``type=``.
When mmdet is importable the same names are registered there (``force=True`` so this package can shadow the
reference plugin); otherwise a shim registry with the same ``register_module()/build(cfg)`` API is used.
"""
from __future__ import annotations


class _ShimRegistry:
    def __init__(self, name):
        self.name = name
        self.module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        def deco(cls):
            self.module_dict[name or cls.__name__] = cls
            return cls
        return deco(module) if module is not None else deco

    def get(self, key):
        return self.module_dict.get(key)

    def build(self, cfg, **default_args):
        cfg = dict(cfg)
        cls = self.module_dict[cfg.pop("type")]
        cfg.update(default_args)
        return cls(**cfg)


try:  # pragma: no cover - mmdet is not installed in the build image
    from mmdet.models.builder import BACKBONES, NECKS
    HAVE_MMDET = True
except Exception:  # noqa: BLE001
    BACKBONES, NECKS = _ShimRegistry("backbone"), _ShimRegistry("neck")
    HAVE_MMDET = False
try:  # pragma: no cover
    from mmdet.models.utils.builder import TRANSFORMER
except Exception:  # noqa: BLE001
    TRANSFORMER = _ShimRegistry("transformer")
try:  # pragma: no cover
    from mmdet.core.bbox.builder import BBOX_CODERS
except Exception:  # noqa: BLE001
    BBOX_CODERS = _ShimRegistry("bbox_coder")
try:  # pragma: no cover
    from mmdet.models.builder import HEADS
except Exception:  # noqa: BLE001
    HEADS = _ShimRegistry("head")
try:  # pragma: no cover
    from mmdet.models.builder import DETECTORS
except Exception:  # noqa: BLE001
    DETECTORS = _ShimRegistry("detector")


def register_all():
    from .backbone import EVA_ViT, ToC3DEVAViT
    from .decoder import PETRTemporalTransformer
    from .detector import Petr3D
    from .focal_head import FocalHead
    from .head import StreamPETRHead
    from .head_outputs import NMSFreeCoder
    from .neck import CPFPN
    for reg, cls in ((BACKBONES, ToC3DEVAViT), (BACKBONES, EVA_ViT), (NECKS, CPFPN), (TRANSFORMER, PETRTemporalTransformer), (BBOX_CODERS, NMSFreeCoder),
                     (HEADS, StreamPETRHead), (HEADS, FocalHead), (DETECTORS, Petr3D)):
        try:
            reg.register_module(name=cls.__name__, force=True, module=cls)
        except TypeError:
            reg.register_module()(cls)


def build_backbone(cfg, **kw):
    return BACKBONES.build(cfg, **kw) if not HAVE_MMDET else BACKBONES.build(dict(cfg, **kw))


def build_neck(cfg, **kw):
    return NECKS.build(cfg, **kw) if not HAVE_MMDET else NECKS.build(dict(cfg, **kw))


def build_transformer(cfg, **kw):
    return TRANSFORMER.build(cfg, **kw) if isinstance(TRANSFORMER, _ShimRegistry) else TRANSFORMER.build(dict(cfg, **kw))


def build_bbox_coder(cfg, **kw):
    return BBOX_CODERS.build(cfg, **kw) if isinstance(BBOX_CODERS, _ShimRegistry) else BBOX_CODERS.build(dict(cfg, **kw))


def build_head(cfg, **kw):
    return HEADS.build(cfg, **kw) if isinstance(HEADS, _ShimRegistry) else HEADS.build(dict(cfg, **kw))


def build_detector(cfg, **kw):
    return DETECTORS.build(cfg, **kw) if isinstance(DETECTORS, _ShimRegistry) else DETECTORS.build(dict(cfg, **kw))
