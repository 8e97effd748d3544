"""Generates the decoder fixtures from the REAL reference: tests/golden/decoder_tiny.npz, decoder_full.npz and decoder_state_dict_spec.json.

The reference's ``projects/mmdet3d_plugin/models/utils/petr_transformer.py`` is imported where it lies (``oracle.ref_harness.load_reference()`` for the
package skeleton, plus the stand-in modules below for what that file pulls from mmcv / mmdet) and its own ``PETRTemporalTransformer`` /
``PETRTransformerDecoder`` / ``PETRTemporalDecoderLayer`` / ``PETRMultiheadAttention`` are built from the shipped config block
(``toc3d_amd.synth.decoder_cfg``) with ``torch.nn.MultiheadAttention`` inside, and run in eval mode in f32 (and f64 for the arbiter) on seeded inputs.
Runs only where the reference tree exists; nothing of it is copied.

LIMITATION.  mmcv is not installed, so two pieces of arithmetic that live in mmcv are stood in here, with the parameter names of the mmcv classes:
  * mmcv's ``FFN`` (``add_identity=True``): ``x + Linear(ReLU(Linear(x)))`` under ``layers.0.0`` / ``layers.1``;
  * mmcv's ``MultiheadAttention`` (the ``self_attn`` of the config): ``identity + nn.MultiheadAttention(q + q_pos, k + k_pos, v)[0]`` -- the dataflow of the
    reference's own ``PETRMultiheadAttention.forward`` (:297-337), which is used as the stand-in with the attention weights dropped.
Everything else that computes (the layer's operation order and its cat of query and temp_memory, the cross-attention, the shared post_norm, the transposes of
``PETRTemporalTransformer.forward``) is the reference's code.  ``TransformerLayerSequence`` is stood in as a container only: with
``return_intermediate=True`` the reference's decoder runs its own loop over ``self.layers``.
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R              # noqa: E402
from toc3d_amd import synth                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL_ROWS = slice(0, None, 8)                    # decoder_full.npz keeps every 8th query (113 of 900 rows, fresh and propagated): committed files stay under 1 MiB


class _Reg:
    def __init__(self):
        self.d = {}

    def register_module(self, name=None, **_):
        def deco(cls):
            self.d[name or cls.__name__] = cls
            return cls
        return deco

    def build(self, cfg, default=None):
        cfg = copy.deepcopy(dict(cfg))           # as mmcv's build_from_cfg: the classes edit their config dicts
        return self.d[cfg.pop("type", default)](**cfg)


def load_petr_transformer():
    R.load_reference()                           # package skeleton + the mmcv / mmdet stand-ins of the backbone files
    ATT, LAYER, SEQ, TR = _Reg(), _Reg(), _Reg(), _Reg()

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

    class ConfigDict(dict):
        pass

    class FFN(BaseModule):                       # mmcv.cnn.bricks.transformer.FFN, num_fcs = 2, add_identity = True
        def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=None, ffn_drop=0.0, dropout_layer=None, add_identity=True, init_cfg=None, **kw):
            super().__init__(init_cfg)
            assert num_fcs == 2 and add_identity
            self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(ffn_drop)),
                                        nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))

        def forward(self, x, identity=None):
            return (x if identity is None else identity) + self.layers(x)

    class TransformerLayerSequence(BaseModule):  # container: builds num_layers copies of the layer config
        def __init__(self, transformerlayers=None, num_layers=None, init_cfg=None):
            super().__init__(init_cfg)
            self.num_layers = num_layers
            self.layers = nn.ModuleList([LAYER.build(transformerlayers) for _ in range(num_layers)])
            self.embed_dims, self.pre_norm = self.layers[0].embed_dims, self.layers[0].pre_norm

    deco = lambda *a, **k: (lambda f: f)
    sm = sys.modules
    R._mod("mmcv.cnn.bricks")
    R._mod("mmcv.cnn.bricks.transformer", BaseTransformerLayer=BaseModule, TransformerLayerSequence=TransformerLayerSequence,
           build_transformer_layer_sequence=lambda cfg: SEQ.build(cfg), build_attention=lambda cfg: ATT.build(cfg),
           build_feedforward_network=lambda cfg, default=None: FFN(**{k: v for k, v in cfg.items() if k != "type"}))
    R._mod("mmcv.cnn.bricks.drop", build_dropout=lambda cfg: nn.Dropout(cfg.get("drop_prob", 0.0)))
    R._mod("mmcv.cnn.bricks.registry", ATTENTION=ATT, TRANSFORMER_LAYER=LAYER, TRANSFORMER_LAYER_SEQUENCE=SEQ)
    R._mod("mmcv.utils", deprecated_api_warning=deco, ConfigDict=ConfigDict)
    R._mod("mmcv.runner.base_module", BaseModule=BaseModule)
    R._mod("mmdet.models.utils.builder", TRANSFORMER=TR)
    sm["mmcv.cnn"].build_norm_layer = lambda cfg, dims: ("ln", nn.LayerNorm(dims))
    sm["mmcv.cnn"].xavier_init = None
    sm["mmcv.runner"].BaseModule = BaseModule
    import importlib
    pt = importlib.import_module("projects.mmdet3d_plugin.models.utils.petr_transformer")

    class MultiheadAttention(pt.PETRMultiheadAttention):      # mmcv's class of that name: same dataflow, returns the tensor alone
        def forward(self, *a, **k):
            return super().forward(*a, **k)[0]
    ATT.d["MultiheadAttention"] = MultiheadAttention
    return pt, TR


def build_reference(TR, sizes, sd):
    m = TR.build(synth.decoder_cfg(**sizes))
    m.load_state_dict(sd, strict=True)
    return m.eval()


def run(m, inp, dtype=torch.float32, capture=None):
    c = lambda t: None if t is None else t.to(dtype)
    hooks = []
    if capture is not None:
        for i, layer in enumerate(m.decoder.layers):
            for n, norm in enumerate(layer.norms):
                hooks.append(norm.register_forward_hook(lambda mod, a, out, key=f"l{i}_norm{n}": capture.__setitem__(key, out.detach().transpose(0, 1).float().numpy())))
    with torch.no_grad():
        B, Nq = inp["query_pos"].shape[:2]
        Nkeys = Nq + (0 if inp["temp_memory"] is None else inp["temp_memory"].shape[1])
        masks = torch.zeros(Nq, Nkeys, dtype=torch.bool)     # streampetr_head.py:643-647 at eval: all False
        outs, mem, _ = m(c(inp["memory"]), c(inp["tgt"]), c(inp["query_pos"]), c(inp["pos_embed"]), masks, c(inp["temp_memory"]), c(inp["temp_pos"]))
    for h in hooks:
        h.remove()
    return outs


def main():
    pt, TR = load_petr_transformer()
    spec = {}
    # ---- tiny: both cases, all of outs_dec and the three post-norm intermediates of every layer
    sizes, shape = synth.DECODER_TINY, synth.DECODER_TINY_SHAPE
    sd = synth.decoder_state_dict(sizes)
    m = build_reference(TR, sizes, sd)
    spec["tiny"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert type(m.decoder.layers[0].attentions[1].attn) is nn.MultiheadAttention
    out = {}
    for tag, with_temp in (("temp", True), ("notemp", False)):
        cap = {}
        o = run(m, synth.decoder_inputs(sizes, shape, with_temp=with_temp), capture=cap)
        out[f"{tag}_outs_dec"] = o.numpy()
        out.update({f"{tag}_{k}": v for k, v in cap.items()})
    np.savez_compressed(os.path.join(GOLDEN, "decoder_tiny.npz"), **out)
    print("decoder_tiny.npz", {k: v.shape for k, v in out.items() if k.endswith("outs_dec")})
    # ---- full: the shipped sizes; f32 outs_dec and the last layer of the f64 run of the same modules, on the FULL_ROWS subset of the queries
    sizes, shape = synth.DECODER_FULL, synth.DECODER_FULL_SHAPE
    sd = synth.decoder_state_dict(sizes)
    m = build_reference(TR, sizes, sd)
    spec["full"] = {k: list(v.shape) for k, v in m.state_dict().items()}
    inp = synth.decoder_inputs(sizes, shape)
    o32 = run(m, inp)
    o64 = run(m.double(), inp, torch.float64)
    print("f32 vs f64, per layer (max-abs / max-abs):", [float((o32[l].double() - o64[l]).abs().max() / o64[l].abs().max()) for l in range(o32.shape[0])])
    rows = np.arange(o32.shape[2])[FULL_ROWS]
    np.savez_compressed(os.path.join(GOLDEN, "decoder_full.npz"), rows=rows.astype(np.int32), outs_dec=o32[:, :, rows].numpy(), last_f64=o64[-1][:, rows].numpy())
    json.dump(spec, open(os.path.join(GOLDEN, "decoder_state_dict_spec.json"), "w"), indent=1)
    for f in ("decoder_tiny.npz", "decoder_full.npz", "decoder_state_dict_spec.json"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
