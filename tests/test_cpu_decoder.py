"""CPU: the host side of toc3d_amd.PETRTemporalTransformer (state-dict names, config family, documented exceptions) and the plain-torch
restatement of the decoder (tests/decoder_cases.py) that pins tests/golden/decoder_tiny.npz -- output of the REAL reference (tools/gen_golden_decoder.py) -- to something
checkable where the reference does not exist.  tests/test_gpu_decoder.py uses the same restatement as its control."""
import json
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from decoder_cases import restated_decoder
from support import rel_max
from toc3d_amd import synth


def test_state_dict_names_and_strict_load(golden_dir):
    spec = json.load(open(os.path.join(golden_dir, "decoder_state_dict_spec.json")))
    for tag, sizes in (("tiny", synth.DECODER_TINY), ("full", synth.DECODER_FULL)):
        m = toc3d_amd.PETRTemporalTransformer(**{k: v for k, v in synth.decoder_cfg(**sizes).items() if k != "type"})
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec[tag]
        assert list(m.state_dict()) == list(spec[tag])                                  # the reference's order too
        res = m.load_state_dict(synth.decoder_state_dict(sizes), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    assert "decoder.layers.5.ffns.0.layers.0.0.weight" in spec["full"] and spec["full"]["decoder.layers.0.attentions.1.attn.in_proj_weight"] == [768, 256]


def test_registry_builds_the_class_from_the_shipped_config():
    cfg = dict(type="PETRTemporalTransformer",                                          # projects/configs/ToC3D/ToC3D_faster.py:114-139, verbatim
               decoder=dict(type="PETRTransformerDecoder", return_intermediate=True, num_layers=6,
                            transformerlayers=dict(type="PETRTemporalDecoderLayer",
                                                   attn_cfgs=[dict(type="MultiheadAttention", embed_dims=256, num_heads=8, dropout=0.1),
                                                              dict(type="PETRMultiheadAttention", embed_dims=256, num_heads=8, dropout=0.1)],
                                                   feedforward_channels=2048, ffn_dropout=0.1, with_cp=True,
                                                   operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm"))))
    assert "PETRTemporalTransformer" in toc3d_amd.TRANSFORMER.module_dict
    m = toc3d_amd.build_transformer(cfg)
    assert isinstance(m, toc3d_amd.PETRTemporalTransformer)
    assert (m.num_layers, m.embed_dims, m.num_heads, m.feedforward_channels) == (6, 256, 8, 2048)
    assert m.precision == "fp32x3" and m.encoder is None and m.cross is False
    assert cfg == synth.decoder_cfg(**synth.DECODER_FULL)                               # the seeded config maker hands out the same block


def _cfg(**over):
    cfg = {k: v for k, v in synth.decoder_cfg(**synth.DECODER_FULL).items() if k != "type"}
    lay = cfg["decoder"]["transformerlayers"]
    for k, v in over.items():
        if k in ("encoder", "precision"):
            cfg[k] = v
        elif k == "attn1_type":
            lay["attn_cfgs"][1]["type"] = v
        elif k == "num_heads":
            for a in lay["attn_cfgs"]:
                a["num_heads"] = v
        elif k == "return_intermediate":
            cfg["decoder"][k] = v
        else:
            lay[k] = v
    return cfg


@pytest.mark.parametrize("over", [dict(operation_order=("norm", "self_attn", "norm", "cross_attn", "norm", "ffn")), dict(attn1_type="PETRMultiheadFlashAttention"),
                                  dict(encoder=dict(type="PETRTransformerEncoder")), dict(num_heads=4), dict(return_intermediate=False)])
def test_configs_outside_the_family_are_refused(over):
    with pytest.raises(NotImplementedError, match="not implemented"):
        toc3d_amd.PETRTemporalTransformer(**_cfg(**over))


@pytest.mark.parametrize("precision", ["fp32", "fp32x6"])
def test_other_precisions_name_the_two_that_work(precision):
    with pytest.raises(NotImplementedError, match="'bf16' or 'fp32x3'"):
        toc3d_amd.PETRTemporalTransformer(**_cfg(precision=precision))


def test_masks_and_cpu_tensors_raise_the_documented_exceptions():
    sizes, shape = synth.DECODER_TINY, synth.DECODER_TINY_SHAPE
    m = toc3d_amd.build_transformer(synth.decoder_cfg(**sizes))
    inp = synth.decoder_inputs(sizes, shape)
    args = (inp["memory"], inp["tgt"], inp["query_pos"], inp["pos_embed"])
    with pytest.raises(RuntimeError, match="no CPU"):
        m(*args, None, inp["temp_memory"], inp["temp_pos"])

    class OnDevice(torch.Tensor):                     # is_cuda without a GPU: the checks that follow the device check never touch the data
        is_cuda = True
    fake = inp["memory"].as_subclass(OnDevice)
    mask = torch.zeros(32, 48, dtype=torch.bool)
    mask[3, 5] = True
    with pytest.raises(NotImplementedError, match="training-time denoising queries are out of scope"):
        m(fake, *args[1:], mask, inp["temp_memory"], inp["temp_pos"])
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        m(fake, *args[1:], None, inp["temp_memory"], inp["temp_pos"], mask=torch.zeros(2, 48, dtype=torch.bool))


@pytest.mark.parametrize("tag,with_temp", [("temp", True), ("notemp", False)])
def test_restatement_reproduces_the_reference_fixture(golden_dir, tag, with_temp):
    """<= 1e-5 relative (max-abs error / max-abs reference), the bound SURVEY.md section 8d sets for restatements: all of outs_dec and, per layer, the three
    post-norm intermediates."""
    g = np.load(os.path.join(golden_dir, "decoder_tiny.npz"))
    sizes, shape = synth.DECODER_TINY, synth.DECODER_TINY_SHAPE
    cap = {}
    with torch.no_grad():
        outs = restated_decoder(synth.decoder_state_dict(sizes), sizes, synth.decoder_inputs(sizes, shape, with_temp=with_temp), capture=cap)
    assert outs.shape == (2, 2, 32, 64) == g[f"{tag}_outs_dec"].shape
    errs = {"outs_dec": rel_max(outs, g[f"{tag}_outs_dec"])}
    for k, v in cap.items():
        errs[k] = rel_max(v, g[f"{tag}_{k}"])
    print(tag, {k: f"{e:.2e}" for k, e in errs.items()})
    assert len(errs) == 1 + 3 * sizes["num_layers"] and max(errs.values()) <= 1e-5, errs
    if with_temp:                                      # the two cases differ: the fixture exercises the temp_memory keys
        assert rel_max(g["temp_outs_dec"], g["notemp_outs_dec"]) > 1e-2
