"""CPU: the host side of attention at head dims 72 .. 128 -- the activation a checkpoint's configuration names, the ViT-H/14
architecture, the gate of the hand-written block chain under the head-dim switch, and the switch in the header, the binding
and the library."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lemon_hip.h")).read()


def _tiny_hf(hidden_act, seed=0):
    from transformers import CLIPConfig, CLIPModel
    cfg = CLIPConfig(projection_dim=32,
                     vision_config=dict(hidden_size=48, num_hidden_layers=2, num_attention_heads=4, intermediate_size=96,
                                        image_size=32, patch_size=8, hidden_act=hidden_act),
                     text_config=dict(hidden_size=40, num_hidden_layers=2, num_attention_heads=4, intermediate_size=80,
                                      vocab_size=300, max_position_embeddings=16, hidden_act=hidden_act,
                                      eos_token_id=2, bos_token_id=0, pad_token_id=1))     # legacy ids => argmax EOT pooling
    torch.manual_seed(seed)
    hf = CLIPModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in hf.named_parameters():
            # weights large enough that the two activations differ far beyond the tolerance below
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (0.02 if "embedding" in name else 2.0 * p[0].numel() ** -0.5))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return hf


def _unwrap(o):
    return o if torch.is_tensor(o) else o.pooler_output


def _inputs():
    g = torch.Generator().manual_seed(7)
    px = torch.randn(3, 3, 32, 32, generator=g)
    ids = torch.randint(3, 299, (4, 16), generator=g)
    ids[:, 0] = 0
    for i, n in enumerate((16, 3, 9, 12)):
        ids[i, n - 1] = 299                                    # EOT = the largest id, at ragged positions
        ids[i, n:] = 1
    return px, ids


def _ours(hf, cfg_dict, px, ids):
    from lemon_amd.clip import ClipConfig, LemonCLIP
    cfg = ClipConfig.from_hf_dict(cfg_dict)
    m = LemonCLIP(cfg).load_hf_state_dict(hf.state_dict()).eval()
    return cfg, (m.encode_image(px), m.encode_text(ids))


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_hidden_act_of_the_checkpoint_reaches_both_towers(act):
    hf = _tiny_hf(act)
    px, ids = _inputs()
    with torch.no_grad():
        ref = _unwrap(hf.get_image_features(pixel_values=px)), _unwrap(hf.get_text_features(input_ids=ids))
    cfg, got = _ours(hf, hf.config.to_dict(), px, ids)
    assert cfg.hidden_act == act
    for name, r, o in zip(("image", "text"), ref, got):
        d = float((o - r).abs().max())
        assert d <= 2e-5 * max(1.0, float(r.abs().max())), (act, name, d)
    # the two activations are told apart at this tolerance: the same weights under the other activation miss it, in both towers
    swapped = hf.config.to_dict()
    swapped["vision_config"]["hidden_act"] = swapped["text_config"]["hidden_act"] = "quick_gelu" if act == "gelu" else "gelu"
    _, wrong = _ours(hf, swapped, px, ids)
    for name, r, o in zip(("image", "text"), ref, wrong):
        assert float((o - r).abs().max()) > 1e-3 * float(r.abs().max()), (act, name)


def test_from_hf_dict_hidden_act_rules():
    from lemon_amd.clip import ClipConfig
    base = dict(vision_config={}, text_config={})
    assert ClipConfig.from_hf_dict(base).hidden_act == "quick_gelu" == ClipConfig().hidden_act
    both = dict(vision_config=dict(hidden_act="gelu"), text_config=dict(hidden_act="gelu"))
    assert ClipConfig.from_hf_dict(both).hidden_act == "gelu"
    with pytest.raises(ValueError):
        ClipConfig.from_hf_dict(dict(vision_config=dict(hidden_act="gelu"), text_config=dict(hidden_act="quick_gelu")))
    with pytest.raises(ValueError):
        ClipConfig.from_hf_dict(dict(vision_config=dict(hidden_act="relu"), text_config=dict(hidden_act="relu")))


def test_vit_h_14_architecture():
    from lemon_amd.clip import ClipConfig, TowerConfig
    for name in ("vit-h-14", "ViT_H_14", "h14"):
        c = ClipConfig.named(name)
        assert c.vision == TowerConfig(1280, 32, 16, 5120) and c.text == TowerConfig(1024, 24, 16, 4096), name
        assert (c.embed_dim, c.patch_size, c.image_size, c.hidden_act) == (1024, 14, 224, "gelu"), name
        assert c.vision.width // c.vision.heads == 80 and (c.image_size // c.patch_size) ** 2 + 1 == 257
    assert ClipConfig.named("vit-l-14").hidden_act == "quick_gelu"          # the existing names keep their meaning


def test_the_block_chain_accepts_head_dim_80_with_the_switch_on():
    from lemon_amd import ops
    assert ops.attention_head_dims() == 0, "the default is off"
    assert not ops.block_fused_supported(1280, 5120, 16, 257) and not ops.attention_supported(1280, 16, 257)
    assert ops.attention_supported(1024, 16, 257) and ops.fused_width_max() == 1024
    assert ops.set_attention_head_dims(1) == 0                 # host state: usable without a device
    try:
        assert ops.attention_head_dims() == 1
        assert ops.block_fused_supported(1280, 5120, 16, 257) and ops.block_fused_supported(1280, 5120, 16, 577)
        assert ops.block_fused_supported(1024, 4096, 16, 257) and ops.fused_width_max() == 2048
        assert ops.attention_supported(1408, 16, 257) and ops.attention_supported(1664, 16, 257)        # g/14: 88, bigG/14: 104
        assert not ops.block_fused_supported(1408, 6144, 16, 257)                                       # 1408 is no multiple of 256
        assert not ops.attention_supported(1280, 16, ops.ATTENTION_MAX_SEQ + 1)
        for width, heads in ((960, 16), (1088, 16), (2176, 16), (512, 16), (1290, 16)):                 # 60, 68, 136, 32, no integer
            assert not ops.attention_supported(width, heads, 257), (width, heads)
    finally:
        assert ops.set_attention_head_dims(0) == 1
    assert not ops.block_fused_supported(1280, 5120, 16, 257)


def test_head_dims_switch_is_declared_bound_and_exported():
    from lemon_amd import _lib
    assert re.search(r"\bint\s+lemon_attention_set_head_dims\s*\(\s*int\s+mode\s*\)\s*;", _header())
    assert re.search(r"\bint\s+lemon_attention_get_head_dims\s*\(\s*void\s*\)\s*;", _header())
    assert "lemon_attention_set_head_dims" in _lib.EXPORTS and "lemon_attention_get_head_dims" in _lib.EXPORTS
    assert os.path.exists(_lib.SO_PATH), "liblemon_hip.so is not built (python -m lemon_amd.build)"
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(raw, "lemon_attention_set_head_dims") and hasattr(raw, "lemon_attention_get_head_dims")
    bound = _lib.load()
    assert bound.lemon_attention_set_head_dims.argtypes == [ctypes.c_int]
    assert bound.lemon_attention_get_head_dims() == 0
    assert bound.lemon_attention_set_head_dims(2) == 0
    try:
        for bad in (3, -1, 64):
            assert bound.lemon_attention_set_head_dims(bad) < 0, bad
            assert b"mode must be 0, 1 or 2" in bound.lemon_last_error()
            assert bound.lemon_attention_get_head_dims() == 2      # a refused mode changes nothing
        assert bound.lemon_attention_set_head_dims(1) == 2
    finally:
        assert bound.lemon_attention_set_head_dims(0) == 1
