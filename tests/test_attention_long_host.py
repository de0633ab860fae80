"""CPU: the host side of attention beyond 288 tokens -- the architecture names that need it, the gate of the hand-written
block chain, the limit Python and the header agree on, and the new switch in the header, the binding and the library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "lemon_hip.h")).read()


def test_336px_architecture_names():
    from lemon_amd.clip import ClipConfig
    ref = ClipConfig.named("vit-l-14")
    for name in ("vit-l-14-336", "vit-large-patch14-336", "l14-336", "openai/clip-vit-large-patch14-336", "ViT_L_14_336"):
        c = ClipConfig.named(name)
        assert (c.image_size, c.patch_size, c.embed_dim) == (336, 14, 768), name
        assert c.vision == ref.vision and c.text == ref.text and c.context_length == 77, name
        assert (c.image_size // c.patch_size) ** 2 + 1 == 577
    b = ClipConfig.named("vit-b-16-384")
    b16 = ClipConfig.named("vit-b-16")
    assert (b.image_size, b.patch_size, b.embed_dim) == (384, 16, 512) and b.vision == b16.vision and b.text == b16.text
    assert (b.image_size // b.patch_size) ** 2 + 1 == 577
    assert ClipConfig.named("vit-l-14").image_size == 224          # the existing names keep their meaning
    with pytest.raises(ValueError):
        ClipConfig.named("vit-l-14-448")


def test_the_block_chain_accepts_577_tokens_at_head_dim_64_only():
    from lemon_amd import ops
    assert ops.block_fused_supported(1024, 4096, 16, 577)
    assert ops.block_fused_supported(768, 3072, 12, 577) and ops.block_fused_supported(512, 2048, 8, 512)
    assert ops.block_fused_supported(1024, 4096, 16, ops.ATTENTION_MAX_SEQ)
    assert not ops.block_fused_supported(1024, 4096, 16, ops.ATTENTION_MAX_SEQ + 1)
    assert not ops.block_fused_supported(1280, 5120, 16, 577)      # head_dim 80 (ViT-H): the SDPA fallback stays
    assert ops.block_fused_supported(1024, 4096, 16, 257)


def test_python_limit_is_the_headers():
    from lemon_amd import _lib, ops
    m = re.search(r"#define\s+LEMON_ATTENTION_MAX_SEQ\s+(\d+)", _header())
    assert m, "include/lemon_hip.h must state LEMON_ATTENTION_MAX_SEQ"
    assert ops.ATTENTION_MAX_SEQ == _lib.ATTENTION_MAX_SEQ == int(m.group(1)) >= 4096
    assert "seq_len <= LEMON_ATTENTION_MAX_SEQ" in _header()


def test_stream_min_switch_is_declared_bound_and_exported():
    from lemon_amd import _lib
    assert re.search(r"\bint\s+lemon_attention_set_stream_min\s*\(\s*int\s+seq_len\s*\)\s*;", _header())
    assert "lemon_attention_set_stream_min" in _lib.EXPORTS
    assert os.path.exists(_lib.SO_PATH), "liblemon_hip.so is not built (python -m lemon_amd.build)"
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "lemon_attention_set_stream_min")
    bound = _lib.load()
    assert bound.lemon_attention_set_stream_min.argtypes == [ctypes.c_int]
    # the switch is host state: usable without a device.  Default 288, range 64 .. 288, refused values change nothing
    assert bound.lemon_attention_set_stream_min(64) == 288
    try:
        assert bound.lemon_attention_set_stream_min(63) < 0 and bound.lemon_attention_set_stream_min(289) < 0
        assert b"64 .. 288" in bound.lemon_last_error()
        assert bound.lemon_attention_set_stream_min(200) == 64
    finally:
        assert bound.lemon_attention_set_stream_min(288) == 200
