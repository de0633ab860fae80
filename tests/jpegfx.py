"""JPEG files written by PIL at test time for tests/test_jpeg_host.py and tests/test_gpu_jpeg.py: the accepted set (every case
must decode bit for bit like PIL and none may be declined) and the set the host pass must decline."""
import io
import os

import numpy as np
from PIL import Image

SHAPES = [(37, 53), (64, 80), (16, 16), (33, 5), (9, 4), (50, 3), (1, 1), (41, 67)]     # (width, height)


def pixels(w, h, rng, noise=False, channels=3):
    if noise:
        return rng.integers(0, 256, (h, w, channels), dtype=np.uint8).squeeze()
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 128 + 90 * np.sin(yy[..., None] / 7.0 + xx[..., None] / 11.0 + np.arange(channels))
    return np.clip(base + rng.normal(0, 12, (h, w, channels)), 0, 255).astype(np.uint8).squeeze()


def jpeg_bytes(px, **kw):
    b = io.BytesIO()
    (px if isinstance(px, Image.Image) else Image.fromarray(px)).save(b, "JPEG", **kw)
    return b.getvalue()


def accepted_cases(seed=0):
    """[(name, bytes)]: 8 shapes x subsampling 0/1/2 x quality 30/90 (sinusoid + noise) and 100 (uniform noise) = 72, then
    grayscale, optimize=True, restart markers by blocks and by rows, 640x480, 612x612, and 4 KB of EXIF / COM segments."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in SHAPES:
        for ss in (0, 1, 2):
            for q in (30, 90, 100):
                out.append((f"{w}x{h}_ss{ss}_q{q}", jpeg_bytes(pixels(w, h, rng, noise=q == 100), quality=q, subsampling=ss)))
    assert len(out) == 72
    out.append(("gray_41x67", jpeg_bytes(pixels(41, 67, rng, channels=1), quality=90)))
    out.append(("gray_1x1", jpeg_bytes(pixels(1, 1, rng, noise=True, channels=1).reshape(1, 1), quality=75)))
    out.append(("optimize", jpeg_bytes(pixels(64, 80, rng), quality=90, subsampling=2, optimize=True)))
    out.append(("optimize_q100", jpeg_bytes(pixels(37, 53, rng, noise=True), quality=100, subsampling=0, optimize=True)))
    out.append(("restart_blocks", jpeg_bytes(pixels(100, 75, rng), quality=90, subsampling=2, restart_marker_blocks=3)))
    out.append(("restart_rows", jpeg_bytes(pixels(100, 75, rng), quality=90, subsampling=1, restart_marker_rows=1)))
    out.append(("restart_many", jpeg_bytes(pixels(200, 75, rng), quality=50, subsampling=0, restart_marker_blocks=1)))
    out.append(("640x480", jpeg_bytes(pixels(640, 480, rng), quality=90, subsampling=2)))
    out.append(("612x612", jpeg_bytes(pixels(612, 612, rng), quality=90, subsampling=2)))
    exif = Image.Exif()
    exif[0x010E] = "x" * 2000          # ImageDescription
    exif[0x0131] = "lemon tests"       # Software
    out.append(("exif_com", jpeg_bytes(pixels(64, 80, rng), quality=90, subsampling=2, exif=exif, comment=b"c" * 2100)))
    return out


def declined_cases(seed=1):
    """[(name, bytes, pil_decodes)]: files the host pass must decline; pil_decodes tells whether PIL itself can decode them."""
    rng = np.random.default_rng(seed)
    px = pixels(64, 80, rng)
    out = [("progressive", jpeg_bytes(px, quality=90, progressive=True), True)]
    out.append(("cmyk", jpeg_bytes(Image.fromarray(px).convert("CMYK"), quality=90), True))
    try:
        raw = jpeg_bytes(px, quality=90, keep_rgb=True)
        if b"Adobe" in raw or raw[raw.index(b"\xff\xc0") + 10:][:1] != b"\x01":      # (an older Pillow ignores keep_rgb)
            out.append(("keep_rgb", raw, True))
    except (TypeError, OSError, ValueError):
        pass
    b = io.BytesIO()
    Image.fromarray(px).save(b, "PNG")
    out.append(("png", b.getvalue(), True))
    base = jpeg_bytes(px, quality=90, subsampling=2)
    out.append(("truncated_60", base[:len(base) * 6 // 10], False))
    at = base.index(b"\xff\xc4") + 5          # the first count byte (codes of length 1) of the first Huffman table
    flipped = bytearray(base)
    flipped[at] ^= 0xFF
    out.append(("huffman_flip", bytes(flipped), False))
    return out


def write_all(d, cases):
    paths = []
    for c in cases:
        ext = ".png" if c[0] == "png" else ".jpg"
        p = os.path.join(d, c[0] + ext)
        with open(p, "wb") as f:
            f.write(c[1])
        paths.append(p)
    return paths
