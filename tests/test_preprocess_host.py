"""Host side of the image preprocessing kernels (no GPU): the reference the GPU tests compare with, and what the planners
promise the kernels.

1. tests/preprocess_ref.py (int64 passes, float32 epilogue, numpy only) reproduces generic_transform -- PIL's bicubic resize,
   centre crop, ToTensor, Normalize -- bit for bit, so that tests/test_gpu_preprocess_edges.py needs no PIL:

       h x w -> size     what the case is for
       1x1, 1x3, 3x1     windows clipped at both ends (one to three taps of five), one and both axes
       2x2, 5x7          small up-scaling, unequal sides (a crop on the longer one)
       8x8 -> 8          no resize: the identity table on both axes
       9x8 -> 8          no resize, a one-row crop
       40x56 -> 12       down-scaling, more taps than five, crop with a left margin
       64x48 -> 8        down-scaling by 6 and 8, crop with a top margin
       508x8 -> 8        a 500-row crop of an image that is not resized
       37x91 -> 30       odd sizes, an output that is no multiple of 4

2. data.transform_geometry (the geometry half of the same-shape planner) and data.ragged_plan over a sweep of shapes:
   k_preprocess_u8 reads a block's first input row from its first output row and its last from its last output row, and
   sizes its LDS tile by max_rows; k_ragged_h resamples rows [vmin, vmin + rows).  The sweep asserts what makes that right:
   window starts and ends non-decreasing in y, every window non-empty and inside the image, max_rows >= the span of every
   block at the chosen rows_per_block, and the two LDS bounds the ABI enforces."""
import numpy as np
import pytest

from lemon_amd import data
from tests import preprocess_ref as PR

PIL_CASES = [(1, 1, 8), (1, 3, 8), (3, 1, 8), (2, 2, 8), (5, 7, 8), (8, 8, 8), (9, 8, 8), (40, 56, 12), (64, 48, 8), (508, 8, 8),
             (37, 91, 30)]


@pytest.mark.parametrize("h,w,size", PIL_CASES)
def test_reference_is_generic_transform_bit_for_bit(h, w, size):
    from PIL import Image
    rng = np.random.default_rng(h * 1000 + w)
    smooth = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.array([0, 60, 130])
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
              rng.choice(np.array([0, 255], np.uint8), (h, w, 3)),                       # overshoot on both sides of the clip
              ((smooth + rng.integers(0, 8, (h, w, 3))) % 256).astype(np.uint8)]
    for k, img in enumerate(images):
        want = data.generic_transform(Image.fromarray(img), size).numpy()
        got = PR.generic_transform(img, size)
        assert got.shape == want.shape == (3, size, size) and got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (k, float(np.abs(got - want).max()))


def test_reference_layouts_and_clip_values():
    f = np.arange(12 * 12 * 3, dtype=np.float32).reshape(12, 12, 3)
    assert PR.nchw(f)[2, 5, 7] == f[5, 7, 2]
    pm = PR.patch_major(f, 4)
    assert pm.shape == (9, 48) and pm[1 * 3 + 2, 2 * 16 + 3 * 4 + 1] == f[4 + 3, 8 + 1, 2]
    # the integers before the clip are returned, and the clip is what the uint8 result applied to them
    img = np.random.default_rng(0).choice(np.array([0, 255], np.uint8), (5, 7, 3))
    th, tv = PR.axis_table(7, 12, 0, 12), PR.axis_table(5, 12, 0, 12)
    r = PR.resample(img, th, tv)
    for u8, pre in ((r["h"], r["h_pre"]), (r["v"], r["v_pre"])):
        assert pre.min() < 0 and pre.max() > 255
        assert np.array_equal(u8, np.clip(pre, 0, 255))
    # the identity table reproduces the pixels
    ident = PR.axis_table(7, 7, 0, 7)
    assert np.array_equal(PR.hpass(img, *ident)[0], img)


def test_transform_geometry_is_the_cropped_full_tables():
    """the pure function computes only the kept rows of each table: the same numbers as the crop of the whole table"""
    for h, w, size in [(32, 32, 224), (37, 91, 30), (480, 640, 224), (1, 3, 8), (224, 224, 224), (1500, 1200, 224)]:
        g = data.transform_geometry(h, w, size)
        nh, nw, top, left = data.resize_geometry(h, w, size)
        kk_h, b_h = data.pil_bicubic_tables(w, nw)
        kk_v, b_v = data.pil_bicubic_tables(h, nh)
        for got, want in ((g["kk_h"], kk_h[left:left + size]), (g["b_h"], b_h[left:left + size]),
                          (g["kk_v"], kk_v[top:top + size]), (g["b_v"], b_v[top:top + size])):
            assert got.dtype == np.int32 and np.array_equal(got, want)
        assert (g["ks_h"], g["ks_v"]) == (kk_h.shape[1], kk_v.shape[1])
    assert data.transform_geometry(1500, 1200, 224)["rows_per_block"] == 8
    assert data.transform_geometry(3000, 2000, 224)["rows_per_block"] == 4
    with pytest.raises(ValueError):
        data.transform_geometry(8000, 6000, 224)


SIDES = list(range(1, 71)) + [91, 224, 225, 375, 480, 500, 640, 1000, 1200, 1500, 2000, 3000]
SIZES = (8, 12, 30, 224, 336)


def _check_windows(b, n_in, what):
    start, end = b[:, 0].astype(np.int64), b[:, 0].astype(np.int64) + b[:, 1]
    assert np.all(np.diff(start) >= 0) and np.all(np.diff(end) >= 0), (what, "windows not monotone")
    assert np.all(b[:, 1] >= 1) and np.all(start >= 0) and np.all(end <= n_in), (what, "window outside the image")


@pytest.mark.parametrize("size", SIZES)
def test_planners_keep_their_promise_to_the_kernels(size):
    """SIDES x SIDES.  Everything asserted is a property of one axis' table; a table depends on (h, w) only through (input
    side, resized side, crop origin), and the horizontal table of h x w is the vertical table of w x h.  A shape is skipped
    when its vertical table has been checked already: the sweep is symmetric, so every table of either axis is visited."""
    seen, plans, no_plan, visited = set(), 0, 0, 0
    for h in SIDES:
        for w in SIDES:
            nh, nw, top, left = data.resize_geometry(h, w, size)
            if (h, nh, top) in seen:
                continue
            seen.add((h, nh, top))
            visited += 1
            try:
                g = data.transform_geometry(h, w, size)
            except ValueError:
                no_plan += 1
                g = None
            if g is not None:
                plans += 1
                what = (h, w, size)
                _check_windows(g["b_v"], h, what + ("v",))
                _check_windows(g["b_h"], w, what + ("h",))
                assert g["kk_v"].shape == (size, g["ks_v"]) and g["kk_h"].shape == (size, g["ks_h"])
                assert np.all(g["b_v"][:, 1] <= g["ks_v"]) and np.all(g["b_h"][:, 1] <= g["ks_h"])
                R = g["rows_per_block"]
                assert R >= 1 and g["max_rows"] >= max(PR.block_spans(g["b_v"], R)), what
                assert R * (2 + g["ks_v"]) <= 512 and g["max_rows"] * size * 3 <= 56 * 1024, what
            try:
                hdr, taps = data.ragged_plan(h, w, size)
            except ValueError:
                continue
            ks_h, ks_v, R, vmin, rows = (int(hdr[i]) for i in (6, 7, 8, 10, 11))
            b_h = taps[hdr[3]:hdr[3] + 2 * size].reshape(size, 2)
            b_v = taps[hdr[5]:hdr[5] + 2 * size].reshape(size, 2)
            _check_windows(b_v, h, (h, w, size, "ragged v"))
            _check_windows(b_h, w, (h, w, size, "ragged h"))
            assert (hdr[0], hdr[1]) == (h, w) and len(taps) == size * (ks_h + ks_v + 4)
            assert vmin == b_v[0, 0] and vmin + rows == b_v[-1].sum() and vmin + rows <= h
            assert np.all(b_v[:, 0] >= vmin) and np.all(b_v.sum(1) <= vmin + rows)
            assert 1 <= R <= 16 and R * (2 + ks_v) <= 4096 and hdr[9] == -(-size // R) and hdr[12] == -(-rows // 16)
            if g is not None:
                assert np.array_equal(b_v, g["b_v"]) and np.array_equal(taps[hdr[4]:hdr[4] + size * ks_v].reshape(size, ks_v), g["kk_v"])
    print(f"[preprocess] size {size}: {plans} same-shape plans, {no_plan} shapes without one, {visited} of {len(SIDES) ** 2} shapes visited")
    assert plans >= 300
