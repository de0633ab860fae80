"""Reference of the image preprocessing kernels (lemon_amd/csrc/preprocess.hip) in numpy: PIL's two integer resampling passes
in int64 and the float epilogue of generic_transform in IEEE float32, restated from the operation (no PIL, no torch in the
arithmetic).  Pinned against PIL + torch by tests/test_preprocess_host.py; tests/test_gpu_preprocess_edges.py compares the
kernels with it bit for bit.

A pass takes the tap table of its axis, kk [S, ks] int32 and bnd [S, 2] (first input index, tap count), for the S output
indices that are kept; the two axes' tables are independent (axis_table), which is what lets a test pair a 509-tap vertical
pass with a 4-pixel identity row."""
import numpy as np

from lemon_amd import datasets as ds
from lemon_amd.data import PIL_PRECISION_BITS, pil_bicubic_rows, resize_geometry

ROUND = 1 << (PIL_PRECISION_BITS - 1)
MEAN = np.asarray(ds.CLIP_MEAN, np.float32)
STD = np.asarray(ds.CLIP_STD, np.float32)


def axis_table(n_in, n_out, lo, S):
    """(kk, bnd) of output indices [lo, lo + S) of an n_in -> n_out resize"""
    return pil_bicubic_rows(n_in, n_out, lo, lo + S)


def _resample(src, kk, bnd):
    """src [n_in, ...] uint8 resampled along axis 0 -> (uint8 [S, ...], the int64 values before the clip)"""
    S = len(bnd)
    pre = np.empty((S,) + src.shape[1:], np.int64)
    for o in range(S):
        first, n = int(bnd[o, 0]), int(bnd[o, 1])
        acc = np.tensordot(kk[o, :n].astype(np.int64), src[first:first + n].astype(np.int64), axes=(0, 0))
        pre[o] = (ROUND + acc) >> PIL_PRECISION_BITS
    return np.clip(pre, 0, 255).astype(np.uint8), pre


def hpass(img, kk, bnd):
    """img [H, W, 3] uint8 -> ([H, S, 3] uint8, pre-clip int64 [H, S, 3])"""
    out, pre = _resample(np.ascontiguousarray(img.transpose(1, 0, 2)), kk, bnd)
    return np.ascontiguousarray(out.transpose(1, 0, 2)), np.ascontiguousarray(pre.transpose(1, 0, 2))


def vpass(tmp, kk, bnd):
    """tmp [H, S, 3] uint8 (input row r at tmp[r]) -> ([S, S, 3] uint8, pre-clip int64)"""
    return _resample(tmp, kk, bnd)


def epilogue(u8, mean=MEAN, std=STD):
    """ToTensor + Normalize of generic_transform in float32: [S, S, 3] uint8 -> [S, S, 3] float32"""
    x = u8.astype(np.float32) / np.float32(255.0)
    return ((x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).astype(np.float32)


def resample(img, th, tv):
    """both passes + epilogue of one image -> dict(h, h_pre, v, v_pre, f): the horizontal pass runs on every input row"""
    h, h_pre = hpass(img, *th)
    v, v_pre = vpass(h, *tv)
    return dict(h=h, h_pre=h_pre, v=v, v_pre=v_pre, f=epilogue(v))


def transform_tables(h, w, size):
    """the tables of generic_transform for an h x w image: ((kk_h, bnd_h), (kk_v, bnd_v))"""
    nh, nw, top, left = resize_geometry(h, w, size)
    return axis_table(w, nw, left, size), axis_table(h, nh, top, size)


def generic_transform(img, size):
    """generic_transform of an [H, W, 3] uint8 array -> float32 [3, size, size]"""
    th, tv = transform_tables(img.shape[0], img.shape[1], size)
    return nchw(resample(img, th, tv)["f"])


# ---- layouts of a float32 [S, S, 3] result ------------------------------------------------------------------------------
def nchw(f):
    return np.ascontiguousarray(f.transpose(2, 0, 1))


def patch_major(f, P):
    """[(S/P)^2, 3 P^2]: row py * nP + px, column c P^2 + (y % P) P + (x % P)"""
    S = f.shape[0]
    nP = S // P
    return np.ascontiguousarray(f.reshape(nP, P, nP, P, 3).transpose(0, 2, 4, 1, 3).reshape(nP * nP, 3 * P * P))


def operand(rows, fill):
    """float32 [m, K] patch rows -> the int32 words of the tile-major fp16 split operand (m padded to 128 rows): the hi and
    lo 2^11 halves of the owed rows where split3.hpp puts them, every other half-word at `fill`.  Needs a GPU (the index and
    the split are those of tests/test_gpu_gemm_forms.py)."""
    import torch
    from tests.test_gpu_gemm_forms import TM, _split, _tiled_index
    m, K = rows.shape
    words = (m + TM - 1) // TM * TM * K
    buf = torch.full((words,), fill, dtype=torch.int32, device="cuda")
    h = buf.view(torch.float16)
    idx = _tiled_index(m, K).reshape(-1)
    hi, lo = _split(torch.from_numpy(np.ascontiguousarray(rows)).cuda())
    h[idx] = hi.reshape(-1)
    h[idx + TM * 16] = lo.reshape(-1)
    return buf.cpu().numpy()


def block_spans(bnd_v, R):
    """input rows spanned by the vertical windows of every block of R output rows"""
    S = len(bnd_v)
    return [int(bnd_v[y0:min(y0 + R, S)].sum(1).max() - bnd_v[y0:min(y0 + R, S), 0].min()) for y0 in range(0, S, R)]
