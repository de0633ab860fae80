"""Dataset readers and preprocessing for the run_lemon surface, without torchvision.

Mirrors (behaviour, not code) of:
  generic_transform                      lib/datasets/utils.py:163-170  (Resize(224, bicubic) -> CenterCrop(224)
                                         -> ToTensor -> Normalize(CLIP_MEAN, CLIP_STD))
  get_dataset('cifar10'|'cifar100'|...)  lib/datasets/utils.py:350-430  (torchvision CIFAR pickles, 80/10/10 split)
  NoisyCombinedDataset                   lib/datasets/dataloader.py:16-30   -> (x, clean, noisy)
  get_captioning_dataset / CaptioningDataset   lib/datasets/utils.py:275-323, dataloader.py:167-198
  get_large_scale_dataset / LargeScaleDataset  lib/datasets/utils.py:325-347, dataloader.py:113-133
Datasets are read from LOCAL paths only (no download: there is no network).  A synthetic class dataset
(`dataset_root='synthetic:N'`: seeded random uint8 images with the dataset's label set) stands in when no data is present.
"""
import functools
import math
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import datasets as ds


# ------------------------------------------------------------------------------ preprocessing
def generic_transform(img, size=224):
    """PIL RGB image -> float32 [3,size,size], CLIP-normalised.  Same steps as torchvision's
    Resize(shorter side, BICUBIC on the PIL image) / CenterCrop / ToTensor / Normalize."""
    from PIL import Image
    w, h = img.size
    if (w <= h and w != size) or (h <= w and h != size):
        if w <= h:
            nw, nh = size, int(size * h / w)
        else:
            nw, nh = int(size * w / h), size
        img = img.resize((nw, nh), Image.BICUBIC)
        w, h = nw, nh
    left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
    img = img.crop((left, top, left + size, top + size))
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0)
    mean = torch.tensor(ds.CLIP_MEAN).view(3, 1, 1)
    std = torch.tensor(ds.CLIP_STD).view(3, 1, 1)
    return (x - mean) / std


_GENERIC_TRANSFORM = generic_transform


# ------------------------------------------------------------------------------ preprocessing on the GPU
PIL_PRECISION_BITS = 22      # Pillow Resample.c: 32 - 8 - 2


def _bicubic(x):
    a = -0.5                 # Pillow's bicubic_filter
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def pil_bicubic_tables(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BICUBIC (Resample.c), restated: for every
    output index the first input index, the tap count and the 22-bit fixed-point taps.  in == out -> the
    identity table (Pillow skips the pass; tap 1<<22 reproduces the pixel exactly)."""
    return pil_bicubic_rows(in_size, out_size, 0, out_size)


def pil_bicubic_rows(in_size, out_size, lo, hi):
    """Rows [lo, hi) of pil_bicubic_tables(in_size, out_size), computed for those output indices only (a 2 x 300 image resizes
    to a width of 33 600 before generic_transform's crop keeps 224 of them)."""
    if in_size == out_size:
        kk = np.full((hi - lo, 1), 1 << PIL_PRECISION_BITS, np.int32)
        bounds = np.stack([np.arange(lo, hi), np.ones(hi - lo, np.int64)], 1).astype(np.int32)
        return kk, bounds
    # the scalar recipe of pil_bicubic_tables, vectorised over output indices: every value is computed by the same float64
    # operations in the same order (the weight sum runs over taps in order; the zero weights past a window add exactly 0.0)
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(lo, hi, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    t = np.arange(ksize)
    x = np.abs(((t[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    a_ = -0.5                                                   # Pillow's bicubic_filter
    w = np.where(x < 1.0, ((a_ + 2.0) * x - (a_ + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a_, 0.0))
    w = np.where(t[None, :] < xmax[:, None], w, 0.0)
    ww = np.zeros(hi - lo)
    for j in range(ksize):
        ww = ww + w[:, j]
    v = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    f = v * (1 << PIL_PRECISION_BITS)
    kk = np.trunc(np.where(v < 0, -0.5 + f, 0.5 + f)).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    return kk, bounds


def resize_geometry(h, w, size):
    """generic_transform's resized size (nh, nw) and crop origin (top, left) for an h x w image."""
    if (w <= h and w != size) or (h <= w and h != size):
        nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
    else:
        nw, nh = w, h
    return nh, nw, int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))


def transform_geometry(h, w, size):
    """Resize geometry of generic_transform for an h x w image on the host (numpy only): the cropped tap tables and the block
    geometry of lemon_preprocess_u8 -- rows_per_block output rows per workgroup, max_rows the input rows the widest block's
    vertical windows span.  The kernel takes a block's first input row from its first output row and the last from its last
    (windows are monotone in y) and sizes its LDS tile by max_rows."""
    nh, nw, top, left = resize_geometry(h, w, size)
    if nw < size or nh < size:
        raise ValueError(f"image {h}x{w} resizes to {nh}x{nw}, smaller than the {size}x{size} crop")
    kk_h, b_h = pil_bicubic_rows(w, nw, left, left + size)
    kk_v, b_v = pil_bicubic_rows(h, nh, top, top + size)
    rows_per_block = 16
    while True:     # input rows one block's vertical windows span; shrink the block until the tile fits LDS
        spans = [int(b_v[min(y0 + rows_per_block, size) - 1].sum() - b_v[y0, 0]) for y0 in range(0, size, rows_per_block)]
        # (the kernel's LDS: the uint8 tile <= 56 KB, and the block's vertical windows, rows x (2 + taps) <= 512 ints)
        fits = max(spans) * size * 3 <= 56 * 1024 and rows_per_block * (2 + kk_v.shape[1]) <= 512
        if fits or rows_per_block == 1:
            break
        rows_per_block //= 2
    if not fits:
        raise ValueError(f"image {h}x{w}: vertical window of {max(spans)} rows / {kk_v.shape[1]} taps does not fit the LDS tile")
    return dict(kk_h=kk_h, b_h=b_h, kk_v=kk_v, b_v=b_v, ks_h=kk_h.shape[1], ks_v=kk_v.shape[1],
                max_rows=max(spans), rows_per_block=rows_per_block)


@functools.lru_cache(maxsize=16)
def _gpu_transform_plan(h, w, size, device_index):
    """transform_geometry(h, w, size) with the tap tables on the device."""
    plan = transform_geometry(h, w, size)
    dev = torch.device("cuda", device_index)
    for key in ("kk_h", "b_h", "kk_v", "b_v"):
        plan[key] = torch.from_numpy(np.ascontiguousarray(plan[key])).to(dev)
    return plan


class PatchOperand:
    """The patch rows of a preprocessed image batch as the tile-major fp16 split operand of lemon_linear_f16x3t
    (lemon_preprocess_u8_f16x3t): `at` flat fp16, rows = batch * n_patches (padded to 128), k = 3 * patch^2."""

    def __init__(self, at, batch, n_patches, k):
        self.at, self.batch, self.n_patches, self.k = at, batch, n_patches, k
        self.is_cuda, self.device = True, at.device


def patch_operand_supported(patch, size=224):
    return patch > 0 and patch % 4 == 0 and size % 4 == 0 and (3 * patch * patch) % 32 == 0


def gpu_transform_batch(images_u8, size=224, patch=0, operand=False):
    """generic_transform for a uint8 CUDA batch [B,H,W,3] in one HIP kernel (lemon_preprocess_u8):
    -> float32 [B,3,size,size], bit-identical to the PIL + torch pipeline; with patch=P the same values
    in patch-major order [B, (size/P)^2, 3*P*P] (the ViT patch embedding then is one GEMM); with operand=True (and
    patch_operand_supported(P)) a PatchOperand: the same rows already split for the hand-written GEMM."""
    import ctypes
    from . import _lib
    from .ops import ptr, stream_ptr
    assert images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[3] == 3
    x = images_u8.contiguous()
    B, H, W, _ = x.shape
    plan = _gpu_transform_plan(H, W, size, x.device.index or 0)
    mean = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in ds.CLIP_MEAN])
    std = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in ds.CLIP_STD])
    lib = _lib.load()
    if operand:
        assert patch_operand_supported(patch, size)
        nP, K = (size // patch) ** 2, 3 * patch * patch
        rows = (B * nP + 127) // 128 * 128
        at = torch.empty((rows * K * 2,), dtype=torch.float16, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.lemon_preprocess_u8_f16x3t(ptr(x), B, H, W, ptr(plan["kk_h"]), ptr(plan["b_h"]), plan["ks_h"],
                                                      ptr(plan["kk_v"]), ptr(plan["b_v"]), plan["ks_v"], size, plan["max_rows"],
                                                      plan["rows_per_block"], mean, std, int(patch), ptr(at), stream_ptr(x.device)),
                       "lemon_preprocess_u8_f16x3t")
        return PatchOperand(at, B, nP, K)
    out = torch.empty((B, 3, size, size) if not patch else (B, (size // patch) ** 2, 3 * patch * patch),
                      dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.lemon_preprocess_u8(ptr(x), B, H, W, ptr(plan["kk_h"]), ptr(plan["b_h"]), plan["ks_h"],
                                           ptr(plan["kk_v"]), ptr(plan["b_v"]), plan["ks_v"], size, plan["max_rows"],
                                           plan["rows_per_block"], mean, std, int(patch), ptr(out), stream_ptr(x.device)),
                   "lemon_preprocess_u8")
    return out


# ------------------------------------------------------------------------------ ragged batches (file datasets)
RAGGED_HROWS = 16             # input rows per horizontal-pass workgroup (preprocess.hip)
RAGGED_PLAN_INTS = 16         # int32 per plan (preprocess.hip: PL_*)
_VTAB_MAX_INTS = 4096        # ints of a vertical-pass workgroup's window table (preprocess.hip: RAGGED_VTAB_INTS)


@functools.lru_cache(maxsize=4096)
def ragged_plan(h, w, size):
    """The resize plan of one input shape for lemon_preprocess_ragged: the cropped PIL tap tables (only the `size` kept rows /
    columns are computed) and the block geometry -> (int32 header [RAGGED_PLAN_INTS] with offsets relative to the plan's own
    taps, int32 taps [kk_h | bnd_h | kk_v | bnd_v])."""
    nh, nw, top, left = resize_geometry(h, w, size)
    if nw < size or nh < size:
        raise ValueError(f"image {h}x{w} resizes to {nh}x{nw}, smaller than the {size}x{size} crop")
    kk_h, b_h = pil_bicubic_rows(w, nw, left, left + size)
    kk_v, b_v = pil_bicubic_rows(h, nh, top, top + size)
    ks_h, ks_v = kk_h.shape[1], kk_v.shape[1]
    R = min(16, _VTAB_MAX_INTS // (2 + ks_v))
    if R < 1:
        raise ValueError(f"image {h}x{w}: {ks_v} vertical taps per output row exceed the kernel's window table")
    vmin = int(b_v[:, 0].min())
    rows = int((b_v[:, 0] + b_v[:, 1]).max()) - vmin
    parts = [kk_h.ravel(), b_h.ravel(), kk_v.ravel(), b_v.ravel()]
    offs = np.cumsum([0] + [len(a) for a in parts])
    hdr = np.zeros(RAGGED_PLAN_INTS, np.int32)
    hdr[:13] = (h, w, offs[0], offs[1], offs[2], offs[3], ks_h, ks_v, R, (size + R - 1) // R, vmin, rows,
                (rows + RAGGED_HROWS - 1) // RAGGED_HROWS)
    return hdr, np.concatenate(parts).astype(np.int32)


class RaggedPlans:
    """The distinct input shapes of a ragged batch and, per output size, their plans on the device (built once, shared by
    every sub-batch)."""

    def __init__(self, shapes):
        self.shapes = list(shapes)          # plan index -> (H, W)
        self._dev = {}

    def tables(self, size, device):
        key = (size, str(device))
        if key not in self._dev:
            hdrs, taps, base = [], [], 0
            for h, w in self.shapes:
                hdr, t = ragged_plan(h, w, size)
                hdr = hdr.copy()
                hdr[2:6] += base
                hdrs.append(hdr); taps.append(t); base += len(t)
            hdr = np.stack(hdrs) if hdrs else np.zeros((0, RAGGED_PLAN_INTS), np.int32)
            taps = np.concatenate(taps) if taps else np.zeros(1, np.int32)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)
            self._dev[key] = (hdr, up(hdr), up(taps))
        return self._dev[key]


class RaggedImages:
    """A batch of uint8 HWC images of different sizes on the device: `data` one packed uint8 buffer, `desc` (host int64
    [n, 4]: byte offset, H, W, plan index) and the batch's RaggedPlans.  len(), contiguous slices and index tensors select
    sub-batches: a subset of descriptors over the same buffer, nothing is repacked."""
    dtype = torch.uint8

    def __init__(self, data, desc, plans):
        self.data, self.desc, self.plans = data, np.asarray(desc, np.int64).reshape(-1, 4), plans
        self.device, self.is_cuda = data.device, data.is_cuda

    @classmethod
    def from_arrays(cls, arrays, device):
        """Pack a list of uint8 HWC numpy arrays (any sizes) into one device batch."""
        shapes, desc, off = {}, [], 0
        for a in arrays:
            h, w = a.shape[:2]
            desc.append((off, h, w, shapes.setdefault((h, w), len(shapes))))
            off += a.nbytes
        buf = torch.empty(max(off, 1), dtype=torch.uint8).pin_memory()
        flat = buf.numpy()
        for (o, h, w, _), a in zip(desc, arrays):
            flat[o:o + a.nbytes] = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
        return cls(buf.to(device, non_blocking=True), np.array(desc, np.int64), RaggedPlans(shapes))

    def __len__(self):
        return len(self.desc)

    @property
    def shape(self):
        return (len(self),)

    def __getitem__(self, sel):
        if isinstance(sel, torch.Tensor):
            sel = sel.cpu().numpy()
        return RaggedImages(self.data, self.desc[sel], self.plans)

    def to(self, device, non_blocking=False):
        assert torch.device(device) == self.device or (torch.device(device).type == "cuda" and torch.device(device).index is None)
        return self

    def image(self, i):
        """Image i as a uint8 [H, W, 3] device tensor (a view of the packed buffer)."""
        o, h, w, _ = (int(v) for v in self.desc[i])
        return self.data[o:o + h * w * 3].view(h, w, 3)


def launch_jpeg_decode(data, layout, poison=None):
    """Enqueue lemon_jpeg_decode on the current stream for a device buffer `data` laid out by a jpeg_host.BatchLayout
    ([payload with records and aux table | decoded RGB]): the records' pixels appear at their RaggedImages offsets.  `poison`
    (a byte, for tests) pre-fills the decoded region and the work buffer."""
    from . import _lib
    import ctypes
    from .ops import stream_ptr
    if not layout.n_jpeg:
        return
    assert data.is_cuda and data.dtype == torch.uint8 and data.numel() >= layout.total_bytes
    dev = data.device
    with torch.cuda.device(dev):
        work = torch.empty((layout.work_bytes,), dtype=torch.uint8, device=dev)
        if poison is not None:
            work.fill_(poison)
            data[layout.decoded_off:].fill_(poison)
        base, vp = data.data_ptr(), ctypes.c_void_p
        _lib.check(_lib.load().lemon_jpeg_decode(vp(base), layout.rec_end, layout.n_jpeg, vp(base + layout.aux_off),
                                                 layout.idct_blocks, layout.rgb_blocks, vp(work.data_ptr()), work.numel(), vp(base),
                                                 data.numel(), stream_ptr(dev)), "lemon_jpeg_decode")


def launch_jpeg_entropy(data, layout, poison=None, return_workspace=False):
    """Enqueue lemon_jpeg_entropy_device on the current stream for the scan packets of a device buffer `data` laid out by a
    jpeg_host.BatchLayout: their coefficient records appear in the buffer's device-only region, where launch_jpeg_decode (to be
    called after this) reads them; progressive packets (layout.prog_packets) go through lemon_jpeg_prog_entropy_device behind the
    baseline ones.  Returns the int32 device tensor of the packets' statuses, in the order of layout.packets then
    layout.prog_packets (layout.status_record; None without packets).  `poison` (a byte, for tests) pre-fills the records' region and the workspace.  return_workspace=True (for
    tools/jpeg_entropy_time.py) returns (statuses, the workspace tensor), whose first int32 [n_packets, 4] hold diagnostics
    (csrc/jpeg_entropy.hip::JentWs)."""
    from . import _lib
    import ctypes
    from .ops import stream_ptr
    n_base, n_prog = getattr(layout, "n_packets", 0), getattr(layout, "n_prog", 0)
    if not n_base and not n_prog:
        return (None, None) if return_workspace else None
    assert data.is_cuda and data.dtype == torch.uint8 and data.numel() >= layout.total_bytes
    dev = data.device
    with torch.cuda.device(dev):
        lib = _lib.load()
        need = lib.lemon_jpeg_entropy_workspace_bytes(n_base, layout.groups, layout.intervals)
        if need < 0:
            raise _lib.LemonHipError(f"lemon_jpeg_entropy_workspace_bytes: {layout.groups} workgroups, {layout.intervals} intervals")
        pneed = lib.lemon_jpeg_prog_entropy_workspace_bytes(n_prog, layout.prog_items, layout.prog_levels) if n_prog else 0
        if pneed < 0:
            raise _lib.LemonHipError(f"lemon_jpeg_prog_entropy_workspace_bytes: {layout.prog_items} items, {layout.prog_levels} levels")
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        pws = torch.empty((max(pneed, 16),), dtype=torch.uint8, device=dev)
        status = torch.empty((n_base + n_prog,), dtype=torch.int32, device=dev)
        if poison is not None:
            ws.fill_(poison)
            pws.fill_(poison)
            status.fill_(poison)
            data[layout.payload_bytes:layout.decoded_off].fill_(poison)
        base, vp = data.data_ptr(), ctypes.c_void_p
        if n_base:
            _lib.check(lib.lemon_jpeg_entropy_device(vp(base), layout.payload_bytes, n_base, vp(base + layout.edesc_off),
                                                     layout.groups, layout.intervals, layout.subseq, vp(base), layout.rec_end,
                                                     vp(status.data_ptr()), vp(ws.data_ptr()), ws.numel(), stream_ptr(dev)),
                       "lemon_jpeg_entropy_device")
        if n_prog:                                   # the progressive packets, behind the baseline ones on the same stream
            _lib.check(lib.lemon_jpeg_prog_entropy_device(vp(base), layout.payload_bytes, n_prog, vp(base + layout.pdesc_off),
                                                          layout.prog_items, layout.prog_levels, vp(base), layout.rec_end,
                                                          vp(status.data_ptr() + 4 * n_base), vp(pws.data_ptr()), pws.numel(),
                                                          stream_ptr(dev)), "lemon_jpeg_prog_entropy_device")
    return (status, ws) if return_workspace else status


def decode_jpegs(files, device, fallback=False, poison=None, entropy="host", progressive=False):
    """Decode JPEG files on the GPU -> RaggedImages of `Image.open(f).convert("RGB")`'s pixels, bit for bit.  `files`: paths or
    bytes objects.  entropy="host": the Huffman pass runs here on the host (csrc/jpeg_entropy.hpp), everything after it in
    lemon_jpeg_decode.  entropy="device": the host only strips the files down to scan packets (lemon_jpeg_pack), the Huffman pass
    runs in lemon_jpeg_entropy_device and the statuses are read back once before
    returning.  A file that is declined (progressive, CMYK, not a JPEG, corrupt, ...) raises ValueError, or with fallback=True is
    decoded by PIL (whose own exception a corrupt file then raises).  progressive=True: a progressive file is not declined but
    takes the progressive Huffman pass, on the host (csrc/jpeg_prog.hpp) or on the device (csrc/jpeg_prog.hip) as `entropy`
    says.  The result carries `layout` (jpeg_host.BatchLayout)."""
    import io
    from PIL import Image
    from . import jpeg_host
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy={entropy!r}: expected 'host' or 'device'")
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("decode_jpegs needs a CUDA/HIP device: there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    lay, items, off, sources = jpeg_host.BatchLayout(), [], 0, {}
    declined = lambda what, status: ValueError(f"{what}: not decodable on the GPU ({jpeg_host.STATUS.get(status, status)})")
    for f in files:
        raw = f if isinstance(f, (bytes, bytearray, memoryview)) else open(f, "rb").read()
        what = "<bytes>" if raw is f else f
        if entropy == "device":
            rec, info = jpeg_host.pack(bytes(raw), progressive=progressive)
        else:
            rec, info = jpeg_host.decode_record(bytes(raw), progressive=progressive)
        if rec is None:
            if not fallback:
                raise declined(what, info.status)
            px = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
            lay.add_pixels(off, px.shape[0], px.shape[1])
            items.append((off, px.reshape(-1)))
            off = (off + px.nbytes + 15) & ~15
        else:
            if entropy == "device":
                lay.add_packet(off, rec)
                sources[len(lay.records) - 1] = (what, raw)
            else:
                lay.add_record(off, rec)
            items.append((off, rec.data))
            off = (off + rec.data.nbytes + 15) & ~15
    aux = lay.finish(off)
    buf = torch.empty((max(lay.payload_bytes, 1),), dtype=torch.uint8).pin_memory()
    flat = buf.numpy()
    for o, a in items:
        flat[o:o + a.nbytes] = a
    if aux.size:
        flat[lay.aux_off:lay.payload_bytes] = aux.view(np.uint8)
    data = torch.empty((max(lay.total_bytes, buf.numel()),), dtype=torch.uint8, device=device)
    data[:buf.numel()].copy_(buf, non_blocking=True)
    status = launch_jpeg_entropy(data, lay, poison)
    launch_jpeg_decode(data, lay, poison)
    if status is not None:
        st = status.cpu().numpy()                                 # (the one read-back)
        for k in np.flatnonzero(st):                              # (rare: the scan itself is corrupt)
            what, raw = sources[lay.status_record(k)]
            if not fallback:
                raise declined(what, int(st[k]))
            px = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
            o, h, w, _ = lay.desc[lay.records[lay.status_record(k)][0]]
            if px.shape != (h, w, 3):
                raise declined(what, int(st[k]))
            data[o:o + px.size].copy_(torch.from_numpy(px.reshape(-1).copy()))
    out = RaggedImages(data, np.array(lay.desc, np.int64).reshape(-1, 4), RaggedPlans(lay.shapes))
    out.layout = lay
    return out


def launch_png_decode(data, layout, poison=None):
    """Enqueue lemon_png_decode on the current stream for the PNG records of a device buffer `data` laid out by a
    jpeg_host.BatchLayout: their pixels appear at their RaggedImages offsets (lib/datasets/dataloader.py:184's
    `Image.open(p).convert("RGB")`).  Returns the int32 device tensor of the images' statuses in the order of
    layout.png_records (0, LEMON_PNG_FILTER, LEMON_PNG_INDEX: the caller decodes those with PIL; None without PNG records).
    `poison` (a byte, for tests) pre-fills the PNGs' pixel region, the work buffer and the statuses."""
    from . import _lib
    import ctypes
    from .ops import stream_ptr
    if not getattr(layout, "n_png", 0):
        return None
    assert data.is_cuda and data.dtype == torch.uint8 and data.numel() >= layout.total_bytes
    dev = data.device
    with torch.cuda.device(dev):
        work = torch.empty((layout.png_work_bytes,), dtype=torch.uint8, device=dev)
        status = torch.empty((layout.n_png,), dtype=torch.int32, device=dev)
        if poison is not None:
            work.fill_(poison)
            status.fill_(poison)
            data[layout.png_decoded_off:].fill_(poison)
        base, vp = data.data_ptr(), ctypes.c_void_p
        _lib.check(_lib.load().lemon_png_decode(vp(base), layout.png_rec_end, layout.n_png, vp(base + layout.png_aux_off),
                                                vp(work.data_ptr()), work.numel(), vp(base), data.numel(), vp(status.data_ptr()),
                                                stream_ptr(dev)), "lemon_png_decode")
    return status


def launch_png_inflate(data, layout, poison=None):
    """Enqueue lemon_png_inflate on the current stream for the PNG streams of a device buffer `data` laid out by a
    jpeg_host.BatchLayout (add_png_stream): the filtered scanlines of lib/datasets/dataloader.py:177-184's file appear in their
    device-only records, each behind its palette (copied from the payload for palette images), where launch_png_decode -- to be
    called next on the same stream -- reads them.  Returns the int32 device tensor of the streams' statuses in the order of
    layout.png_records (0, LEMON_PNG_STREAM; None without streams).  `poison` (a byte, for tests) pre-fills the records and the
    statuses."""
    from . import _lib
    import ctypes
    from .ops import stream_ptr
    if not getattr(layout, "png_streams", None):
        return None
    assert data.is_cuda and data.dtype == torch.uint8 and data.numel() >= layout.total_bytes
    dev = data.device
    with torch.cuda.device(dev):
        status = torch.empty((len(layout.png_streams),), dtype=torch.int32, device=dev)
        if poison is not None:
            status.fill_(poison)
            data[layout.png_rec_off:layout.png_rec_end].fill_(poison)
        base, vp = data.data_ptr(), ctypes.c_void_p
        _lib.check(_lib.load().lemon_png_inflate(vp(base), layout.payload_bytes, len(layout.png_streams), vp(base + layout.png_zaux_off),
                                                 vp(base), layout.png_rec_end, vp(status.data_ptr()), stream_ptr(dev)), "lemon_png_inflate")
        for k, zoff, _, _ in layout.png_streams:
            _, roff, _, _, ct, _ = layout.png_records[k]
            if ct == 3:                          # (lemon_png_decode reads the palette of a palette image only)
                data[roff:roff + 1024].copy_(data[zoff:zoff + 1024])
    return status


def first_png_status(inflate_status, decode_status):
    """The verdict of a PNG that took both kernels: the inflate's where it is not zero, else the decode's (device tensors)."""
    if inflate_status is None:
        return decode_status
    return torch.where(inflate_status != 0, inflate_status, decode_status)


def decode_pngs(files, device, fallback=False, poison=None, inflate="host"):
    """Decode PNG files on the GPU -> RaggedImages of `Image.open(f).convert("RGB")`'s pixels, bit for bit
    (lib/datasets/dataloader.py:177-184).  `files`: paths or bytes objects.  The chunk walk and the inflate run here on the host
    (png_host.py), unfiltering and the expansion to RGB in lemon_png_decode; the statuses are read back once before returning.
    inflate="device": only the chunk walk runs here (png_host.pack_stream), the files cross to the device compressed and
    lemon_png_inflate writes their records there; a stream it declines is a declined file like any other.
    A file that is declined (16-bit, interlaced, corrupt, not a PNG, a filter byte above 4, a palette index beyond PLTE, ...)
    raises ValueError naming the status, or with fallback=True is decoded by PIL (whose own exception a corrupt file then
    raises).  The result carries `layout` (jpeg_host.BatchLayout) and `status` (int32 numpy, per PNG record)."""
    import io
    from PIL import Image
    from . import jpeg_host, png_host
    if inflate not in ("host", "device"):
        raise ValueError(f"inflate={inflate!r}: expected 'host' or 'device'")
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("decode_pngs needs a CUDA/HIP device: there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    lay, items, off, sources = jpeg_host.BatchLayout(), [], 0, []
    declined = lambda what, status: ValueError(f"{what}: not decodable on the GPU ({png_host.STATUS.get(status, status)})")
    for f in files:
        raw = f if isinstance(f, (bytes, bytearray, memoryview)) else open(f, "rb").read()
        what = "<bytes>" if raw is f else f
        raw = bytes(raw)
        rec, info = png_host.pack_stream(raw) if inflate == "device" else png_host.decode_record(raw)
        if rec is None:
            if not fallback:
                raise declined(what, info.status)
            px = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
            lay.add_pixels(off, px.shape[0], px.shape[1])
            items.append((off, px.reshape(-1)))
            off = (off + px.nbytes + 15) & ~15
        else:
            (lay.add_png_stream if inflate == "device" else lay.add_png_record)(off, rec)
            sources.append((what, raw))
            items.append((off, rec.data))
            off = (off + rec.data.nbytes + 15) & ~15
    aux = lay.finish(off)
    buf = torch.empty((max(lay.payload_bytes, 1),), dtype=torch.uint8).pin_memory()
    flat = buf.numpy()
    for o, a in items:
        flat[o:o + a.nbytes] = a
    if aux.size:
        flat[lay.aux_off:lay.payload_bytes] = aux.view(np.uint8)
    data = torch.empty((max(lay.total_bytes, buf.numel()),), dtype=torch.uint8, device=device)
    data[:buf.numel()].copy_(buf, non_blocking=True)
    status = first_png_status(launch_png_inflate(data, lay, poison), launch_png_decode(data, lay, poison))
    st = status.cpu().numpy() if status is not None else np.zeros(0, np.int32)      # (the one read-back)
    for k in np.flatnonzero(st):
        what, raw = sources[k]
        if not fallback:
            raise declined(what, int(st[k]))
        px = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
        o, h, w, _ = lay.desc[lay.png_records[k][0]]
        if px.shape != (h, w, 3):
            raise declined(what, int(st[k]))
        data[o:o + px.size].copy_(torch.from_numpy(px.reshape(-1).copy()))
    out = RaggedImages(data, np.array(lay.desc, np.int64).reshape(-1, 4), RaggedPlans(lay.shapes))
    out.layout, out.status = lay, st
    return out


def mimic_image_path(path):
    """The file lib/datasets/dataloader.py:177-184 opens for a mimiccxr_caption frame path: the fifth path component from the
    end replaced by `downsampled_files` and the suffix by `.png` when that file exists, else `path` itself."""
    from pathlib import Path
    parts = list(Path(path).parts)
    if len(parts) >= 5:
        parts[-5] = "downsampled_files"
        reduced = Path(*parts).with_suffix(".png")
        if reduced.is_file():
            return str(reduced)
    return path


def gpu_transform_ragged(images, size=224, patch=0, operand=False):
    """generic_transform of a RaggedImages batch in one lemon_preprocess_ragged call (two launches): float32 [B,3,size,size],
    patch-major [B, (size/P)^2, 3 P^2] with patch=P, or with operand=True a PatchOperand -- row i = image i of the batch, the
    same bits as gpu_transform_batch on each image (and as the PIL + torch pipeline)."""
    import ctypes
    from . import _lib
    from .ops import ptr, stream_ptr
    assert isinstance(images, RaggedImages) and images.is_cuda
    dev = images.device
    B = len(images)
    hdr, plans_dev, taps_dev = images.plans.tables(size, dev)
    desc = images.desc
    ph = hdr[desc[:, 3]] if B else np.zeros((0, RAGGED_PLAN_INTS), np.int32)
    rows = ph[:, 11].astype(np.int64)
    hpre = np.concatenate([[0], np.cumsum(ph[:, 12], dtype=np.int64)])
    vpre = np.concatenate([[0], np.cumsum(ph[:, 9], dtype=np.int64)])
    ioff = np.concatenate([[0], np.cumsum(rows * 3 * size)])
    aux = torch.from_numpy(np.concatenate([desc.ravel(), hpre, vpre, ioff[:-1]]).astype(np.int64)).pin_memory()
    aux = aux.to(dev, non_blocking=True)
    work = torch.empty((max(int(ioff[-1]), 4),), dtype=torch.uint8, device=dev)
    mean = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in ds.CLIP_MEAN])
    std = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in ds.CLIP_STD])
    if operand:
        assert patch_operand_supported(patch, size)
        nP, K = (size // patch) ** 2, 3 * patch * patch
        out = torch.empty(((B * nP + 127) // 128 * 128 * K * 2,), dtype=torch.float16, device=dev)
    else:
        out = torch.empty((B, 3, size, size) if not patch else (B, (size // patch) ** 2, 3 * patch * patch),
                          dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lemon_preprocess_ragged(ptr(images.data), images.data.numel(), B, ptr(aux), int(hpre[-1]), int(vpre[-1]), ptr(plans_dev),
                                                       ptr(taps_dev), ptr(work), size, mean, std, int(patch), int(bool(operand)),
                                                       ptr(out), stream_ptr(dev)), "lemon_preprocess_ragged")
    return PatchOperand(out, B, nP, K) if operand else out


class ImageLabelSet:
    """(x, clean, noisy) triples like NoisyCombinedDataset / CaptioningDataset.  `images` is one of
      * uint8 [N,H,W,3] in memory (CIFAR pickles, `pixels.npy`): generic_transform runs on the GPU per batch;
      * float32 [N,...] in memory: pixel tensors that are ALREADY what the model consumes (a preprocessed cache);
        passed through unchanged;
      * a list of file paths: with a CUDA device, decoded by worker processes and transformed on the GPU as RaggedImages
        batches (lemon_amd/loader.py), with LEMON_PNG=gpu PNGs unfiltered and expanded on the GPU (default pil), with LEMON_JPEG=gpu baseline JPEGs with the device half of their decode on the GPU, with LEMON_JPEG=device their Huffman pass too (default pil: all by PIL); otherwise (or with LEMON_DECODE_WORKERS=0) PIL decode + generic_transform in a thread pool.
    Labels are ints (class datasets) or strings (captions)."""

    def __init__(self, images, clean, noisy, image_size=224, workers=8):
        assert len(images) == len(clean) == len(noisy)
        self.images, self.clean, self.noisy = images, clean, noisy
        self.image_size, self.workers = image_size, workers

    def __len__(self):
        return len(self.noisy)

    def subset(self, idx):
        pick = (lambda a: a[idx]) if isinstance(self.images, np.ndarray) else (lambda a: [a[i] for i in idx])
        lab = lambda a: a[idx] if isinstance(a, np.ndarray) else [a[i] for i in idx]
        return ImageLabelSet(pick(self.images), lab(self.clean), lab(self.noisy), self.image_size, self.workers)

    def _load(self, i):
        from PIL import Image
        item = self.images[i]
        img = Image.fromarray(item) if isinstance(item, np.ndarray) else Image.open(item).convert("RGB")
        return generic_transform(img, self.image_size)

    def batches(self, batch_size, lo=0, hi=None, device=None):
        """Yield (pixel_values [B,3,S,S] f32, clean[B], noisy[B]) in order (never shuffled, last batch
        short: SURVEY Appendix B.6).  PIL work runs in a thread pool (the reference forks 8 DataLoader
        workers, run_lemon.py:129-131; threads avoid fork-after-HIP-init)."""
        hi = len(self) if hi is None else hi
        if isinstance(self.images, np.ndarray) and self.images.dtype == np.float32:
            for s in range(lo, hi, batch_size):
                sl = slice(s, min(hi, s + batch_size))
                yield torch.from_numpy(np.ascontiguousarray(self.images[sl])), self.clean[sl], self.noisy[sl]
            return
        if device is not None and torch.device(device).type == "cuda" and isinstance(self.images, np.ndarray) \
                and self.images.dtype == np.uint8 and self.images.ndim == 4:
            # in-memory uint8 arrays (CIFAR): 3 KB per image cross PCIe instead of 602 KB, and the
            # bicubic up-sampling runs in lemon_preprocess_u8 (bit-identical to the PIL path below)
            for s in range(lo, hi, batch_size):
                sl = slice(s, min(hi, s + batch_size))
                u8 = torch.from_numpy(np.ascontiguousarray(self.images[sl])).to(device, non_blocking=True)
                yield gpu_transform_batch(u8, self.image_size), self.clean[sl], self.noisy[sl]
            return
        if device is not None and torch.device(device).type == "cuda" and isinstance(self.images, list) \
                and generic_transform is _GENERIC_TRANSFORM:
            # image files: decoded by a pool of worker processes ahead of the consumer, copied as uint8, and transformed on
            # the GPU as a ragged batch (lemon_amd/loader.py); LEMON_DECODE_WORKERS=0 keeps the thread path below, and so
            # does a transform other than generic_transform installed in this module (the GPU kernel computes that one only)
            from . import loader
            world = 1
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                world = torch.distributed.get_world_size()
            workers = loader.default_workers(world)
            if workers > 0:
                for s, e, imgs in loader.ragged_batches(self.images, batch_size, lo, hi, device, workers=workers):
                    yield imgs, self.clean[s:e], self.noisy[s:e]
                return
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            for s in range(lo, hi, batch_size):
                idx = range(s, min(hi, s + batch_size))
                px = torch.stack(list(pool.map(self._load, idx)))
                sl = slice(s, min(hi, s + batch_size))
                yield px, self.clean[sl], self.noisy[sl]


# ------------------------------------------------------------------------------ dataset factory
def synthetic_caption_frame(n, seed, n_cat=80, image_hw=32):
    """Stand-in for a caption dataset's `multimodal_mislabel_split.pkl` (lib/datasets/utils.py:275-323) when no data is
    present: n rows with the columns the reader uses -- split (train/val/test/restval in Karpathy-like proportions;
    restval rows are dropped by the reference's no-op remap), a UNIQUE sentence per row (a few exact
    duplicates, as in COCO), `cat_labels` / `nouns_int` id lists (some rows without categories) -- plus in-memory
    uint8 images [n, hw, hw, 3] whose pattern depends on the first category, so an encoder sees structure."""
    import pandas as pd
    rs = np.random.RandomState(seed)
    cats = [sorted(set(rs.randint(0, n_cat, rs.randint(1, 4)).tolist())) for _ in range(n)]
    for j in range(0, n, 53):
        cats[j] = []
    nouns = [sorted(set(rs.randint(0, 400, rs.randint(1, 6)).tolist())) for _ in range(n)]
    first = np.array([c[0] if c else rs.randint(0, n_cat) for c in cats])
    words = ["red", "small", "two", "wooden", "old", "bright", "open", "tall", "wet", "quiet", "busy", "empty"]
    sent = [f"a {words[i % 12]} {words[(i // 12) % 12]} scene number {i} showing object {first[i]} near thing {nouns[i][0]}"
            for i in range(n)]
    for j in range(7, n, 97):
        sent[j] = sent[j - 7]
    u = rs.rand(n)
    split = np.where(u < 0.66, "train", np.where(u < 0.70, "val", np.where(u < 0.74, "test", "restval"))).astype(object)
    cocoid = 100000 + rs.permutation(3 * n)[:n]
    pat = rs.randint(0, 256, (n_cat, image_hw, image_hw, 3)).astype(np.int16)
    px = np.clip(pat[first] + rs.randint(-64, 65, (n, image_hw, image_hw, 3)), 0, 255).astype(np.uint8)
    df = pd.DataFrame({"split": split, "filepath": "synthetic", "filename": [f"{c}.jpg" for c in cocoid], "sentence": sent,
                       "cat_labels": cats, "nouns_int": nouns}, index=cocoid)
    return df, px


def _read_cifar(root, name, train=True):
    """The CIFAR python pickles torchvision's CIFAR10 / CIFAR100(train=...) classes unpickle (lib/datasets/utils.py:356-386):
    uint8 [N, 32, 32, 3] images and the (fine) labels."""
    if name.startswith("cifar100"):
        with open(os.path.join(root, "cifar-100-python", "train" if train else "test"), "rb") as f:
            d = pickle.load(f, encoding="bytes")
        x, y = d[b"data"], np.array(d[b"fine_labels"])
    else:
        xs, ys = [], []
        for fn in ([f"data_batch_{i}" for i in range(1, 6)] if train else ["test_batch"]):
            with open(os.path.join(root, "cifar-10-batches-py", fn), "rb") as f:
                d = pickle.load(f, encoding="bytes")
            xs.append(d[b"data"]); ys += list(d[b"labels"])
        x, y = np.concatenate(xs), np.array(ys)
    return np.ascontiguousarray(x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)), y


CAPTION_DATASETS = ("mscoco", "flickr30k", "mimiccxr_caption", "mmimdb", "cc3m")


def cluster_text_labels(sets, embedder, tokenizer, n_clusters=100, random_state=42, **kmeans_kwargs):
    """lib/datasets/utils.py:312-316,396-400 + lib/datasets/dataloader.py:190-192: k-means on the embeddings of the NOISY
    train sentences, val / test predicted with the same model; every caption set becomes a label set with
    noisy = cluster id of the given sentence and clean = -1 where the sentence was swapped (is_mislabel), else the same id
    (int64).  Returns (km, (train, val, test)); the new sets keep the sentences as `.noisy_text` / `.clean_text`."""
    from . import kmeans
    train = sets[0]
    km, labels = kmeans.cluster_caption_text(embedder, tokenizer, list(train.noisy), n_clusters=n_clusters,
                                             random_state=random_state, **kmeans_kwargs)
    out = []
    for i, part in enumerate(sets):
        if i > 0:
            labels = km.predict(list(part.noisy)).squeeze(1).cpu().numpy() if len(part) else np.zeros(0, np.int64)
        noisy = np.asarray(labels, dtype=np.int64)
        mis = np.array([c != t for c, t in zip(part.clean, part.noisy)], dtype=bool)
        new = ImageLabelSet(part.images, np.where(mis, np.int64(-1), noisy), noisy, part.image_size, part.workers)
        new.noisy_text, new.clean_text, new.cluster_model = list(part.noisy), list(part.clean), km
        out.append(new)
    return km, tuple(out)


def _cluster_tools(cluster_kwargs):
    """(embedder, tokenizer, n_clusters, extra KMeans arguments) from get_dataset's cluster_kwargs: either a ready
    (`embedder`, `tokenizer`) pair or (`clip_model`, `clip_path`[, `bpe_path`, `device`, `encoder_batch`]), from which both are
    built the way lemon_amd/cli_common.py builds them."""
    kw = dict(cluster_kwargs or {})
    n_clusters = int(kw.pop("n_clusters", 100))
    embedder, tokenizer = kw.pop("embedder", None), kw.pop("tokenizer", None)
    clip_model, clip_path = kw.pop("clip_model", "huggingface_clip"), kw.pop("clip_path", None)
    bpe_path, device, batch = kw.pop("bpe_path", None), kw.pop("device", None), int(kw.pop("encoder_batch", 512))
    if (embedder is None) != (tokenizer is None):
        raise ValueError("cluster_kwargs: give both `embedder` and `tokenizer`, or `clip_model` and `clip_path`")
    if embedder is None:
        if clip_path is None:
            raise ValueError("cluster_kwargs needs (`embedder`, `tokenizer`) or (`clip_model`, `clip_path`) to embed the captions")
        from . import clip as clip_mod
        from .pipeline import Embedder
        model, tokenizer = clip_mod.algorithm_class_from_scratch(clip_model, text_base_name=clip_path, img_base=None,
                                                                 return_tokenizer=True, bpe_path=bpe_path)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        embedder = Embedder(model, device, batch_size=batch, text_dedup=True)
    return embedder, tokenizer, n_clusters, kw


def get_dataset(name, data_seed, percent_flips=0.40, flip_type="real", data_root="./data", image_size=224,
                cluster_text=False, cluster_kwargs=None):
    """train/val/test ImageLabelSets for the datasets run_lemon.py accepts (run_lemon.py:37-38,105-106).
    `data_root='synthetic:N'` builds an N-sample synthetic class dataset with the named dataset's labels.
    `cluster_text=True` (lib/datasets/utils.py:312-316,352,396-400) turns the captions of a caption dataset into cluster
    labels (cluster_text_labels; `cluster_kwargs`: n_clusters and the text tower, see _cluster_tools); class datasets ignore
    it, as upstream."""
    if cluster_text and name in CAPTION_DATASETS:
        sets = get_dataset(name, data_seed, percent_flips, flip_type, data_root, image_size)
        embedder, tokenizer, n_clusters, extra = _cluster_tools(cluster_kwargs)
        return cluster_text_labels(sets, embedder, tokenizer, n_clusters=n_clusters, **extra)[1]
    if name in ("cifar10", "cifar100"):
        C = ds.class_num_dict[name]
        if str(data_root).startswith("synthetic"):
            n = int(str(data_root).split(":")[1]) if ":" in str(data_root) else 5000
            rs = np.random.RandomState(data_seed)
            y = rs.randint(0, C, n)
            # seeded random CIFAR-shaped uint8 images: the same code path (and GPU preprocessing) as the real pickles
            images = rs.randint(0, 256, (n, 32, 32, 3), dtype=np.uint8)
        else:
            images, y = _read_cifar(data_root, name)
            n = len(y)
        noisy = np.asarray(ds.add_noisy_labels(name, flip_type, percent_flips, data_seed, list(y), data_root))
        tr, va, te = ds.split_80_10_10(n, data_seed)
        full = ImageLabelSet(images, y, noisy, image_size)
        return full.subset(tr), full.subset(va), full.subset(te)
    if name in ("cifar10_full", "cifar100_full"):
        # lib/datasets/utils.py:374-391: train / val = an 80 / 20 split of the training set, test = the dataset's own test
        # split, each with its own noise vector drawn with the same seed
        C = ds.class_num_dict[name]
        if str(data_root).startswith("synthetic"):
            n = int(str(data_root).split(":")[1]) if ":" in str(data_root) else 5000
            rs = np.random.RandomState(data_seed)
            y, y_te = rs.randint(0, C, n), rs.randint(0, C, max(n // 5, 1))
            images = rs.randint(0, 256, (n, 32, 32, 3), dtype=np.uint8)
            images_te = rs.randint(0, 256, (len(y_te), 32, 32, 3), dtype=np.uint8)
        else:
            images, y = _read_cifar(data_root, name, True)
            images_te, y_te = _read_cifar(data_root, name, False)
        noisy = np.asarray(ds.add_noisy_labels(name, flip_type, percent_flips, data_seed, list(y), data_root))
        noisy_te = np.asarray(ds.add_noisy_labels(name, flip_type, percent_flips, data_seed, list(y_te), data_root))
        tr, va = ds.split_80_20(len(y), data_seed)
        full = ImageLabelSet(images, y, noisy, image_size)
        return full.subset(tr), full.subset(va), ImageLabelSet(images_te, y_te, noisy_te, image_size)
    if name in ("mscoco", "flickr30k", "mimiccxr_caption", "mmimdb", "cc3m"):
        import pandas as pd
        pixels = None
        if str(data_root).startswith("synthetic"):
            n = int(str(data_root).split(":")[1]) if ":" in str(data_root) else 5000
            df, pixels = synthetic_caption_frame(n, data_seed)
        else:
            df = pd.read_pickle(os.path.join(data_root, "multimodal_mislabel_split.pkl"))
            # optional pre-decoded images aligned with the frame's rows: uint8 [N,H,W,3] (GPU preprocessing) or
            # float32 [N,...] (already preprocessed); replaces per-file JPEG decoding
            if os.path.exists(os.path.join(data_root, "pixels.npy")):
                pixels = np.load(os.path.join(data_root, "pixels.npy"), mmap_mode="r")
                assert len(pixels) == len(df), "pixels.npy must have one entry per frame row"
        if pixels is not None:         # position in pixels.npy = position in the frame AS LOADED (before any row is dropped)
            df = df.assign(_row=np.arange(len(df)))
        if "restval" in df.split:      # quirk kept: tests the Series INDEX
            df.loc[df.split == "restval", "split"] = "train"
        if name == "mimiccxr_caption":
            df = df[df.sentence.str.len() > 0]       # lib/datasets/utils.py:293
        if pixels is None and "path" not in df:
            df["path"] = [os.path.join(data_root, *(p for p in (r.get("filepath", ""), r["filename"]) if p))
                          for _, r in df.iterrows()]
        out = []
        for split in ("train", "val", "test"):
            part = df.query(f'split == "{split}"')
            if flip_type == "random":
                nd = ds.random_noise_dict(len(part), percent_flips, data_seed)
            elif flip_type == "noun":
                nd = ds.calc_noise_by_integer_matching(part["nouns_int"].values, percent_flips, data_seed)
            elif flip_type == "cat":
                nd = ds.calc_noise_by_integer_matching(part["cat_labels"].values, percent_flips, data_seed)
            else:
                raise NotImplementedError(flip_type)
            part = ds.noise_given_dict(part, nd)
            images = np.ascontiguousarray(pixels[part["_row"].values]) if pixels is not None else list(part["path"])
            if name == "mimiccxr_caption" and pixels is None:
                images = [mimic_image_path(p) for p in images]       # lib/datasets/dataloader.py:177-184
            out.append(ImageLabelSet(images, list(part["gold_sentence"]), list(part["sentence"]), image_size))
        return tuple(out)
    if name in ("stanford_cars", "mini_imagenet"):
        import pandas as pd
        from sklearn.model_selection import train_test_split
        assert flip_type == "real"
        df = pd.read_csv(os.path.join(data_root, "multimodal_mislabel_split.csv"))
        if "path" not in df:
            df["path"] = [os.path.join(data_root, f) for f in df["filename"]]
        trv, te = train_test_split(df.index, random_state=data_seed, train_size=0.75, stratify=df.is_clean)
        tr, va = train_test_split(trv, random_state=data_seed, train_size=0.5 / 0.75, stratify=df.loc[trv].is_clean)
        out = []
        for idx in (tr, va, te):
            part = df.loc[sorted(idx)]
            noisy = part["label"].values
            clean = np.where(part["is_clean"].values, noisy, noisy - 1)   # dataloader.py:130-131
            out.append(ImageLabelSet(list(part["path"]), clean, noisy, image_size))
        return tuple(out)
    raise NotImplementedError(name)
