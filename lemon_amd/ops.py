"""Host-side mirror of the reference's row-wise helpers, running on liblemon_hip.so.

  normalize_vectors      lib/utils/utils.py:39-40
  paired_distance        run_lemon.py:169,173,250-253
  d1_normalized          run_lemon.py:244-248
  calc_scores_given_hparams(_vectorized)   lib/metrics/utils.py:21-82

Inputs are torch CUDA tensors (device memory is torch's job; the arithmetic is the HIP
library's).  Host inputs are rejected loudly: there is no CPU path in the product.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

_METRICS = {"cosine": _lib.METRIC_IP, "ip": _lib.METRIC_IP, "euclidean": _lib.METRIC_L2,
            "l2": _lib.METRIC_L2, _lib.METRIC_IP: _lib.METRIC_IP, _lib.METRIC_L2: _lib.METRIC_L2}


def metric_id(metric):
    try:
        return _METRICS[metric]
    except KeyError:
        raise ValueError(f"unknown metric {metric!r} (cosine|euclidean)")


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dev_f32(t, name="tensor"):
    """Contiguous float32 CUDA tensor on a 16-byte boundary (converted or copied if needed); refuses CPU tensors.  The
    search entry points refuse rows that are not 16-byte aligned when d % 4 == 0 (include/lemon_hip.h, "row alignment"): a
    view that starts in the middle of a buffer is copied here so that they never see one."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a torch CUDA tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _lib.LemonHipError(f"{name} lives on {t.device}: the LEMoN hot path only runs on the GPU "
                                 "(no CPU fallback). Move it with .cuda().")
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(name, device, *args):
    """lib.<name>(*args, stream) with `device` current; raises LemonHipError on a non-zero status"""
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.load(), name)(*args, stream_ptr(device)), name)


def normalize_vectors(vectors):
    """F.normalize(vectors, p=2, dim=1) -- lib/utils/utils.py:39-40."""
    x = dev_f32(vectors, "vectors")
    assert x.dim() == 2
    y = torch.empty_like(x)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.lemon_normalize_rows(ptr(x), x.shape[0], x.shape[1], ptr(y), stream_ptr(x.device)),
                   "lemon_normalize_rows")
    return y


def our_metric(first, second, dist="cosine"):
    """DistanceEvaluator.our_metric (lib/metrics/distance_metrics.py:48-73): paired cosine /
    euclidean (not squared) / manhattan distance of un-normalised embeddings, without the reference's
    n x n detour.  Returns a CUDA float32 tensor [n]."""
    kind = {"cosine": 0, "euclidean": 1, "manhattan": 2}.get(dist)
    if kind is None:
        raise NotImplementedError(dist)
    a, b = dev_f32(first, "first"), dev_f32(second, "second")
    assert a.shape == b.shape and a.dim() == 2
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    lib = _lib.load()
    with torch.cuda.device(a.device):
        _lib.check(lib.lemon_paired_metric(kind, ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(out),
                                           stream_ptr(a.device)), "lemon_paired_metric")
    return out


def grid_f1(rec, y, hparams, xtol=1e-8, maxfun=500, return_scores=False):
    """Batched hyper-parameter grid: for every row (beta, gamma, tau_1_n, tau_2_n, tau_1_m, tau_2_m) of
    `hparams` [G,6] the F1-optimal threshold search of optimize_f1_efficient on the device-resident
    record `rec` (lemon_grid_f1) -> (f1 [G], thres [G]) numpy float64, bit-identical to the host loop."""
    import numpy as np
    dev = rec["D_n"].device
    f32 = lambda key: dev_f32(rec[key], key)
    d1, Dn, trn, dn, Dm, trm, dm = (f32(key) for key in ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m"))
    n, k = Dn.shape
    yb = torch.as_tensor(np.asarray(y).astype(bool).astype(np.uint8)).to(dev)
    hp = torch.as_tensor(np.asarray(hparams, dtype=np.float64).reshape(-1, 6)).to(dev)
    G = hp.shape[0]
    f1 = torch.empty(G, dtype=torch.float64, device=dev)
    th = torch.empty(G, dtype=torch.float64, device=dev)
    lib = _lib.load()
    chunk = max(1, min(65535, (1 << 30) // (8 * n)))             # <= 1 GiB of score workspace per launch
    ws = torch.empty((min(G, chunk), n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for g0 in range(0, G, chunk):
            g1 = min(G, g0 + chunk)
            _lib.check(lib.lemon_grid_f1(ptr(d1), ptr(Dn), ptr(trn), ptr(dn), ptr(Dm), ptr(trm), ptr(dm), ptr(yb), n, k,
                                         ptr(hp[g0:g1]), g1 - g0, float(xtol), int(maxfun), ptr(ws), ptr(f1[g0:g1]),
                                         ptr(th[g0:g1]), stream_ptr(dev)), "lemon_grid_f1")
    if return_scores:
        return f1.cpu().numpy(), th.cpu().numpy(), ws[:min(G, chunk)].cpu().numpy()
    return f1.cpu().numpy(), th.cpu().numpy()


def grid_f1_ks(rec, y, hparams, ks, xtol=1e-8, maxfun=500, return_scores=False):
    """grid_f1 for every k of `ks` from ONE record of depth kmax >= max(ks) (lemon_grid_f1_ks): the neighbour terms of all ks
    come from one walk over the record, once per distinct (tau_1, tau_2) pair of a side -> (f1 [K, G], thres [K, G]) numpy
    float64 (+ scores [K, G, n] with return_scores), row t bit-identical to grid_f1 on the contiguous [n, ks[t]] prefix.
    `ks` strictly ascending.  Chunked over G so that the workspace of a launch stays within 1 GiB."""
    dev = rec["D_n"].device
    f32 = lambda key: dev_f32(rec[key], key)
    d1, Dn, trn, dn, Dm, trm, dm = (f32(key) for key in ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m"))
    n, kmax = Dn.shape
    ks = [int(k) for k in ks]
    K = len(ks)
    yb = torch.as_tensor(np.asarray(y).astype(bool).astype(np.uint8)).to(dev)
    hp = np.ascontiguousarray(np.asarray(hparams, dtype=np.float64).reshape(-1, 6))
    G = hp.shape[0]
    lib = _lib.load()
    c_ks = (ctypes.c_int * max(K, 1))(*ks)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f1 = np.empty((K, G), dtype=np.float64)
    th = np.empty((K, G), dtype=np.float64)
    scores = np.empty((K, G, n), dtype=np.float64) if return_scores else None
    bound = 1 << 30

    def ws_bytes(g0, g1):
        b = lib.lemon_grid_f1_ks_workspace_bytes(n, K, g1 - g0, dp(hp[g0:g1]))
        if b < 0:
            _lib.check(-1, "lemon_grid_f1_ks_workspace_bytes")
        return b

    chunk = max(1, min(65535, G, bound // (8 * n * max(K, 1))))
    while chunk > 1 and any(ws_bytes(g0, min(G, g0 + chunk)) > bound for g0 in range(0, G, chunk)):
        chunk = (chunk + 1) // 2
    spans = [(g0, min(G, g0 + chunk)) for g0 in range(0, G, chunk)]
    need = max([ws_bytes(*sp) for sp in spans] + [8])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for g0, g1 in spans:
            f1c = torch.empty((K, g1 - g0), dtype=torch.float64, device=dev)
            thc = torch.empty((K, g1 - g0), dtype=torch.float64, device=dev)
            sc = torch.empty((K, g1 - g0, n), dtype=torch.float64, device=dev) if return_scores else None
            _lib.check(lib.lemon_grid_f1_ks(ptr(d1), ptr(Dn), ptr(trn), ptr(dn), ptr(Dm), ptr(trm), ptr(dm), ptr(yb), n, kmax,
                                            c_ks, K, dp(hp[g0:g1]), g1 - g0, float(xtol), int(maxfun), ptr(ws), need, ptr(sc),
                                            ptr(f1c), ptr(thc), stream_ptr(dev)), "lemon_grid_f1_ks")
            f1[:, g0:g1], th[:, g0:g1] = f1c.cpu().numpy(), thc.cpu().numpy()
            if return_scores:
                scores[:, g0:g1] = sc.cpu().numpy()
    return (f1, th, scores) if return_scores else (f1, th)


ATTENTION_MAX_SEQ = _lib.ATTENTION_MAX_SEQ    # the header's LEMON_ATTENTION_MAX_SEQ; beyond 288 tokens the streaming kernels
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
_ACT_CODE = {None: ACT_NONE, "silu": ACT_SILU, "gelu": ACT_GELU}      # 'gelu': the exact (erf) GELU of BiomedCLIP's towers
QUICK_GELU_SCALE = 1.702
_linear_tuned_loaded = set()      # device indices whose per-device hipBLASLt state has the recorded choices


def _ensure_linear_tuned(lib, device):
    """Hand the recorded hipBLASLt solution choices (lemon_amd/data/linear_gfx950.csv, or $LEMON_LINEAR_TUNED) to the
    library once per DEVICE: the library keeps one state per device (selected by hipGetDevice), so the file is loaded with
    `device` current -- a rank on cuda:3 gets the same solutions (same embedding bits, same speed) as rank 0.  A key that is
    not in the file uses the library's first-ranked solution (no timing; lemon_linear_set_tuning(1) turns timing on)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _linear_tuned_loaded:
        return
    _linear_tuned_loaded.add(idx)
    import os
    path = os.environ.get("LEMON_LINEAR_TUNED",
                          os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "linear_gfx950.csv"))
    if path and os.path.exists(path):
        with torch.cuda.device(device):
            lib.lemon_linear_load_tuned(path.encode())


def _linear_rows(name, x, weight, bias, residual, act, alpha):
    """The body linear and linear_split share: x [..., k] . weight [n, k]^T through the library GEMM entry `name` -> float32 [..., n]."""
    x, weight = x.contiguous(), weight.contiguous()
    k, n = x.shape[-1], weight.shape[0]
    y = torch.empty(x.shape[:-1] + (n,), dtype=torch.float32, device=x.device)
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == torch.float32
        residual = residual.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    _ensure_linear_tuned(_lib.load(), x.device)
    _call(name, x.device, ptr(x), ptr(weight), ptr(bias), ptr(residual), x.numel() // k, n, k, float(alpha), _ACT_CODE[act], ptr(y))
    return y


def linear(x, weight, bias=None, residual=None, act=None, alpha=1.0):
    """y = act(alpha * x @ weight.T + bias) (+ residual) in ONE hipBLASLt GEMM (SiLU / residual add ride
    in the epilogue; 'gelu', the exact one, is an in-place pass behind it).  x [..., k] float32 CUDA, weight [n, k]; act in
    (None, 'silu', 'gelu')."""
    assert x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
    assert weight.shape[1] == x.shape[-1]
    return _linear_rows("lemon_linear_f32", x, weight, bias, residual, act, alpha)


# ---- fp32-equivalent GEMMs on the 16-bit matrix cores (split operands: lemon_linear_bf16x6 / lemon_linear_f16x3) -----------
_SCHEMES = {"bf16x6": (torch.bfloat16, 6), "f16x3": (torch.float16, 3)}


_forced_gemm_mode = None          # set by gemm_mode_forced(): overrides $LEMON_GEMM for the calls inside the context


class gemm_mode_forced:
    """with gemm_mode_forced("bf16x6"): ... -- the GEMM mode of the towers for the calls inside, whatever $LEMON_GEMM says
    (pipeline.Embedder re-runs a micro-batch whose fp16 split operands overflowed with the range-free bf16 scheme)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        global _forced_gemm_mode
        self.prev, _forced_gemm_mode = _forced_gemm_mode, self.mode
        return self

    def __exit__(self, *exc):
        global _forced_gemm_mode
        _forced_gemm_mode = self.prev
        return False


def select_attention_arithmetic(mode):
    """The attention kernels' arithmetic follows the GEMM mode: split products on the fp16 matrix cores with 'f16x3' (inputs
    must stay inside the fp16 range, like the GEMM operands of that mode), v_mfma_f32_32x32x2_f32 with 'bf16x6' (the mode whose
    point is to have no range limit) and 'f32'.  $LEMON_ATTN_F16=0 keeps the fp32 form in every mode.  The library keeps the
    selection per calling thread (lemon_attention_set_f16) and this is called in front of every tower pass WITHOUT a host-side
    cache: a direct lemon_attention_set_f16 call, another embedder or another thread cannot leave a stale choice behind."""
    import os
    _lib.load().lemon_attention_set_f16(1 if (mode == "f16x3" and os.environ.get("LEMON_ATTN_F16", "1") != "0") else 0)


def gemm_mode():
    """How the four GEMMs of every transformer block run (LEMON_GEMM):
    'f16x3' (default): 2-way fp16 split operands, three cross products, one fp16 GEMM over 3k -- the fp32 GEMM's accuracy
        (max / rms error vs float64 measured slightly below it), 2.4x faster than the tuned fp32 GEMMs at the tower shapes;
    'bf16x6' (alias 'split'): 3-way bf16 split operands, six cross products, one bf16 GEMM over 6k (same delivered accuracy --
        fp32 accumulation bounds both --, no fp16 range limit on the operands, 1.4x faster than fp32);
    'f32': every GEMM on the fp32 matrix cores."""
    import os
    v = (_forced_gemm_mode or os.environ.get("LEMON_GEMM", DEFAULT_GEMM_MODE)).lower()
    if v in ("f32", "fp32", "0"):
        return "f32"
    if v in ("split", "bf16x6"):
        return "bf16x6"
    if v in ("f16x3", "fp16x3"):
        return "f16x3"
    raise ValueError(f"LEMON_GEMM={v!r}: expected f32, bf16x6 (split) or f16x3")


DEFAULT_GEMM_MODE = "f16x3"


def weight_scale_f16x3(w):
    """The power of two that lifts max|w| into [2^14, 2^15) -- the `wscale` of lemon_split_f16x3 (one host read per weight)."""
    mx = float(w.detach().abs().max())
    if not (mx > 0.0) or mx != mx or mx == float("inf"):
        return 1.0
    import math
    return 2.0 ** (15 - math.frexp(mx)[1])


def split_operand(x, mode="bf16x6", weight=False, wscale=1.0):
    """float32 [..., k] -> the split operand rows of `mode` ([..., 6k] bf16 or [..., 3k] fp16): activation layout, or the weight
    layout (f16x3: of x * wscale)."""
    dtype, seg = _SCHEMES[mode]
    assert x.is_cuda and x.dtype == torch.float32 and x.shape[-1] % 4 == 0
    x = x.contiguous()
    k = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (seg * k,), dtype=dtype, device=x.device)
    if mode == "bf16x6":
        _call("lemon_split3_f32", x.device, ptr(x), x.numel() // k, k, int(bool(weight)), ptr(y))
    else:
        _call("lemon_split_f16x3", x.device, ptr(x), x.numel() // k, k, int(bool(weight)), float(wscale), ptr(y))
    return y


def split3(x, weight=False):
    """float32 [..., k] -> bf16 [..., 6k] split operand rows (activation layout, or the weight layout)."""
    return split_operand(x, "bf16x6", weight)


def layer_norm_split(x, weight, bias, eps=1e-5, mode="bf16x6"):
    """LayerNorm whose output is the split activation operand of `mode` (one pass: lemon_layernorm_split3 / _f16x3)."""
    dtype, seg = _SCHEMES[mode]
    assert x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    width = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (seg * width,), dtype=dtype, device=x.device)
    lib = _lib.load()
    fn = lib.lemon_layernorm_split3 if mode == "bf16x6" else lib.lemon_layernorm_f16x3
    with torch.cuda.device(x.device):
        _lib.check(fn(ptr(x), ptr(weight.contiguous()), ptr(bias.contiguous()), float(eps), x.numel() // width, width, ptr(y),
                      stream_ptr(x.device)), "lemon_layernorm_" + mode)
    return y


def layer_norm_split3(x, weight, bias, eps=1e-5):
    return layer_norm_split(x, weight, bias, eps, "bf16x6")


def linear_split(xs, ws, bias=None, residual=None, act=None, alpha=1.0):
    """y = act(alpha * xs . ws^T + bias) (+ residual), float32, from split operands of one scheme (the dtype says which):
    bf16 [..., 6k] x [n, 6k] or fp16 [..., 3k] x [n, 3k].  f16x3: the caller folds 1 / wscale into alpha."""
    assert xs.is_cuda and xs.dtype == ws.dtype and xs.dtype in (torch.bfloat16, torch.float16) and xs.shape[-1] == ws.shape[1]
    return _linear_rows("lemon_linear_bf16x6" if xs.dtype == torch.bfloat16 else "lemon_linear_f16x3", xs, ws, bias, residual, act, alpha)


linear_split3 = linear_split


# ---- the MLP of a block in the hand-written split-fp16 GEMM (gemm_f16x3.hip: tile-major operands, fused fc1 epilogue) ----
def mlp_mode():
    """LEMON_MLP, with LEMON_GEMM=f16x3: 'block' (default): all four GEMMs of a block in the hand-written kernel (gemm_f16x3.hip):
    LayerNorm and attention write its tile-major operands, fc1's epilogue writes fc2's -- with the 16x16x32 kernel of round 4
    this is the fastest mode (35.6 k scores/s against 35.4 k for 'fused' on the same box; in round 3, with the 32x32x16 kernel,
    it was 2 % slower); 'fused': only the MLP there, QKV and the output projection in the library (lemon_linear_f16x3);
    'lib': the library GEMMs throughout, with the separate split pass."""
    import os
    v = os.environ.get("LEMON_MLP", "block").lower()
    if v not in ("block", "fused", "lib"):
        raise ValueError(f"LEMON_MLP={v!r}: expected block, fused or lib")
    return v


def mlp_fused_supported(width, mlp):
    return width % 256 == 0 and mlp % 256 == 0


def attention_head_dims():
    """The calling thread's head-dim mode (lemon_attention_get_head_dims): 0 = head_dim 64 only, 1 / 2 = multiples of 8 up to 128."""
    return int(_lib.load().lemon_attention_get_head_dims())


def set_attention_head_dims(mode):
    """lemon_attention_set_head_dims for the calling thread (initially $LEMON_ATTN_HEAD_DIMS, default 0) -> the previous mode."""
    lib = _lib.load()
    prev = lib.lemon_attention_get_head_dims()
    rc = lib.lemon_attention_set_head_dims(int(mode))
    if rc < 0:
        _lib.check(rc, "lemon_attention_set_head_dims")
    return int(prev)


def _attention_limits(hd, seq_len, head_dims, varlen=False):
    """The limits of csrc/attention_plan.hpp: head_dim 64, or with the head-dim mode on a multiple of 8 in 72 .. 128 (never with
    per-sequence lengths); seq_len up to ATTENTION_MAX_SEQ, with lengths up to what the one-workgroup kernels hold."""
    if varlen:
        return hd == 64 and seq_len <= ATTENTION_VARLEN_MAX_SEQ
    return seq_len <= ATTENTION_MAX_SEQ and (hd == 64 or (head_dims != 0 and hd % 8 == 0 and 64 < hd <= 128))


def _attention_takes(width, heads, seq_len, head_dims):
    return heads > 0 and width % heads == 0 and _attention_limits(width // heads, seq_len, head_dims)


def attention_supported(width, heads, seq_len):
    """Do the HIP attention kernels take this tower?  head_dim 64 always; multiples of 8 in 72 .. 128 with the head-dim mode on."""
    return _attention_takes(width, heads, seq_len, attention_head_dims())


def fused_width_max():
    """Widest residual stream the split-GEMM paths of a block take: 1024, or 2048 (what the LayerNorm and row-statistics kernels
    hold) with the head-dim mode on -- the towers beyond 1024 are the ones with head dims beyond 64."""
    return 2048 if attention_head_dims() != 0 else 1024


def block_fused_supported(width, mlp, heads, seq_len):
    """all four GEMMs of a block in the hand-written kernel: additionally 3 * width a multiple of 256 and the HIP attention"""
    return mlp_fused_supported(width, mlp) and (3 * width) % 256 == 0 and attention_supported(width, heads, seq_len)


# ---- which path a transformer block takes: the one place that decides (clip.Block and biomed.BertLayer branch on its fields) ----
# mode: gemm_mode().  qkv: 'torch' (CPU / autograd; the rest is then 'torch' / 'sdpa' too), 'f32' (lemon_linear_f32), 'split' (the
# library's split GEMMs), 'tiled' (the hand-written GEMM behind a LayerNorm kernel), 'tiled_ln' (the same, LayerNorm folded in).
# attn: 'sdpa' (PyTorch), 'f32' (ops.attention), 'split' / 'tiled' (attention_split / attention_t write the operand).  out, mlp: the
# output projection, fc1 + fc2 -- as qkv.  chain: forward_chain may chain the block, the residual stream at lean level `lean`.
BlockPlan = collections.namedtuple("BlockPlan", "mode qkv attn out mlp chain lean")


def block_plan(fused, width, mlp, heads, seq_len, pooled, carry, gemm_mode, mlp_mode, ln_fold, chain_res, head_dims, width_cap):
    """Pure: the BlockPlan of one block.  fused: CUDA fp32 input without autograd; pooled: only some rows of the block's output are
    wanted (the towers' last block); carry: the block in front left its operand and row statistics; width_cap: the widest
    residual stream the caller's split paths take."""
    if not fused:
        return BlockPlan(gemm_mode, "torch", "sdpa", "torch", "torch", False, 0)
    hip_attn = _attention_takes(width, heads, seq_len, head_dims)
    if gemm_mode == "f32" or width % 4 or width > width_cap:
        return BlockPlan(gemm_mode, "f32", "f32" if hip_attn else "sdpa", "f32", "f32", False, 0)
    hand_mlp = gemm_mode == "f16x3" and mlp_fused_supported(width, mlp)      # (3 * width is then a multiple of 256 too)
    hand = hand_mlp and mlp_mode == "block" and hip_attn
    if hand and not pooled:
        return BlockPlan(gemm_mode, "tiled", "tiled", "tiled", "tiled", bool(ln_fold), chain_res if ln_fold else 0)
    # a pooled block still needs every token's keys and values: its QKV GEMM stays in the hand-written kernel, the rest runs for
    # the pooled rows in the library
    qkv = "split" if not hand else "tiled_ln" if carry and ln_fold else "tiled"
    attn = "sdpa" if not hip_attn else "f32" if pooled else "split"
    return BlockPlan(gemm_mode, qkv, attn, "split", "tiled" if hand_mlp and not pooled and mlp_mode != "lib" else "split", False, 0)


def on_fused_path(x):
    return x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()


def current_block_plan(fused, width, mlp, heads, seq_len, pooled=False, carry=False, width_cap=None, head_dims=None):
    """block_plan under the knobs as they stand: LEMON_GEMM, LEMON_MLP, LEMON_LNFOLD, LEMON_CHAIN_RES and the thread's head-dim mode."""
    if not fused:          # CPU / autograd: no knob is read and the library is not asked
        return block_plan(False, width, mlp, heads, seq_len, pooled, carry, None, None, False, 0, 0, 0)
    hd = attention_head_dims() if head_dims is None else head_dims
    cap = (2048 if hd != 0 else 1024) if width_cap is None else width_cap           # (fused_width_max())
    return block_plan(fused, width, mlp, heads, seq_len, pooled, carry, gemm_mode(), mlp_mode(), ln_fold_enabled(), chain_operand_residual(),
                      hd, cap)


def _tiled_rows(m):
    return (m + 127) // 128 * 128


def pack_weight_t(w, wscale):
    """float32 [n, k] -> the tile-major fp16 weight operand of lemon_linear_f16x3t (of w * wscale)."""
    assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.shape[0] % 256 == 0 and w.shape[1] % 16 == 0
    w = w.contiguous()
    wt = torch.empty((w.shape[0] * w.shape[1] * 2,), dtype=torch.float16, device=w.device)
    _call("lemon_pack_weight_f16x3t", w.device, ptr(w), w.shape[0], w.shape[1], float(wscale), ptr(wt))
    return wt


def layer_norm_t(x, weight, bias, eps=1e-5):
    """LayerNorm whose output is the tile-major fp16 activation operand of lemon_linear_f16x3t (flat fp16 tensor)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.shape[-1] % 16 == 0
    x = x.contiguous()
    width = x.shape[-1]
    m = x.numel() // width
    at = torch.empty((_tiled_rows(m) * width * 2,), dtype=torch.float16, device=x.device)
    _call("lemon_layernorm_f16x3t", x.device, ptr(x), ptr(weight.contiguous()), ptr(bias.contiguous()), float(eps), m, width, ptr(at))
    return at


def _linear_t(entry, at, wt, m, n, k, bias=None, residual=None, act=None, alpha=1.0, out_shape=None, row_aff=None, colsum=None, emit=False,
              residual_t=None, fp32_out=True):
    """What linear_t, linear_t_ln and linear_t_chain share (`entry`: '', '_ln', '_chain' of lemon_linear_f16x3t): validation, output
    and emit allocation, contiguity, the call.  -> (out or None, emitted operand or None, its row-statistics partials or None)"""
    assert at.is_cuda and at.dtype == torch.float16 and wt.dtype == torch.float16
    assert at.numel() == _tiled_rows(m) * k * 2 and wt.numel() == n * k * 2 and (entry == "" or k % 32 == 0)
    assert (row_aff is None) == (colsum is None) and not (emit and row_aff is not None)
    assert residual is None or residual_t is None
    dev = at.device
    out = et = st = None
    if act is not None:
        assert act in ("silu", "gelu") and residual is None and not emit
        out = torch.empty((_tiled_rows(m) * n * 2,), dtype=torch.float16, device=dev)
    elif fp32_out:
        out = torch.empty(out_shape if out_shape is not None else (m, n), dtype=torch.float32, device=dev)
        assert out.numel() == m * n
    if bias is not None:
        bias = bias.contiguous()
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.numel() == m * n
        residual = residual.contiguous()
    if residual_t is not None:
        assert residual_t.dtype == torch.float16 and residual_t.numel() == _tiled_rows(m) * n * 2
    if row_aff is not None:
        assert row_aff.dtype == torch.float32 and row_aff.numel() == 2 * m and colsum.dtype == torch.float32 and colsum.numel() == n
        row_aff, colsum = row_aff.contiguous(), colsum.contiguous()
    if emit:
        et = torch.empty((_tiled_rows(m) * n * 2,), dtype=torch.float16, device=dev)
        st = torch.empty((m, n // 128, 2), dtype=torch.float32, device=dev)
    args = [ptr(at), ptr(wt), ptr(bias), ptr(residual)]
    if entry == "_chain":
        args += [ptr(residual_t), m, n, k, float(alpha), ptr(out), ptr(et), ptr(st)]
    else:
        args += [m, n, k, float(alpha), _ACT_CODE[act], int(act is not None), ptr(out)]
        if entry == "_ln":
            args += [ptr(row_aff), ptr(colsum), ptr(et), ptr(st)]
    _call("lemon_linear_f16x3t" + entry, dev, *args)
    return out, et, st


def linear_t(at, wt, m, n, k, bias=None, residual=None, act=None, alpha=1.0, out_shape=None):
    """lemon_linear_f16x3t on tile-major operands: act None -> float32 [m, n] (view `out_shape`) = alpha x W^T + bias (+ residual);
    act 'silu' / 'gelu' -> the tile-major activation operand (k' = n) of act(alpha x W^T + bias)."""
    return _linear_t("", at, wt, m, n, k, bias, residual, act, alpha, out_shape)[0]


LN_FOLD_MAX_SHIFT = 8.0     # csrc/common.hpp LEMON_LN_FOLD_MAX_SHIFT: rows with |mean| rstd beyond it get a NaN row affine (-> fallback)


_forced_ln_fold = None            # set by ln_fold_forced(): overrides $LEMON_LNFOLD for the calls inside the context


class ln_fold_forced:
    """with ln_fold_forced(False): ... -- the towers run their LayerNorms as kernels for the calls inside, whatever $LEMON_LNFOLD
    says (pipeline.Embedder re-runs a micro-batch whose rows were beyond the fold's mean bound this way first)."""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        global _forced_ln_fold
        self.prev, _forced_ln_fold = _forced_ln_fold, self.on
        return self

    def __exit__(self, *exc):
        global _forced_ln_fold
        _forced_ln_fold = self.prev
        return False


def ln_fold_enabled():
    """LEMON_LNFOLD (default 1): with LEMON_GEMM=f16x3 and LEMON_MLP=block the LayerNorms in front of QKV and fc1 are folded into
    the hand-written GEMMs (lemon_linear_f16x3t_ln): the output projection / fc2 write the residual stream also as the next
    GEMM's operand together with row statistics, QKV / fc1 apply (rstd, -mean rstd) and the weight-row sums in their epilogue --
    no LayerNorm pass over the token matrix.  0: LayerNorm kernels as before (A/B aid)."""
    import os
    if _forced_ln_fold is not None:
        return _forced_ln_fold
    return os.environ.get("LEMON_LNFOLD", "1") != "0"


def fold_layernorm_weight(w, b, gamma, beta, extra=1.0):
    """The weight side of a folded LayerNorm: LN(x) W^T + b = rstd (x W'^T - mean c) + b' with W' = W diag(gamma).  Returns
    (tile-major packed W' * wscale, 1 / wscale, colsum, bias'): colsum[n] = extra / wscale * sum_k of the PACKED weight row (hi + lo,
    float64 sum), bias' = extra * (b + W beta) -- `extra` is the factor the caller multiplies alpha = 1 / wscale with (QuickGELU's
    1.702 for fc1)."""
    wp = (w.detach() * gamma.detach()[None, :]).contiguous()
    wscale = weight_scale_f16x3(wp)
    wt = pack_weight_t(wp, wscale)
    t = wp * wscale                                       # exact: wscale is a power of two
    hi = t.to(torch.float16)
    lo = (t - hi.float()).to(torch.float16)               # split3.hpp split2h<WEIGHT = true>
    colsum = ((hi.double() + lo.double()).sum(1) * (extra / wscale)).float().contiguous()
    bias = (b.detach().double() if b is not None else 0.0) + w.detach().double() @ beta.detach().double()
    return wt, 1.0 / wscale, colsum, (bias * extra).float().contiguous()


def rowstats_t(x, eps):
    """x as the tile-major activation operand + its rows' (rstd, -mean rstd) [m, 2]: the input of a folded LayerNorm for a tensor
    no GEMM epilogue produced (lemon_rowstats_f16x3t)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.shape[-1] % 16 == 0
    x = x.contiguous()
    width = x.shape[-1]
    m = x.numel() // width
    at = torch.empty((_tiled_rows(m) * width * 2,), dtype=torch.float16, device=x.device)
    aff = torch.empty((m, 2), dtype=torch.float32, device=x.device)
    _call("lemon_rowstats_f16x3t", x.device, ptr(x), float(eps), m, width, ptr(at), ptr(aff))
    return at, aff


def ln_finalize(stats, m, width, eps):
    """[m, width / 128, 2] (mean, M2) partials of lemon_linear_f16x3t_ln's emit side -> (rstd, -mean rstd) [m, 2]."""
    assert stats.is_cuda and stats.dtype == torch.float32 and stats.numel() == m * (width // 128) * 2
    aff = torch.empty((m, 2), dtype=torch.float32, device=stats.device)
    _call("lemon_ln_finalize", stats.device, ptr(stats), m, width, float(eps), ptr(aff))
    return aff


def linear_t_ln(at, wt, m, n, k, bias=None, residual=None, act=None, alpha=1.0, out_shape=None, row_aff=None, colsum=None, emit=False):
    """linear_t with a folded LayerNorm on one side (lemon_linear_f16x3t_ln).  row_aff / colsum: this GEMM stands behind a LayerNorm
    whose input `at` holds (see fold_layernorm_weight / rowstats_t / ln_finalize).  emit: returns (out, out as the next GEMM's
    tile-major operand, its row-statistics partials [m, n / 128, 2])."""
    res = _linear_t("_ln", at, wt, m, n, k, bias, residual, act, alpha, out_shape, row_aff, colsum, emit)
    return res if emit else res[0]


def chain_operand_residual():
    """LEMON_CHAIN_RES: how the residual stream travels inside a block chain (ln_fold_enabled).
    2 (default): as the GEMMs' tile-major operand only -- the output projection and fc2 leave their result as the next GEMM's
       operand + row statistics (no fp32 tensor: 6 instead of 10 bytes written per element) and take their residual from the
       operand the GEMM in front left (hi + lo 2^-11: 22 significant bits per hop, the size of the terms the split products drop
       anyway); only the last chained block also writes fp32 (the pooled last block and the final LayerNorm read it);
    1: only the stream between the output projection and fc2 is carried that way (fc2 writes fp32 at every block boundary);
    0: fp32 residual stream between all GEMMs (A/B aid)."""
    import os
    v = os.environ.get("LEMON_CHAIN_RES", "2")
    return 0 if v == "0" else (1 if v == "1" else 2)


def linear_t_chain(at, wt, m, n, k, bias=None, residual=None, residual_t=None, alpha=1.0, out_shape=None, fp32_out=True):
    """lemon_linear_f16x3t_chain: alpha x W^T + bias + residual -> (fp32 [m, n] or None, the same as the next GEMM's tile-major
    operand, its row-statistics partials [m, n / 128, 2]); the residual is fp32 [m, n] (`residual`) or a tile-major operand
    (`residual_t`)."""
    return _linear_t("_chain", at, wt, m, n, k, bias, residual, None, alpha, out_shape, emit=True, residual_t=residual_t, fp32_out=fp32_out)


def gemm_profiling(on):
    """HIP events around every lemon_linear_f16x3t launch from now on (bench.py: the roofline of the step's dominant kernel)."""
    _lib.check(_lib.load().lemon_linear_f16x3t_set_profiling(int(bool(on))), "lemon_linear_f16x3t_set_profiling")


def gemm_profile_read():
    """{launches, kernel_ms, flops} of the bracketed launches since the last read (waits for them; rewinds the event pool)."""
    n, ms, fl = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    _lib.check(_lib.load().lemon_linear_f16x3t_profile_read(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)),
               "lemon_linear_f16x3t_profile_read")
    return {"launches": int(n.value), "kernel_ms": float(ms.value), "flops": float(fl.value)}


ATTENTION_VARLEN_MAX_SEQ = 288     # the one-workgroup kernels: the streaming kernels take no per-sequence lengths


def attention_varlen_supported(width, heads, seq_len):
    """Do the lemon_attention_*_varlen entry points (a key length per sequence) take this tower at this token count?"""
    return heads > 0 and width % heads == 0 and seq_len >= 1 and _attention_limits(width // heads, seq_len, 0, varlen=True)


def attention_lengths(lengths, batch, device):
    """-> int32 [batch] on `device`: a CUDA tensor as it is (converted if need be), a host sequence / tensor through a pinned
    staging buffer and a non-blocking copy -- no synchronisation either way."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        t = lengths.to(device=device, dtype=torch.int32).contiguous()
    else:
        host = torch.as_tensor(lengths).to(torch.int32).reshape(-1).contiguous()
        t = host.pin_memory().to(device, non_blocking=True)
    assert t.dim() == 1 and t.shape[0] == batch, (tuple(t.shape), batch)
    return t


def _varlen_args(lengths, causal, B, L, heads, hd, device):
    assert not causal, "per-sequence lengths: bidirectional attention only (padding behind a caption is invisible under a causal mask)"
    if not _attention_limits(hd, L, 0, varlen=True):
        raise ValueError(f"attention with per-sequence lengths: head_dim 64 and seq_len <= {ATTENTION_VARLEN_MAX_SEQ} "
                         f"(got head_dim {hd}, seq_len {L}); see ops.attention_varlen_supported")
    return attention_lengths(lengths, B, device)


def _attention(form, qkv, heads, causal, lengths):
    """The one attention call behind attention (form 'f32'), attention_split ('split3' / 'f16x3') and attention_t ('f16x3t'): shape
    checks, the output of that form, the entry with or without per-sequence lengths."""
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and (form != "f32" or qkv.is_contiguous())
    qkv = qkv.contiguous()
    B, L, W3 = qkv.shape
    W = W3 // 3
    hd = W // heads
    assert W3 == 3 * W and W == heads * hd and (form != "f16x3t" or W % 16 == 0) and L <= ATTENTION_MAX_SEQ
    if form == "f16x3t":
        out = torch.empty((_tiled_rows(B * L) * W * 2,), dtype=torch.float16, device=qkv.device)
    else:
        dtype, seg = (torch.float32, 1) if form == "f32" else _SCHEMES["bf16x6" if form == "split3" else form]
        out = torch.empty((B, L, seg * W), dtype=dtype, device=qkv.device)
    name = "lemon_attention_" + form + ("_varlen" if lengths is not None else "")
    with torch.cuda.device(qkv.device):
        how = ptr(_varlen_args(lengths, causal, B, L, heads, hd, qkv.device)) if lengths is not None else int(bool(causal))
        _lib.check(getattr(_lib.load(), name)(ptr(qkv), B, L, heads, hd, how, ptr(out), stream_ptr(qkv.device)), name.replace("split3", "bf16x6"))
    return out


def attention_t(qkv, heads, causal=False, lengths=None):
    """attention() whose output is the tile-major fp16 activation operand of lemon_linear_f16x3t (rows = B*L, k = W = heads*head_dim,
    a multiple of 16).  lengths: see attention()."""
    return _attention("f16x3t", qkv, heads, causal, lengths)


def unpack_act_t(at, m, k):
    """tile-major activation operand -> float32 [m, k] (hi + lo 2^-11)."""
    y = torch.empty((m, k), dtype=torch.float32, device=at.device)
    _call("lemon_unpack_act_f16x3t", at.device, ptr(at), m, k, ptr(y))
    return y


def layer_norm(x, weight, bias, eps=1e-5):
    """nn.LayerNorm over the last dimension of a float32 CUDA tensor in one HIP pass (lemon_layernorm_f32)."""
    assert x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    width = x.shape[-1]
    y = torch.empty_like(x)
    _call("lemon_layernorm_f32", x.device, ptr(x), ptr(weight.contiguous()), ptr(bias.contiguous()), float(eps), x.numel() // width, width, ptr(y))
    return y


def vision_tokens_ln(patches, cls, pos, ln_weight, ln_bias, eps=1e-5):
    """[B, nP, W] patch embeddings -> pre-LayerNormed token matrix [B, nP+1, W] (class token + positions) in one pass;
    ln_weight = ln_bias = None: token assembly without the LayerNorm (timm ViT)."""
    assert patches.is_cuda and patches.dtype == torch.float32 and patches.dim() == 3
    patches = patches.contiguous()
    B, nP, W = patches.shape
    y = torch.empty((B, nP + 1, W), dtype=torch.float32, device=patches.device)
    ln = [ptr(t.contiguous()) if t is not None else None for t in (ln_weight, ln_bias)]
    _call("lemon_vision_tokens_ln", patches.device, ptr(patches), ptr(cls.contiguous()), ptr(pos.contiguous()), *ln, float(eps), B, nP + 1, W, ptr(y))
    return y


def text_tokens(input_ids, seq_len, tok_weight, pos):
    """tok_weight[ids[:, :seq_len]] + pos[:seq_len] -> [B, seq_len, W] in one pass (ids int64 CUDA [B, ctx])."""
    assert input_ids.is_cuda and input_ids.dtype == torch.int64 and input_ids.dim() == 2 and input_ids.stride(1) == 1
    B, W = input_ids.shape[0], tok_weight.shape[1]
    y = torch.empty((B, seq_len, W), dtype=torch.float32, device=input_ids.device)
    _call("lemon_text_tokens", input_ids.device, ptr(input_ids), input_ids.stride(0), ptr(tok_weight.contiguous()), ptr(pos.contiguous()), B,
          int(seq_len), W, tok_weight.shape[0], ptr(y))
    return y


def linear_dump_tuned(path):
    """Write the solution choices made so far in this process (tools/tune_gemms.py)."""
    return _lib.load().lemon_linear_dump_tuned(str(path).encode())


def attention(qkv, heads, causal=False, lengths=None):
    """Fused self-attention on the packed projection output qkv [B, L, 3*W] (float32, contiguous,
    W = heads*head_dim; head_dim 64, or see attention_supported) -> [B, L, W]; the HIP kernel behind LemonCLIP's blocks.
    lengths: None, or the key count of every sequence -- an int32 CUDA tensor [B], or a host sequence (uploaded without a
    synchronisation): sequence b attends to its first clamp(lengths[b], 1, L) tokens only and its rows beyond them come out as
    zeros (lemon_attention_*_varlen: bidirectional, head_dim 64, L <= 288, see attention_varlen_supported)."""
    return _attention("f32", qkv, heads, causal, lengths)


def attention_split(qkv, heads, causal=False, mode="bf16x6", lengths=None):
    """attention() whose output is the split activation operand of `mode`: [B, L, 6*W] bf16 (lemon_attention_split3) or
    [B, L, 3*W] fp16 (lemon_attention_f16x3).  lengths: see attention()."""
    return _attention({"bf16x6": "split3", "f16x3": "f16x3"}[mode], qkv, heads, causal, lengths)


def attention_split3(qkv, heads, causal=False):
    return attention_split(qkv, heads, causal, "bf16x6")


def paired_distance(metric, a, b):
    a, b = dev_f32(a, "a"), dev_f32(b, "b")
    assert a.shape == b.shape and a.dim() == 2
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    lib = _lib.load()
    with torch.cuda.device(a.device):
        _lib.check(lib.lemon_paired_distance(metric_id(metric), ptr(a), ptr(b), a.shape[0], a.shape[1],
                                             ptr(out), stream_ptr(a.device)), "lemon_paired_distance")
    return out


def checked_labels(noisy_label, n, C, device):
    """The noisy labels as an int32 tensor on `device`, checked first: the kernels compare them with class numbers and
    quietly give 0 for one outside [0, C), where the reference's `softmax(...)[label]` raises (>= C) or wraps round (< 0).
    Labels arrive on the host (run_lemon.py:244-248 reads them from the dataset's metadata), where the check is free; a
    tensor that is already on a device is checked there (one read-back)."""
    lab = torch.as_tensor(noisy_label)
    if lab.dim() != 1 or lab.shape[0] != n:
        raise ValueError(f"noisy_label: expected {n} labels, got shape {tuple(lab.shape)}")
    if n and (lab.is_floating_point() or lab.dtype == torch.bool):
        raise ValueError(f"noisy_label: expected integer class numbers, got {lab.dtype}")
    if n and (int(lab.min()) < 0 or int(lab.max()) >= C):
        raise ValueError(f"noisy_label: every label must lie in [0, {C}), got {int(lab.min())} .. {int(lab.max())}")
    return lab.to(device=device, dtype=torch.int32).contiguous()


def d1_normalized(metric, q_img, cls_txt, noisy_label):
    q, c = dev_f32(q_img, "q_img"), dev_f32(cls_txt, "cls_txt")
    if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1]:
        raise ValueError(f"q_img {tuple(q.shape)} and cls_txt {tuple(c.shape)} must be [n, d] and [C, d] with the same d")
    lab = checked_labels(noisy_label, q.shape[0], c.shape[0], q.device)
    out = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        _lib.check(lib.lemon_d1_normalized(metric_id(metric), ptr(q), q.shape[0], q.shape[1], ptr(c),
                                           c.shape[0], ptr(lab), ptr(out), stream_ptr(q.device)),
                   "lemon_d1_normalized")
    return out


HP_ORDER = ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")


def lemon_score(rec, hparams, return_dn=False):
    """Score aggregation on device arrays.  rec: dict with d_1 [n], D_n, dists_tr_n, dists_n, D_m,
    dists_tr_m, dists_m [n,k] CUDA tensors.  Returns float64 CUDA tensors."""
    names = ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")
    arrs = [dev_f32(rec[nm], nm) for nm in names]
    n, k = arrs[1].shape
    dev = arrs[0].device
    score = torch.empty(n, dtype=torch.float64, device=dev)
    dn = torch.empty(n, dtype=torch.float64, device=dev)
    dm = torch.empty(n, dtype=torch.float64, device=dev)
    hp = (ctypes.c_double * 6)(*[float(hparams[h]) for h in HP_ORDER])
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.lemon_score(*[ptr(a) for a in arrs], n, k, hp, ptr(score), ptr(dn), ptr(dm),
                                   stream_ptr(dev)), "lemon_score")
    return (score, dn, dm) if return_dn else score


def _force_masks(force_zero, force_one):
    return (sum(1 << HP_ORDER.index(nm) for nm in set(force_zero)), sum(1 << HP_ORDER.index(nm) for nm in set(force_one)))


def _cell_masks(what, force_zero, force_one, cells):
    """[(force_zero mask, force_one mask), ...]: of `cells`, a non-empty list of (force_zero, force_one) name pairs, or of the
    one pair force_zero / force_one where cells is None."""
    if cells is None:
        return [_force_masks(force_zero, force_one)]
    if force_zero or force_one:
        raise ValueError(f"{what}: give the force masks either as force_zero= / force_one= or as cells=, not both")
    cells = list(cells)
    if not cells:
        raise ValueError(f"{what}: cells is empty; expected a list of (force_zero, force_one) pairs")
    return [_force_masks(fz, fo) for fz, fo in cells]


def _by_cell(rows, n_cells, n_ks, per_k, ks, cells):
    """rows in spec's order (cell, k, the per_k results of one k) -> what the caller asked for: per cell where `cells` was
    given, per k where `ks` was given."""
    per = [rows[c * n_ks * per_k:(c + 1) * n_ks * per_k] for c in range(n_cells)]
    if ks is not None:
        per = [[r[t * per_k:(t + 1) * per_k] for t in range(n_ks)] for r in per]
    return per[0] if cells is None else per


def local_search(rec, y, x0s, methods=("Powell", "Nelder-Mead"), force_zero=(), force_one=(), ks=None, return_info=False,
                 cells=None):
    """The scipy local searches of maximize_metric (lib/metrics/utils.py:151-158) on the device-resident record `rec`, all in
    ONE launch and one copy back (lemon_hparam_search): for each x0 of `x0s`, for each method -- the reference's order -- what
    scipy.optimize.minimize(objective, x0, method=method, options={}) returns on maximize_metric's objective, bit for bit.
    -> [(x [6] float64, fun), ...]; with `ks` (values of knn_k, each <= the record's depth: a search sees the [n, k] prefix)
    one such list per k.  return_info: (x, fun, nfev, nit, status) instead.  force_zero / force_one: names of HP_ORDER.
    cells=[(force_zero, force_one), ...]: the searches of several mask pairs on the same record -- the ablations of a cell
    sweep -- still in ONE launch (for each cell, each k, each x0, each method) -> one entry per cell, each what the call with
    that pair as force_zero / force_one returns, bit for bit (a search is one workgroup and sees only its own row of spec)."""
    dev = rec["D_n"].device
    f32 = lambda key: dev_f32(rec[key], key)
    d1, Dn, trn, dn, Dm, trm, dm = (f32(key) for key in ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m"))
    n, kmax = Dn.shape
    k_list = [kmax] if ks is None else [int(k) for k in ks]
    if any(k < 1 or k > kmax for k in k_list):
        raise ValueError(f"local_search: every k must lie in 1 .. {kmax} (the record's depth), got {k_list}")
    unknown = [m for m in methods if m not in _lib.SEARCH_METHODS]
    if unknown:
        raise ValueError(f"local_search: unknown method(s) {unknown}; the device path has {sorted(_lib.SEARCH_METHODS)}")
    masks = _cell_masks("local_search", force_zero, force_one, cells)
    x0s = np.asarray(x0s, dtype=np.float64).reshape(-1, 6)
    per_k = len(x0s) * len(methods)
    S = per_k * len(k_list) * len(masks)
    shaped = lambda rows: _by_cell(rows, len(masks), len(k_list), per_k, ks, cells)
    if S == 0:
        return shaped([])
    x0 = np.repeat(np.tile(x0s, (len(masks) * len(k_list), 1)), len(methods), axis=0)  # for each cell, each k, each x0, each method
    spec = np.array([[_lib.SEARCH_METHODS[m], k, fz, fo] for fz, fo in masks for k in k_list for _ in range(len(x0s)) for m in methods],
                    dtype=np.int32)
    lib = _lib.load()
    need = lib.lemon_hparam_search_workspace_bytes(n, S)
    if need < 0:
        _lib.check(int(need), "lemon_hparam_search_workspace_bytes")
    yb = torch.as_tensor(np.asarray(y).astype(bool).astype(np.uint8)).to(dev)
    x0_d, spec_d = torch.from_numpy(x0).to(dev), torch.from_numpy(spec).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(S * ctypes.sizeof(_lib.SearchResult), dtype=torch.uint8, device=dev)
    _call("lemon_hparam_search", dev, ptr(d1), ptr(Dn), ptr(trn), ptr(dn), ptr(Dm), ptr(trm), ptr(dm), ptr(yb), n, kmax, S,
          ptr(x0_d), ptr(spec_d), ptr(ws), need, ptr(out))
    res = (_lib.SearchResult * S).from_buffer_copy(out.cpu().numpy().tobytes())
    rows = [(np.array(list(r.x), dtype=np.float64), float(r.fun)) + ((int(r.nfev), int(r.nit), int(r.status)) if return_info else ())
            for r in res]
    bad = [s for s, r in enumerate(res) if r.status == 5]
    if bad:
        raise _lib.LemonHipError(f"lemon_hparam_search: search(es) {bad} ended at the iteration limit of scipy's bracket(), where "
                                 "scipy.optimize.minimize raises RuntimeError")
    return shaped(rows)


def lbfgs_polish(rec, y, x0s, force_zero=(), force_one=(), ks=None, return_info=False, cells=None):
    """The LBFGS polish of maximize_metric (lib/metrics/utils.py:160-176) on the device-resident record `rec`, all start points
    in ONE launch and one copy back (lemon_lbfgs_polish): for each x0 of `x0s` -- the reference's order -- the x that 20
    optimizer.step calls of torch.optim.LBFGS leave on the SoftMargin proxy, computed in fixed-order IEEE double (a function of
    the record alone; not bit-compatible with torch's own float32-promoted run, see include/lemon_hip.h).
    -> [(x [6] float64, status), ...], status 1 = x or the loss is not finite; with `ks` (values of knn_k, each <= the record's
    depth: a polish sees the [n, k] prefix) one such list per k.  return_info: (x, status, loss, nfev, nit) instead.
    force_zero / force_one: names of HP_ORDER.  cells=[(force_zero, force_one), ...]: as in local_search -- the polishes of
    several mask pairs in ONE launch (for each cell, each k, each x0) -> one entry per cell, each what the call with that pair
    returns, bit for bit."""
    dev = rec["D_n"].device
    f32 = lambda key: dev_f32(rec[key], key)
    d1, Dn, trn, dn, Dm, trm, dm = (f32(key) for key in ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m"))
    n, kmax = Dn.shape
    k_list = [kmax] if ks is None else [int(k) for k in ks]
    if any(k < 1 or k > kmax for k in k_list):
        raise ValueError(f"lbfgs_polish: every k must lie in 1 .. {kmax} (the record's depth), got {k_list}")
    masks = _cell_masks("lbfgs_polish", force_zero, force_one, cells)
    x0s = np.asarray(x0s, dtype=np.float64).reshape(-1, 6)
    per_k = len(x0s)
    S = per_k * len(k_list) * len(masks)
    shaped = lambda rows: _by_cell(rows, len(masks), len(k_list), per_k, ks, cells)
    if S == 0:
        return shaped([])
    x0 = np.tile(x0s, (len(masks) * len(k_list), 1))                                  # for each cell, each k, each x0
    spec = np.array([[k, fz, fo] for fz, fo in masks for k in k_list for _ in range(per_k)], dtype=np.int32)
    yb = torch.as_tensor(np.asarray(y).astype(bool).astype(np.uint8)).to(dev)
    x0_d, spec_d = torch.from_numpy(x0).to(dev), torch.from_numpy(spec).to(dev)
    out = torch.empty(S * ctypes.sizeof(_lib.PolishResult), dtype=torch.uint8, device=dev)
    _call("lemon_lbfgs_polish", dev, ptr(d1), ptr(Dn), ptr(trn), ptr(dn), ptr(Dm), ptr(trm), ptr(dm), ptr(yb), n, kmax, S,
          ptr(x0_d), ptr(spec_d), _lib.POLISH_OUTER_STEPS, ptr(out))
    res = (_lib.PolishResult * S).from_buffer_copy(out.cpu().numpy().tobytes())
    rows = [(np.array(list(r.x), dtype=np.float64), int(r.status)) + ((float(r.loss), int(r.nfev), int(r.nit)) if return_info else ())
            for r in res]
    return shaped(rows)


EVAL_THRESHOLDS = ("F1_optimal", "F1_prev", "F1_heuristic")      # the order of LemonEvalRecord.thres / .counts


def eval_segments(segments):
    """[(offset, n, prevalence, thres_from), ...] -> a ctypes array of LemonEvalSegment"""
    arr = (_lib.EvalSegment * len(segments))()
    for g, (offset, n, prevalence, thres_from) in zip(arr, segments):
        g.offset, g.n, g.prevalence, g.thres_from, g.pad = int(offset), int(n), float(prevalence), int(thres_from), 0
    return arr


def _binary_from_counts(tp, fp, fn, tn, suffix):
    """metrics.binary_metrics(targets, score >= t, suffix=suffix) from the four counts: its keys in its order, its arithmetic
    on Python ints (sklearn's accuracy, F1 and balanced accuracy are these quotients), its Python types -- the ints 0 / 1
    where the reference assigns ints."""
    n = tp + fp + fn + tn
    res = {"accuracy": (tp + tn) / n, "F1": 2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0, "n_samples": n}
    res.update(TN=tn, FN=fn, TP=tp, FP=fp, error=fn + fp)
    res["TPR"], res["FNR"] = ((tp / (tp + fn), fn / (tp + fn)) if tp + fn else (0, 1))
    res["FPR"], res["TNR"] = ((fp / (fp + tn), tn / (fp + tn)) if fp + tn else (1, 0))
    res["PPV"] = tp / (tp + fp) if tp + fp > 0 else 0
    res["NPV"] = tn / (tn + fn) if tn + fn > 0 else 0
    res["pred_prevalence"] = (tp + fp) / n
    res["prevalence"] = (tp + fn) / n
    if tp + fn and fp + tn:
        res["balanced_acc"] = (tn / (tn + fp) + tp / (tp + fn)) / 2.0
    return {f"{k}{suffix}": v for k, v in res.items()}


def eval_status_error(s, status):
    """The exception of segment s with a non-zero status: the class the host path raises first (sklearn's and gaussian_kde's
    ValueError, numpy.linalg.LinAlgError where scipy's Cholesky meets a zero variance)."""
    if status == _lib.EVAL_ZERO_VARIANCE:
        return np.linalg.LinAlgError(f"eval_metrics: segment {s}: the scores have zero variance, the KDE's covariance is singular")
    why = {_lib.EVAL_NONFINITE: "a score is not finite", _lib.EVAL_ONE_CLASS: "only one class is present, AUROC is not defined",
           _lib.EVAL_FEW_ROWS: "the KDE needs at least two rows",
           _lib.EVAL_SOURCE: "the segment its thresholds come from could not be served"}.get(status, f"status {status}")
    return ValueError(f"eval_metrics: segment {s}: {why}")


def eval_record_dict(rec, source=None):
    """A LemonEvalRecord -> the dict of metrics.eval_metrics: its keys in its order, its Python types (AUROC / AUPRC float, the
    F1_optimal and F1_heuristic thresholds numpy.float64, the F1_prev threshold the float of scipy's bisect or fminbound's
    numpy.float64).  source: the record of the free segment a fixed one was counted at (None: rec is free itself)."""
    source = rec if source is None else source
    t_opt, t_prev, t_heur = (float(t) for t in rec.thres)
    out = {"AUROC": float(rec.auroc), "AUPRC": float(rec.auprc), "F1_optimal_thres": np.float64(t_opt),
           "F1_prev_thres": np.float64(t_prev) if source.bisect_fallback else t_prev, "F1_heuristic_thres": np.float64(t_heur)}
    for k, name in enumerate(EVAL_THRESHOLDS):
        tp, fp, fn, tn = (int(c) for c in rec.counts[k])
        out.update(_binary_from_counts(tp, fp, fn, tn, name[len("F1"):]))
    return out


def eval_records_dicts(records, segments):
    """the dicts of all segments; raises the exception of the first free segment with a status, else of the first fixed one
    (the host path evaluates the free rows first)"""
    order = sorted(range(len(segments)), key=lambda s: (segments[s][3] != -1, s))
    for s in order:
        if records[s].status != _lib.EVAL_OK:
            raise eval_status_error(s, records[s].status)
    return [eval_record_dict(r, None if g[3] == -1 else records[g[3]]) for r, g in zip(records, segments)]


def eval_metrics_records(score, y, segments):
    """lemon_eval_metrics on device tensors: score float64 [total], y uint8 [total], segments [(offset, n, prevalence,
    thres_from), ...] -> [LemonEvalRecord, ...] (one launch sequence, one copy back; a status is reported, not raised)"""
    if not (torch.is_tensor(score) and score.is_cuda and torch.is_tensor(y) and y.is_cuda):
        raise _lib.LemonHipError("eval_metrics: score and y must be CUDA tensors (no CPU fallback for the device path)")
    if score.dtype != torch.float64 or y.dtype != torch.uint8 or score.dim() != 1 or y.shape != score.shape:
        raise TypeError("eval_metrics: score float64 [total] and y uint8 [total] expected")
    score, y, dev = score.contiguous(), y.contiguous(), score.device
    S, total = len(segments), score.shape[0]
    lib = _lib.load()
    need = lib.lemon_eval_metrics_workspace_bytes(total, S, sum(1 for g in segments if g[3] == -1))
    if need < 0:
        _lib.check(int(need), "lemon_eval_metrics_workspace_bytes")
    segs_d = torch.frombuffer(bytearray(bytes(eval_segments(segments))), dtype=torch.uint8).to(dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(S * ctypes.sizeof(_lib.EvalRecord), dtype=torch.uint8, device=dev)
    _call("lemon_eval_metrics", dev, ptr(score), ptr(y), total, ptr(segs_d), S, ptr(ws), need, ptr(out))
    return list((_lib.EvalRecord * S).from_buffer_copy(out.cpu().numpy().tobytes()))


def eval_metrics(score, y, segments):
    """metrics.eval_metrics for every segment of one device-resident score in ONE call (lemon_eval_metrics): a free segment
    (thres_from -1) finds its three thresholds on its own rows, a fixed one is counted at the thresholds of the free segment
    thres_from names -- the val -> train / val / test pattern of a run.  -> one dict per segment with the keys, order and
    Python types of metrics.eval_metrics; thresholds, counts and count-derived values equal the host path by their bits, AUROC
    is the correctly rounded exact value and AUPRC a fixed-order sum (both within n 2^-52 of sklearn).  A segment that cannot
    be served raises what the host path raises first: ValueError (a non-finite score, one class, fewer than two free rows),
    numpy.linalg.LinAlgError (zero variance)."""
    segments = [tuple(g) for g in segments]
    return eval_records_dicts(eval_metrics_records(score, y, segments), segments)


def _stack_col(df, col, device):
    return torch.from_numpy(np.stack(df[col].values).astype(np.float32, copy=False)).to(device)


def calc_scores_given_hparams_vectorized(df, best_hparams, return_dn=False, torch_arr=False, device="cuda"):
    """Drop-in for lib/metrics/utils.py:47-82 on the reference's DataFrame schema
    (run_lemon.py:291-307): returns numpy arrays (torch CPU tensors when torch_arr)."""
    rec = {c: _stack_col(df, c, device) for c in ("D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")}
    rec["d_1"] = torch.from_numpy(np.asarray(df["d_1"].values, dtype=np.float32)).to(device)
    s, dn, dm = lemon_score(rec, best_hparams, return_dn=True)
    # d_1 is float64 in the reference frame (`d1.item()`): add it back at full precision
    s = s - rec["d_1"].double() + torch.from_numpy(np.asarray(df["d_1"].values, dtype=np.float64)).to(device)
    conv = (lambda t: t.cpu()) if torch_arr else (lambda t: t.cpu().numpy())
    if return_dn:
        return conv(s), conv(dn), conv(dm)
    return conv(s)


calc_scores_given_hparams = calc_scores_given_hparams_vectorized  # loop twin, lib/metrics/utils.py:21-45
