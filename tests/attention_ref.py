"""Shared by the attention tests (tests/test_gpu_attention_short.py, tests/test_gpu_attention_long.py on the GPU,
tests/test_attention_bound_host.py on the CPU): the float64 reference of csrc/attention.hip, the switches of the C ABI, the
poisoned-buffer constants, six input families, a per-element error bound derived from the split-fp16 arithmetic, and a plain
torch emulation of that arithmetic into which single faults can be planted.  No tests in here."""
import ctypes

import torch

TAIL = 1024                   # canary words (4 KB) behind every output
OUT_FILL = 0x7FF17FF1         # an fp32 NaN = two fp16 NaNs = two bf16 NaNs
TM = 128

HD = 64
U = 2.0 ** -21                # relative rounding of a split product: three fp16 products, lo.lo dropped
C_BOUND = 2.0


def _lib():
    from lemon_amd import _lib as L
    return L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _arith:
    """with _arith(f16): the attention arithmetic of the calling thread, restored on exit"""

    def __init__(self, f16):
        self.f16 = f16

    def __enter__(self):
        self.prev = _lib().lemon_attention_set_f16(self.f16)

    def __exit__(self, *a):
        _lib().lemon_attention_set_f16(self.prev)


def _reference64(qkv, H, causal):
    B, L, _ = qkv.shape
    q, k, v = qkv.double().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, 64 * H)


def _tiled_index(m, width):
    """[m, width] offsets (in halves) of the hi part of every element of a tile-major activation operand (split3.hpp tiled_off);
    the lo part sits TM * 16 halves further"""
    r = torch.arange(m, device="cuda", dtype=torch.int64)[:, None]
    c = torch.arange(width, device="cuda", dtype=torch.int64)[None, :]
    tile, rr = r // TM, r % TM
    return ((tile * (width >> 4) + (c >> 4)) * 2) * (TM * 16) + (rr >> 5) * 512 + ((c >> 3) & 1) * 256 + (rr & 31) * 8 + (c & 7)


# ---- input families: [B, L, 3, H, 64] float32, packed like the QKV projection's output ------------------------------------------
def _gauss(B, L, H, g):
    return torch.randn(B, L, 3, H, HD, generator=g) * 1.5


def _peaked(B, L, H, g):
    x = _gauss(B, L, H, g)
    x[:, :, :2] = torch.randn(B, L, 2, H, HD, generator=g) * 4.0          # logits: std 4 * 4 * 8 / 8 = 16, a nearly one-hot softmax
    return x


def _flat(B, L, H, g):
    x = _gauss(B, L, H, g)
    x[:, :, 0] = 0.0                                                       # every visible key weighs the same: the running mean of v
    return x


def _offset(B, L, H, g):
    x = _gauss(B, L, H, g)
    u = torch.nn.functional.normalize(torch.randn(H, HD, generator=g), dim=-1)
    x[:, :, :2] = 0.5 * torch.randn(B, L, 2, H, HD, generator=g) + 12.0 * u   # all logits near 144 / 8 = 18, small spread
    return x


def _tail_v(B, L, H, g):
    x = _gauss(B, L, H, g)
    x[:, :, 2] *= torch.exp(torch.rand(B, L, H, 1, generator=g) * 12.0 - 6.0)
    return x


def _onekey(B, L, H, g):
    x = _gauss(B, L, H, g)
    x[:, :, :2] = torch.randn(B, L, 2, H, HD, generator=g) * 0.5
    x[:, L - 1, 1] = 40.0 * x[:, :, 0].mean(dim=1)                         # one dominant key in the last tile: the maximum moves late
    return x


_FAMILIES = {"gauss": _gauss, "peaked": _peaked, "flat": _flat, "offset": _offset, "tail_v": _tail_v, "onekey": _onekey}


def families():
    """name -> make(B, L, H, seed=0) -> qkv [B, L, 3 * H * 64] float32 on the CPU, deterministic"""
    def bind(fn, salt):
        def make(B, L, H, seed=0):
            g = torch.Generator().manual_seed(((seed * 8 + salt) * 4099 + B) * 4099 + L * 7 + H)
            return fn(B, L, H, g).reshape(B, L, 3 * H * HD).contiguous()
        return make
    return {name: bind(fn, i) for i, (name, fn) in enumerate(_FAMILIES.items())}


def _heads(qkv, H, dtype):
    B, L, _ = qkv.shape
    return qkv.to(dtype).view(B, L, 3, H, HD).permute(2, 0, 3, 1, 4)       # q, k, v: [B, H, L, 64]


def _visible(L, causal):
    vis = torch.ones(L, L, dtype=torch.bool)
    return vis.tril() if causal else vis


def bound(qkv, H, causal, C=C_BOUND):
    """-> (ref, bnd), both [B, L, H * 64] float64: the float64 attention and the error a correct kernel may show per element.

    With p the float64 probabilities and U = 2^-21:
        A[i, d] = sum_j p[i, j] |v[j, d]|
        E_s[i]  = max over visible j of (U sum_d |q_id| |k_jd| + 2^-25 sum_d (|q_id| + |k_jd|)) / 8
        bnd     = C (U + E_s[i]) A[i, d] + 2^-24
    E_s is the error of a score: its first term the rounding of the split product (three fp16 products, lo.lo dropped: 2^-21 of
    the products' magnitudes), its second the absolute floor 2^-25 of the unscaled fp16 lo parts of q and k the general kernels
    use.  The softmax turns a score error delta into a relative error delta of p, so (U + E_s) A bounds the product P.V with its
    own split rounding U; 2^-24 is the lo parts' floor on v (sum_j p = 1).  C = 2: a plain fp32 evaluation and the emulation
    below reach at most half of C = 1 on the families above (tests/test_attention_bound_host.py)."""
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float64)
    vis = _visible(L, causal)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, -1)
    ref = (p @ v).transpose(1, 2).reshape(B, L, H * HD)
    A = p @ v.abs()
    e = (U * (q.abs() @ k.abs().transpose(-1, -2)) + 2.0 ** -25 * (q.abs().sum(-1)[..., :, None] + k.abs().sum(-1)[..., None, :])) / 8.0
    E_s = e.masked_fill(~vis, 0.0).amax(dim=-1, keepdim=True)
    bnd = C * (U + E_s) * A + 2.0 ** -24
    return ref, bnd.transpose(1, 2).reshape(B, L, H * HD)


def evaluate_f32(qkv, H, causal):
    """the formula of _reference64 in plain fp32 PyTorch"""
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float32)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~_visible(L, causal), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, H * HD).double()


def _split_u(x):
    """fp32 -> fp16 hi and unscaled fp16 lo (attention.hip: split8u), both returned as float64"""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


FAULTS = ("drop_qlo", "drop_plo", "padkey", "strict")


def emulate_split(qkv, H, causal, fault=None):
    """The arithmetic of the general split-fp16 kernels on the CPU: q, k, v and the probabilities as fp16 hi / unscaled lo pairs,
    lo.lo dropped, the softmax in fp32 with the probabilities carried at 2^10, every sum exact (float64).  -> [B, L, H * 64] float64.

    fault: None, or one planted defect --
      drop_qlo   no q_lo . k_hi product
      drop_plo   no p_lo . v_hi product
      padkey     one zero K / V row at index L (the padding of the last tile) left unmasked for every query
      strict     causal mask j < i instead of j <= i (query 0 keeps key 0)"""
    assert fault is None or fault in FAULTS, fault
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float32)
    vis = _visible(L, causal)
    if fault == "strict" and causal:
        vis = vis.tril(-1)
        vis[0, 0] = True
    if fault == "padkey":
        k = torch.cat([k, torch.zeros(B, H, 1, HD)], dim=2)
        v = torch.cat([v, torch.zeros(B, H, 1, HD)], dim=2)
        vis = torch.cat([vis, torch.ones(L, 1, dtype=torch.bool)], dim=1)
    qh, ql = _split_u(q)
    kh, kl = _split_u(k)
    vh, vl = _split_u(v)
    s = qh @ kh.transpose(-1, -2) + qh @ kl.transpose(-1, -2)
    if fault != "drop_qlo":
        s = s + ql @ kh.transpose(-1, -2)
    s = s.float().masked_fill(~vis, float("-inf"))
    c_exp = 0.125 * 1.44269504088896340736
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp2((s - m) * c_exp + 10.0)                                  # fp32
    ph, pl = _split_u(p)
    o = ph @ vh + ph @ vl
    if fault != "drop_plo":
        o = o + pl @ vh
    o = o / p.double().sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, L, H * HD)
