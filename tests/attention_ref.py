"""Shared by the attention tests (tests/test_gpu_attention_short.py, tests/test_gpu_attention_long.py,
tests/test_gpu_attention_stream_edges.py on the GPU, tests/test_attention_bound_host.py, tests/test_attention_stream_host.py on the
CPU): the float64 reference of csrc/attention.hip and csrc/attention_hd.hip, the switches of the C ABI, the poisoned-buffer
constants, six input families and three more built for the online softmax of the streaming kernels, a per-element error bound
derived from the split-fp16 arithmetic, a plain torch emulation of that arithmetic and one of the streaming kernels' running
maximum / sum / rescale, into both of which single faults can be planted.  The head dimension is a parameter (64 by default).
No tests in here."""
import ctypes
import math

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


def _reference64(qkv, H, causal, hd=HD):
    B, L, _ = qkv.shape
    q, k, v = qkv.double().view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, hd * H)


def _tiled_index(m, width):
    """[m, width] offsets (in halves) of the hi part of every element of a tile-major activation operand (split3.hpp tiled_off);
    the lo part sits TM * 16 halves further"""
    r = torch.arange(m, device="cuda", dtype=torch.int64)[:, None]
    c = torch.arange(width, device="cuda", dtype=torch.int64)[None, :]
    tile, rr = r // TM, r % TM
    return ((tile * (width >> 4) + (c >> 4)) * 2) * (TM * 16) + (rr >> 5) * 512 + ((c >> 3) & 1) * 256 + (rr & 31) * 8 + (c & 7)


# ---- input families: [B, L, 3, H, hd] float32, packed like the QKV projection's output ------------------------------------------
def _gauss(B, L, H, g, hd=HD):
    return torch.randn(B, L, 3, H, hd, generator=g) * 1.5


def _peaked(B, L, H, g, hd=HD):
    x = _gauss(B, L, H, g, hd)
    x[:, :, :2] = torch.randn(B, L, 2, H, hd, generator=g) * 4.0          # logits: std 4 * 4 * sqrt(hd) / sqrt(hd) = 16, a nearly one-hot softmax
    return x


def _flat(B, L, H, g, hd=HD):
    x = _gauss(B, L, H, g, hd)
    x[:, :, 0] = 0.0                                                       # every visible key weighs the same: the running mean of v
    return x


def _offset(B, L, H, g, hd=HD):
    x = _gauss(B, L, H, g, hd)
    u = torch.nn.functional.normalize(torch.randn(H, hd, generator=g), dim=-1)
    x[:, :, :2] = 0.5 * torch.randn(B, L, 2, H, hd, generator=g) + 12.0 * u   # all logits near 144 / sqrt(hd) (18 at 64), small spread
    return x


def _tail_v(B, L, H, g, hd=HD):
    x = _gauss(B, L, H, g, hd)
    x[:, :, 2] *= torch.exp(torch.rand(B, L, H, 1, generator=g) * 12.0 - 6.0)
    return x


def _onekey(B, L, H, g, hd=HD):
    x = _gauss(B, L, H, g, hd)
    x[:, :, :2] = torch.randn(B, L, 2, H, hd, generator=g) * 0.5
    x[:, L - 1, 1] = 40.0 * x[:, :, 0].mean(dim=1)                         # one dominant key in the last tile: the maximum moves late
    return x


# three more for the online softmax of the streaming kernels (running maximum m, running sum l, alpha = exp(m_old - m_new))
def _ascending(B, L, H, g, hd=HD):
    # the logit of key j is about 0.25 j for every query: the running maximum moves in every key tile, alpha < 1 everywhere
    # (the keys' noise has no component along u: it would shift a key for all queries alike, and a last tile of one key could
    # then stay below the maximum for a whole wave)
    x = _gauss(B, L, H, g, hd)
    u = torch.nn.functional.normalize(torch.randn(H, hd, generator=g), dim=-1)
    x[:, :, 0] = math.sqrt(hd) * u + 0.3 * torch.randn(B, L, H, hd, generator=g)
    j = torch.arange(L, dtype=torch.float32)[None, :, None, None]
    n = 0.3 * torch.randn(B, L, H, hd, generator=g)
    x[:, :, 1] = 0.25 * j * u + (n - (n * u).sum(-1, keepdim=True) * u)
    return x


def _firstkey(B, L, H, g, hd=HD):
    # onekey with the dominant key at index 0: after the first key tile the running maximum never moves, alpha == 1 for every
    # row of every later tile.  (onekey's 40 mean(q) is the largest logit of most rows, not of all of them, at several hundred
    # tokens: here every query carries 3 u and key 0 is 5 sqrt(hd) u, its logit 15 +- 2.5 for every query, the others' std 0.3)
    x = _gauss(B, L, H, g, hd)
    u = torch.nn.functional.normalize(torch.randn(H, hd, generator=g), dim=-1)
    x[:, :, :2] = torch.randn(B, L, 2, H, hd, generator=g) * 0.5
    x[:, :, 0] += 3.0 * u
    x[:, 0, 1] = 5.0 * math.sqrt(hd) * u
    return x


def _onerow(B, L, H, g, hd=HD):
    # dominant keys 30 e0 at index 37 and at L - 1; the queries at rows 5 mod 32 are 6 e0 (logit 180 / sqrt(hd) there), every
    # other query has no e0 component: in the tiles of the dominant keys the maximum moves for ONE row of a wave's 32 and the
    # others' alpha is what the 0.5-gaussian logits make it, 1 for many of them (causal too: row 37 = 5 mod 32 sees key 37)
    x = _gauss(B, L, H, g, hd)
    x[:, :, :2] = torch.randn(B, L, 2, H, hd, generator=g) * 0.5
    x[:, :, 0, :, 0] = 0.0
    x[:, 5::32, 0] = 0.0
    x[:, 5::32, 0, :, 0] = 6.0
    for j in ((37, L - 1) if L > 37 else (L - 1,)):
        x[:, j, 1] = 0.0
        x[:, j, 1, :, 0] = 30.0
    return x


_FAMILIES = {"gauss": _gauss, "peaked": _peaked, "flat": _flat, "offset": _offset, "tail_v": _tail_v, "onekey": _onekey}
_STREAM_FAMILIES = dict(_FAMILIES, ascending=_ascending, firstkey=_firstkey, onerow=_onerow)


def families():
    """name -> make(B, L, H, seed=0) -> qkv [B, L, 3 * H * 64] float32 on the CPU, deterministic"""
    def bind(fn, salt):
        def make(B, L, H, seed=0):
            g = torch.Generator().manual_seed(((seed * 8 + salt) * 4099 + B) * 4099 + L * 7 + H)
            return fn(B, L, H, g).reshape(B, L, 3 * H * HD).contiguous()
        return make
    return {name: bind(fn, i) for i, (name, fn) in enumerate(_FAMILIES.items())}


def stream_families(hd=HD):
    """name -> make(B, L, H, seed=0) -> qkv [B, L, 3 * H * hd] float32 on the CPU, deterministic: the six families above at head
    dim hd (other tensors than families() makes: salts of their own) and ascending, firstkey, onerow"""
    def bind(fn, salt):
        def make(B, L, H, seed=0):
            g = torch.Generator().manual_seed((((seed * 16 + salt) * 4099 + B) * 4099 + L * 7 + H) * 257 + hd + (1 << 40))
            return fn(B, L, H, g, hd).reshape(B, L, 3 * H * hd).contiguous()
        return make
    return {name: bind(fn, i) for i, (name, fn) in enumerate(_STREAM_FAMILIES.items())}


def _heads(qkv, H, dtype, hd=HD):
    B, L, _ = qkv.shape
    return qkv.to(dtype).view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)       # q, k, v: [B, H, L, hd]


def _visible(L, causal):
    vis = torch.ones(L, L, dtype=torch.bool)
    return vis.tril() if causal else vis


def bound(qkv, H, causal, C=C_BOUND, hd=HD):
    """-> (ref, bnd), both [B, L, H * hd] float64: the float64 attention and the error a correct kernel may show per element.

    With p the float64 probabilities and U = 2^-21:
        A[i, d] = sum_j p[i, j] |v[j, d]|
        E_s[i]  = max over visible j of (U sum_d |q_id| |k_jd| + 2^-25 sum_d (|q_id| + |k_jd|)) / sqrt(hd)
        bnd     = C (U + E_s[i]) A[i, d] + 2^-24
    E_s is the error of a score: its first term the rounding of the split product (three fp16 products, lo.lo dropped: 2^-21 of
    the products' magnitudes), its second the absolute floor 2^-25 of the unscaled fp16 lo parts of q and k the general kernels
    use.  The softmax turns a score error delta into a relative error delta of p, so (U + E_s) A bounds the product P.V with its
    own split rounding U; 2^-24 is the lo parts' floor on v (sum_j p = 1).  C = 2: a plain fp32 evaluation and the emulations
    below reach at most half of C = 1 on the families above (tests/test_attention_bound_host.py,
    tests/test_attention_stream_host.py)."""
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float64, hd)
    vis = _visible(L, causal)
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, -1)
    ref = (p @ v).transpose(1, 2).reshape(B, L, H * hd)
    A = p @ v.abs()
    e = (U * (q.abs() @ k.abs().transpose(-1, -2)) + 2.0 ** -25 * (q.abs().sum(-1)[..., :, None] + k.abs().sum(-1)[..., None, :])) / math.sqrt(hd)
    E_s = e.masked_fill(~vis, 0.0).amax(dim=-1, keepdim=True)
    bnd = C * (U + E_s) * A + 2.0 ** -24
    return ref, bnd.transpose(1, 2).reshape(B, L, H * hd)


def evaluate_f32(qkv, H, causal, hd=HD):
    """the formula of _reference64 in plain fp32 PyTorch"""
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float32, hd)
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~_visible(L, causal), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, H * hd).double()


def _split_u(x):
    """fp32 -> fp16 hi and unscaled fp16 lo (attention.hip: split8u), both returned as float64"""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


FAULTS = ("drop_qlo", "drop_plo", "padkey", "strict")


def emulate_split(qkv, H, causal, fault=None, hd=HD):
    """The arithmetic of the general split-fp16 kernels on the CPU: q, k, v and the probabilities as fp16 hi / unscaled lo pairs,
    lo.lo dropped, the softmax in fp32 with the probabilities carried at 2^10, every sum exact (float64).  -> [B, L, H * hd] float64.

    fault: None, or one planted defect --
      drop_qlo   no q_lo . k_hi product
      drop_plo   no p_lo . v_hi product
      padkey     one zero K / V row at index L (the padding of the last tile) left unmasked for every query
      strict     causal mask j < i instead of j <= i (query 0 keeps key 0)"""
    assert fault is None or fault in FAULTS, fault
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float32, hd)
    vis = _visible(L, causal)
    if fault == "strict" and causal:
        vis = vis.tril(-1)
        vis[0, 0] = True
    if fault == "padkey":
        k = torch.cat([k, torch.zeros(B, H, 1, hd)], dim=2)
        v = torch.cat([v, torch.zeros(B, H, 1, hd)], dim=2)
        vis = torch.cat([vis, torch.ones(L, 1, dtype=torch.bool)], dim=1)
    qh, ql = _split_u(q)
    kh, kl = _split_u(k)
    vh, vl = _split_u(v)
    s = qh @ kh.transpose(-1, -2) + qh @ kl.transpose(-1, -2)
    if fault != "drop_qlo":
        s = s + ql @ kh.transpose(-1, -2)
    s = s.float().masked_fill(~vis, float("-inf"))
    c_exp = (1.0 / math.sqrt(hd)) * 1.44269504088896340736
    m = s.amax(dim=-1, keepdim=True)
    p = torch.exp2((s - m) * c_exp + 10.0)                                  # fp32
    ph, pl = _split_u(p)
    o = ph @ vh + ph @ vl
    if fault != "drop_plo":
        o = o + pl @ vh
    o = o / p.double().sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, L, H * hd)


STREAM_FAULTS = ("no_rescale", "any_skip", "stale_l", "early_stop")


def stream_deal(TJ, wmax):
    """the even deal of TJ query tiles to workgroups of at most wmax waves (attention_plan.hpp deal_tiles, stream_tiles of the
    kernels) -> [(tile0, ntiles)] per workgroup"""
    nqb = (TJ + wmax - 1) // wmax
    return [(qb * TJ // nqb, (qb + 1) * TJ // nqb - qb * TJ // nqb) for qb in range(nqb)]


def emulate_stream(qkv, H, causal, hd=HD, wmax=4, tb=2, fault=None, trace=None):
    """The online softmax of the streaming kernels (k_attention_hd64_stream, k_attention_hd64_stream_f16, k_attention_hdx_stream) on
    the CPU, in fp32: query tiles of 32 rows dealt to workgroups of at most wmax waves, the keys in blocks of tb tiles of 32; per
    key tile, in the kernels' order, the scores, the masks, the tile maximum, m_new, alpha = exp2((m_run - m_new) c), the
    probabilities exp2((s - m_new) c), l_run = l_run alpha + sum p, the accumulator times alpha unless alpha == 1 for all rows of
    the query tile, the accumulator + P.V; 1 / l_run at the end.  (fp32 products with PyTorch's summation order, not the matrix
    cores': an emulation of the algorithm, not of the bits.)  -> [B, L, H * hd] float64.

    trace: None, or a list that receives (query tile, key tile, alpha == 1 as a bool tensor [B, H, rows]) per step.
    fault: None, or one planted defect --
      no_rescale  the accumulator is never multiplied by alpha
      any_skip    the rescale of a query tile is skipped when ANY of its rows has alpha == 1 (__any for __all)
      stale_l     the running sum is not multiplied by alpha
      early_stop  causal only: the workgroup's last key tile is tile0 + ntiles - 1 (kt_end one short), so its last wave never
                  sees its diagonal tile (a kernel would read stale LDS there; the emulation leaves the tile out)"""
    assert fault is None or fault in STREAM_FAULTS, fault
    B, L, _ = qkv.shape
    q, k, v = _heads(qkv, H, torch.float32, hd)
    TJ = (L + 31) // 32
    c_exp = torch.tensor((1.0 / math.sqrt(hd)) * 1.44269504088896340736, dtype=torch.float32)
    out = torch.empty(B, H, L, hd, dtype=torch.float32)
    for tile0, ntiles in stream_deal(TJ, wmax):
        kt_end = min(tile0 + ntiles, TJ) if causal else TJ
        if fault == "early_stop" and causal:
            kt_end = tile0 + ntiles - 1
        for wave in range(ntiles):
            gt = tile0 + wave
            r0, r1 = 32 * gt, min(32 * gt + 32, L)
            qt = q[:, :, r0:r1]
            qi = torch.arange(r0, r1)[:, None]
            o = torch.zeros(B, H, r1 - r0, hd, dtype=torch.float32)
            m_run = torch.full((B, H, r1 - r0, 1), float("-inf"), dtype=torch.float32)
            l_run = torch.zeros(B, H, r1 - r0, 1, dtype=torch.float32)
            tj_end = min(gt + 1, TJ) if causal else TJ
            for kb in range((kt_end + tb - 1) // tb):
                staged = min(kt_end - kb * tb, tb)                          # nrows / 32: tiles of this block that are in LDS
                for tj in range(kb * tb, min((kb + 1) * tb, tj_end, kb * tb + staged)):
                    j0, j1 = 32 * tj, min(32 * tj + 32, L)
                    s = qt @ k[:, :, j0:j1].transpose(-1, -2)
                    if causal and tj == gt:
                        s = s.masked_fill(torch.arange(j0, j1)[None, :] > qi, float("-inf"))
                    m_new = torch.maximum(m_run, s.amax(dim=-1, keepdim=True))
                    alpha = torch.exp2((m_run - m_new) * c_exp)
                    p = torch.exp2((s - m_new) * c_exp)
                    l_run = (l_run if fault == "stale_l" else l_run * alpha) + p.sum(-1, keepdim=True)
                    m_run = m_new
                    one = alpha == 1.0
                    if trace is not None:
                        trace.append((gt, tj, one[..., 0].clone()))
                    skip = one.any(dim=2, keepdim=True) if fault == "any_skip" else one.all(dim=2, keepdim=True)
                    if fault != "no_rescale":
                        o = torch.where(skip, o, o * alpha)
                    o = o + p @ v[:, :, j0:j1]
            out[:, :, r0:r1] = o * (1.0 / l_run)
    return out.transpose(1, 2).reshape(B, L, H * hd).double()
