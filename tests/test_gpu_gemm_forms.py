"""GPU: every launch form of the hand-written split-fp16 GEMM (csrc/gemm_f16x3.hip) and the LayerNorm operand producers in front
of it, called through the C ABI with buffers this file allocates itself, against float64.

Poisoning: every output buffer is filled with a NaN bit pattern (one fp32 NaN = two fp16 NaNs) and followed by a 4 KB canary tail
before the call.  Every element the call owes must come out finite and within a PER-ELEMENT error bound; every tail word must
keep its value bit for bit.  Rows m .. ceil(m / 128) 128 of a tile-major operand output are unspecified and not checked.  The
padding rows of tile-major INPUT operands hold fp16 NaN / Inf (what torch.empty hands the product path): they must not reach
a stored row.

Error bound of the split GEMM, per element: C 2^-21 (|alpha| (|A| @ |W|^T) + |bias| + |residual|) (the three fp16 products drop
lo.lo and round the lo parts, 2^-22 each, plus fp32 accumulation), widened for operand outputs by the activation's and the
fp16 split's rounding of the stored value.  Dropping one hi.lo product costs ~2^-12 |A| |W| per term: far outside it."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Calibrated on an MI355X: the worst error seen over the 104 GEMM cases below is 0.75 x 2^-21 S (form 2, m = 129, n = 1792,
# k = 768; every form stays below 0.75); C = 2 leaves that a factor of 2.7, while a dropped hi.lo product (~2^-12.5 sqrt(k) of
# the operands' scale per element against C 2^-21 0.64 k) lands 5 x beyond it at k = 3072 and 50 x at k = 32.
C = 2.0
# the LayerNorm producers (fp32 row statistics: the bracket is the row's, see _ln_bound): worst seen on an MI355X 0.34 x 2^-21
# (width 768, 7 rows), for the row statistics of lemon_rowstats_f16x3t / lemon_ln_finalize as well
C_LN = 4.0
U = 2.0 ** -21
TAIL = 1024                   # canary words (4 KB) behind every output
OUT_FILL = 0x7FF17FF1         # output poison: an fp32 NaN, and two fp16 NaNs
PAD_FILL = 0x7C00FE00         # padding rows of input operands: fp16 NaN (low half), +Inf (high half)
TM = 128                      # rows of an activation tile (split3.hpp TILE_A_ROWS)
FOLD_MAX_SHIFT = 8.0          # common.hpp LEMON_LN_FOLD_MAX_SHIFT
EPS = 1e-5

# The 13 instantiations the dispatcher launches (select_form and FACTS of csrc/gemm_f16x3_plan.hpp) and the ABI arguments that reach
# each: `abi` plain = lemon_linear_f16x3t, ln = lemon_linear_f16x3t_ln, chain = lemon_linear_f16x3t_chain; `fold` passes
# row_aff + colsum; `emit` passes emit_t + emit_stats; `out` whether out_dev is non-null; `res_t` the residual as a tile-major
# operand; `mfma` the matrix shape the plain forms are pinned to (lemon_linear_f16x3t_set_mfma: the 32x32 forms are reached
# with 32, and with 16 whenever k / 16 is odd).
FORMS = {
    1: dict(kernel="k_gemm_f16x3t16<2, true, false>", abi="ln", act="gelu", fold=True),
    2: dict(kernel="k_gemm_f16x3t16<1, true, false>", abi="ln", act="silu", fold=True),
    3: dict(kernel="k_gemm_f16x3t16<0, true, false>", abi="ln", act=None, fold=True),
    4: dict(kernel="k_gemm_f16x3t16<0, false, true>", abi="ln", act=None, emit=True, out=True),
    5: dict(kernel="k_gemm_f16x3t16<0, false, true, 1>", abi="chain", act=None, emit=True, out=False),
    6: dict(kernel="k_gemm_f16x3t16<0, false, true, 2>", abi="chain", act=None, emit=True, out=True, res_t=True),
    7: dict(kernel="k_gemm_f16x3t16<0, false, true, 3>", abi="chain", act=None, emit=True, out=False, res_t=True),
    8: dict(kernel="k_gemm_f16x3t16<2, false, false>", abi="plain", act="gelu", mfma=16),
    9: dict(kernel="k_gemm_f16x3t16<1, false, false>", abi="plain", act="silu", mfma=16),
    10: dict(kernel="k_gemm_f16x3t16<0, false, false>", abi="plain", act=None, mfma=16),
    11: dict(kernel="k_gemm_f16x3t<2>", abi="plain", act="gelu", mfma=32),
    12: dict(kernel="k_gemm_f16x3t<1>", abi="plain", act="silu", mfma=32),
    13: dict(kernel="k_gemm_f16x3t<0>", abi="plain", act=None, mfma=32),
}

# Shapes.  n-tile counts 1, 2, 3, 4, 5, 7, 9, 12: every super-block width gn of the tile walk (4, 3, 2, 1) and every case where
# gn does not divide the tile count.  m = 1, 127, 128, 129 and a large m of 33 m-tiles = gm j + 1 for every gm (32, 16, 8): one
# super-block row holds a single m-tile, and the super-block count (2, 3, 5, 3, 10, 14, 15, 9 over the n above) is never a
# multiple of the 8 XCDs the grid is padded to; at n = 1024 the large m is 18 557 (145 m-tiles, ten super-blocks).  k: 16 and
# 48 (one / three k16 steps: 32x32 kernel only), 32, 768, 3072.  Each form walks all eight n with m, k, bias and residual
# rotated by the form number, so that every form sees every m, every k it accepts and every bias / residual combination.
N_ALL = (256, 512, 768, 1024, 1280, 1792, 2304, 3072)
M_CYCLE = (1, 127, "big", 128, 129, 127, 1, 129)
K_EVEN = (32, 768, 3072)
K_32X32 = (16, 48, 32, 768, 3072)


def _cases(form):
    spec = FORMS[form]
    ks = K_32X32 if spec.get("mfma") == 32 else K_EVEN
    out = []
    for i, n in enumerate(N_ALL):
        j = i + form
        m = M_CYCLE[j % 8]
        if m == "big":
            m = 18557 if n == 1024 else 4100
        res = bool((j // 2) % 2) and spec["act"] is None
        if spec.get("res_t"):
            res = True
        out.append((form, m, n, ks[j % len(ks)], bool(j % 2), res))
    return out


CASES = [c for f in FORMS for c in _cases(f)]


def _lib():
    from lemon_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check(rc, what):
    _lib().check(rc, what)


def _words(n, fill):
    """n int32 words + the canary tail, every word = fill"""
    return torch.full((n + TAIL,), fill, dtype=torch.int32, device="cuda")


def _tail_intact(buf, n, fill=OUT_FILL):
    return bool((buf[n:] == fill).all())


def _rows_t(m):
    return (m + TM - 1) // TM * TM


def _tiled_index(m, width):
    """[m, width] offsets (in halves) of the hi part of every element of a tile-major activation operand (split3.hpp
    tiled_off); the lo 2^11 part sits TM * 16 halves further"""
    r = torch.arange(m, device="cuda", dtype=torch.int64)[:, None]
    c = torch.arange(width, device="cuda", dtype=torch.int64)[None, :]
    tile, rr = r // TM, r % TM
    return ((tile * (width >> 4) + (c >> 4)) * 2) * (TM * 16) + (rr >> 5) * 512 + ((c >> 3) & 1) * 256 + (rr & 31) * 8 + (c & 7)


def _split(x):
    """fp32 -> (hi, lo 2^11) fp16 as split3.hpp split2h<false> makes them (exact in torch: both conversions round to nearest)"""
    hi = x.half()
    return hi, ((x - hi.float()) * 2048.0).half()


def _pack_act(x, fill=PAD_FILL):
    """fp32 [m, k] -> the tile-major activation operand, padding rows left at `fill`; returns the int32 word buffer"""
    m, k = x.shape
    nw = _rows_t(m) * k
    buf = _words(nw, fill)
    h = buf[:nw].view(torch.float16)
    idx = _tiled_index(m, k).reshape(-1)
    hi, lo = _split(x)
    h[idx] = hi.reshape(-1)
    h[idx + TM * 16] = lo.reshape(-1)
    return buf


def _unpack(buf, m, width):
    """(hi, lo 2^11) fp16 [m, width] of rows < m of a tile-major operand held in an int32 word buffer"""
    h = buf[:_rows_t(m) * width].view(torch.float16)
    idx = _tiled_index(m, width)
    return h[idx], h[idx + TM * 16]


def _value(hi, lo):
    return hi.double() + lo.double() * (1.0 / 2048.0)


def _pack_weight(w):
    n, k = w.shape
    from lemon_amd import ops
    ws = ops.weight_scale_f16x3(w)
    wt = torch.empty((n * k * 2,), dtype=torch.float16, device="cuda")
    _check(_lib().load().lemon_pack_weight_f16x3t(_p(w), n, k, float(ws), _p(wt), _stream()), "lemon_pack_weight_f16x3t")
    return wt, ws


def _std_rows(g, m, k):
    """[m, k] float64 rows of zero mean and unit spread (population), so that a row's |mean| / sigma is what the caller sets"""
    z = torch.randn(m, k, generator=g, device="cuda", dtype=torch.float64)
    z = z - z.mean(1, keepdim=True)
    return z / z.pow(2).mean(1, keepdim=True).sqrt().clamp_min(1e-30)


def _act64(u, act):
    if act == "gelu":
        return 0.5 * u * (1.0 + torch.erf(u / 2.0 ** 0.5))
    if act == "silu":
        return u * torch.sigmoid(u)
    return u


def _row_aff(x64):
    """float64 (rstd, -mean rstd) of every row as fp32, NaN beyond the fold's bound (what lemon_rowstats_f16x3t promises)"""
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    aff = torch.stack([rstd, -mean * rstd], 1).float()
    far = mean.abs() * rstd > FOLD_MAX_SHIFT
    aff[far] = float("nan")
    return aff.contiguous(), mean, rstd, far


def _inputs(form, m, n, k, bias, res, seed):
    """deterministic operands of one case (CUDA generator: the same values in a child process on the same device)"""
    spec = FORMS[form]
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 0.5 + 2.0 * torch.rand(m, 1, generator=g, device="cuda", dtype=torch.float64)
    if spec.get("fold"):
        shift = 6.0 * torch.rand(m, 1, generator=g, device="cuda", dtype=torch.float64) - 3.0
        x = (_std_rows(g, m, k) + shift) * scale
        if m > 4:
            x[1] = (_std_rows(g, 1, k)[0] + 20.0) * 0.7          # |mean| / sigma = 20: row_aff NaN, its row non-finite
            x[2] = 0.0                                           # constant rows: LayerNorm gives beta
            x[3] = 0.01                                          # (|mean| rstd = 3.2 with eps 1e-5: folded)
    else:
        x = torch.randn(m, k, generator=g, device="cuda", dtype=torch.float64) * scale
    x = x.float().contiguous()
    w = (torch.randn(n, k, generator=g, device="cuda") / k ** 0.5).contiguous()
    b = (0.1 * torch.randn(n, generator=g, device="cuda")).contiguous() if bias else None
    r = None
    if res:
        r = (torch.randn(m, n, generator=g, device="cuda", dtype=torch.float64) * scale
             + 3.0 * torch.randn(m, 1, generator=g, device="cuda", dtype=torch.float64)).float().contiguous()
    alpha = 0.75
    fold = None
    if spec.get("fold"):
        gamma = (1.0 + 0.3 * torch.randn(k, generator=g, device="cuda")).contiguous()
        beta = (0.2 * torch.randn(k, generator=g, device="cuda")).contiguous() if bias else torch.zeros(k, device="cuda")
        fold = dict(gamma=gamma, beta=beta)
    return dict(x=x, w=w, b=b, r=r, alpha=alpha, fold=fold)


def _launch(form, m, n, k, inp):
    """one call of the form's ABI on poisoned outputs: {name: (word buffer, words owed)}"""
    from lemon_amd import ops
    spec = FORMS[form]
    lib = _lib().load()
    x, w, b, r, alpha = inp["x"], inp["w"], inp["b"], inp["r"], inp["alpha"]
    at = _pack_act(x)
    act = ops._ACT_CODE[spec["act"]]
    operand_out = spec["act"] is not None
    outs = {}
    if operand_out:
        outs["op"] = (_words(_rows_t(m) * n, OUT_FILL), _rows_t(m) * n)
    elif spec.get("out", True):
        outs["out"] = (_words(m * n, OUT_FILL), m * n)
    if spec.get("emit"):
        outs["emit"] = (_words(_rows_t(m) * n, OUT_FILL), _rows_t(m) * n)
        outs["stats"] = (_words(m * (n // 128) * 2, OUT_FILL), m * (n // 128) * 2)
    out_buf = outs["op"][0] if operand_out else (outs["out"][0] if "out" in outs else None)
    emit_t = outs["emit"][0] if "emit" in outs else None
    stats = outs["stats"][0] if "stats" in outs else None
    keep = [at]
    if spec.get("fold"):
        f = inp["fold"]
        wt, a, colsum, bp = ops.fold_layernorm_weight(w, b, f["gamma"], f["beta"], alpha)
        aff = _row_aff(x.double())[0]
        bp = bp if b is not None else None
        keep += [wt, colsum, aff, bp]
        # (fold_layernorm_weight scales colsum and the bias by `extra` = alpha, the caller multiplies its 1 / wscale by it)
        _check(lib.lemon_linear_f16x3t_ln(_p(at), _p(wt), _p(bp), _p(r), m, n, k, float(alpha * a), act, int(operand_out),
                                          _p(out_buf), _p(aff), _p(colsum), None, None, _stream()), "lemon_linear_f16x3t_ln")
    else:
        wt, ws = _pack_weight(w)
        keep.append(wt)
        a = alpha / ws
        if spec["abi"] == "plain":
            prev = lib.lemon_linear_f16x3t_set_mfma(16 if (k // 16) % 2 else spec["mfma"])
            assert prev >= 0
            try:
                _check(lib.lemon_linear_f16x3t(_p(at), _p(wt), _p(b), _p(r), m, n, k, float(a), act, int(operand_out), _p(out_buf),
                                               _stream()), "lemon_linear_f16x3t")
            finally:
                lib.lemon_linear_f16x3t_set_mfma(prev)
        elif spec["abi"] == "ln":
            _check(lib.lemon_linear_f16x3t_ln(_p(at), _p(wt), _p(b), _p(r), m, n, k, float(a), act, 0, _p(out_buf), None, None,
                                              _p(emit_t), _p(stats), _stream()), "lemon_linear_f16x3t_ln")
        else:
            rt = _pack_act(r) if spec.get("res_t") else None
            keep.append(rt)
            _check(lib.lemon_linear_f16x3t_chain(_p(at), _p(wt), _p(b), None if rt is not None else _p(r), _p(rt), m, n, k, float(a),
                                                 _p(out_buf), _p(emit_t), _p(stats), _stream()), "lemon_linear_f16x3t_chain")
    torch.cuda.synchronize()
    del keep
    return outs


def _reference(form, m, n, k, inp):
    """float64 (pre-activation u, bracket S of the error bound, rows whose fold row_aff is NaN)"""
    spec = FORMS[form]
    x, w = inp["x"].double(), inp["w"].double()
    alpha = inp["alpha"]
    b = inp["b"].double() if inp["b"] is not None else torch.zeros(n, device="cuda", dtype=torch.float64)
    r = inp["r"].double() if inp["r"] is not None else torch.zeros(m, n, device="cuda", dtype=torch.float64)
    far = torch.zeros(m, dtype=torch.bool, device="cuda")
    if spec.get("fold"):
        gamma, beta = inp["fold"]["gamma"].double(), inp["fold"]["beta"].double()
        ln = torch.nn.functional.layer_norm(x, (k,), gamma, beta, EPS)
        u = alpha * (ln @ w.T + b) + r
        # the folded operand carries x, not LN(x): the products' rounding scales with rstd |x| and the mean correction
        _, mean, rstd, far = _row_aff(x)
        wp = (w * gamma[None, :]).abs()
        S = abs(alpha) * (rstd[:, None] * (x.abs() @ wp.T) + (rstd * mean.abs())[:, None] * wp.sum(1)[None, :]
                          + (b + w @ beta).abs()[None, :]) + r.abs()
    else:
        u = alpha * (x @ w.T) + b + r
        S = abs(alpha) * (x.abs() @ w.abs().T) + b.abs()[None, :] + r.abs()
    return u, S, far


def _assert_close(got, ref, S, rows, what, c=C):
    """every element of the rows `rows` finite and within c 2^-21 S; returns the worst |err| / (2^-21 S)"""
    g, rf, s = got[rows], ref[rows], S[rows]
    bad = ~torch.isfinite(g)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} non-finite values, first at {bad.nonzero()[0].tolist()}"
    ratio = (g - rf).abs() / (U * s).clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > c:
        i = int(ratio.argmax())
        pos = divmod(i, ratio.shape[1])
        raise AssertionError(f"{what}: err {float((g - rf).abs().reshape(-1)[i]):.3e} = {worst:.2f} x 2^-21 S at (row, col) {pos} "
                             f"(bound {c} x); {int((ratio > c).sum())} elements beyond")
    return worst


def _group_stats(y, n):
    """float64 per row and 128-column group (mean, M2)"""
    yg = y.reshape(y.shape[0], n // 128, 128)
    mean = yg.mean(2)
    return mean, (yg - mean[..., None]).pow(2).sum(2), yg


@pytest.mark.parametrize("form,m,n,k,bias,res", CASES,
                         ids=[f"f{c[0]}-m{c[1]}-n{c[2]}-k{c[3]}-{'b' if c[4] else 'nob'}-{'r' if c[5] else 'nor'}" for c in CASES])
def test_gemm_form_against_float64(hip, form, m, n, k, bias, res):
    spec = FORMS[form]
    inp = _inputs(form, m, n, k, bias, res, seed=1000 * form + 7 * m + n + k)
    outs = _launch(form, m, n, k, inp)
    assert _lib().load().lemon_linear_f16x3t_last_kernel().decode("ascii") == spec["kernel"]      # the form ran the kernel it names
    for name, (buf, nw) in outs.items():
        assert _tail_intact(buf, nw), f"form {form} {spec['kernel']}: write past the end of `{name}`"
    u, S, far = _reference(form, m, n, k, inp)
    near = ~far
    tag = f"form {form} {spec['kernel']} m={m} n={n} k={k}"
    worst = 0.0
    if "op" in outs:
        v = _act64(u, spec["act"])
        hi, lo = _unpack(outs["op"][0], m, n)
        got = _value(hi, lo)
        # the activation's rounding (a few ulp of u) and the fp16 split of the stored value (2^-22) ride on top; |act'| <= 1.2
        worst = _assert_close(got, v, 1.2 * S + u.abs() + v.abs(), near, tag + " operand")
        if bool(far.any()):
            assert not bool(torch.isfinite(hi[far]).any()), tag + ": rows beyond the fold's bound must come out non-finite"
    if "out" in outs:
        got = outs["out"][0][:m * n].view(torch.float32).view(m, n)
        worst = max(worst, _assert_close(got.double(), u, S, near, tag + " fp32 out"))
        if bool(far.any()):
            assert not bool(torch.isfinite(got[far]).any()), tag + ": rows beyond the fold's bound must come out non-finite"
    if "emit" in outs:
        hi, lo = _unpack(outs["emit"][0], m, n)
        if "out" in outs:
            # the emitted operand is the fp16 split of exactly the stored fp32 values
            ehi, elo = _split(outs["out"][0][:m * n].view(torch.float32).view(m, n))
            assert torch.equal(hi.view(torch.int16), ehi.view(torch.int16)) and torch.equal(lo.view(torch.int16), elo.view(torch.int16)), \
                tag + ": emitted operand is not the split of the fp32 result"
        worst = max(worst, _assert_close(_value(hi, lo), u, S + u.abs(), near, tag + " emitted operand"))
        st = outs["stats"][0][:m * (n // 128) * 2].view(torch.float32).view(m, n // 128, 2).double()
        mean_r, m2_r, yg = _group_stats(u, n)
        eg = (C * U * S).reshape(m, n // 128, 128).amax(2)                # the group's largest admissible output error
        dev = (yg - mean_r[..., None]).abs().amax(2)
        tol_mean = eg + C * U * yg.abs().amax(2)
        tol_m2 = 2.0 * torch.sqrt(128.0 * m2_r) * eg + 128.0 * eg ** 2 + 16.0 * U * 128.0 * dev ** 2
        assert bool(torch.isfinite(st).all()), tag + ": non-finite row statistics"
        em, e2 = (st[..., 0] - mean_r).abs(), (st[..., 1] - m2_r).abs()
        assert bool((em <= tol_mean).all()), (tag + ": emitted group means", float((em / tol_mean).max()))
        assert bool((e2 <= tol_m2).all()), (tag + ": emitted group M2", float((e2 / tol_m2).max()))
    print(f"[gemm forms] {tag} bias={bias} res={res}: worst err {worst:.3f} x 2^-21 S")


def _facts_names():
    """the reported names of FACTS[] in csrc/gemm_f16x3_plan.hpp"""
    text = open(os.path.join(ROOT, "lemon_amd", "csrc", "gemm_f16x3_plan.hpp")).read()
    body = text[text.index("FACTS[N_FORMS] = {"):]
    return [ln.split('"')[1] for ln in body[:body.index("};")].splitlines() if ln.strip().startswith('{"')]


def test_form_table_is_complete():
    # every instantiation of the dispatcher once in the table, and every form through all eight n-tile counts
    assert sorted(FORMS) == list(range(1, 14)) and len({f["kernel"] for f in FORMS.values()}) == 13
    names = _facts_names()
    assert len(names) == 13 and {f["kernel"] for f in FORMS.values()} == set(names)
    for f in FORMS:
        cs = _cases(f)
        assert sorted(c[2] for c in cs) == list(N_ALL)
        assert {c[1] for c in cs} >= {1, 127, 128, 129} and any(c[1] > 4096 for c in cs)
        assert {c[3] for c in cs} == set(K_32X32 if FORMS[f].get("mfma") == 32 else K_EVEN)


# ---- the LayerNorm operand producers ------------------------------------------------------------------------------------
def _ln_rows(rows, width, seed):
    """rows of |mean| / sigma 0.3, 20, constant 0.5, constant 0.01, 1000, 6 in turn (sigma 0.5 ... 2.5)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = _std_rows(g, rows, width)
    scale = 0.5 + 2.0 * torch.rand(rows, 1, generator=g, device="cuda", dtype=torch.float64)
    shift = torch.tensor([0.3, 20.0, 0.0, 0.0, 1000.0, 6.0], dtype=torch.float64, device="cuda")[torch.arange(rows, device="cuda") % 6]
    x = (z + shift[:, None]) * scale
    kind = torch.arange(rows, device="cuda") % 6
    x[kind == 2] = 0.5
    x[kind == 3] = 0.01
    gamma = (1.0 + 0.3 * torch.randn(width, generator=g, device="cuda")).contiguous()
    beta = (0.2 * torch.randn(width, generator=g, device="cuda")).contiguous()
    return x.float().contiguous(), gamma, beta


def _ln_bound(x64, gamma, beta):
    """2^-21-units bracket of a LayerNorm output: rstd (|x_j| + mean |x|) |gamma_j| + |beta_j| (fp32 mean and variance of the row)"""
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + EPS)
    return rstd[:, None] * (x64.abs() + x64.abs().mean(1, keepdim=True)) * gamma.double().abs()[None, :] + beta.double().abs()[None, :]


@pytest.mark.parametrize("width", [36, 1020, 16, 48, 256, 768, 1024, 2048])
def test_layernorm_producers_against_float64(hip, width):
    lib = _lib().load()
    for rows in (1, 7, 129):
        x, gamma, beta = _ln_rows(rows, width, seed=rows * 4099 + width)
        x64 = x.double()
        ref = torch.nn.functional.layer_norm(x64, (width,), gamma.double(), beta.double(), EPS)
        S = _ln_bound(x64, gamma, beta)
        every = torch.ones(rows, dtype=torch.bool, device="cuda")
        tag = f"width {width} rows {rows}"
        # lemon_layernorm_f32 (k_layernorm for widths 4 x odd, k_layernorm8 otherwise)
        y = _words(rows * width, OUT_FILL)
        _check(lib.lemon_layernorm_f32(_p(x), _p(gamma), _p(beta), EPS, rows, width, _p(y), _stream()), "lemon_layernorm_f32")
        torch.cuda.synchronize()
        assert _tail_intact(y, rows * width), tag + ": lemon_layernorm_f32 wrote past the end"
        yf = y[:rows * width].view(torch.float32).view(rows, width)
        worst = [_assert_close(yf.double(), ref, S, every, tag + " lemon_layernorm_f32", C_LN)]
        if width % 16:
            print(f"[ln producers] {tag}: worst err {max(worst):.3f} x 2^-21")
            continue
        # lemon_layernorm_f16x3t: the split of lemon_layernorm_f32's values, bit for bit
        yt = _words(_rows_t(rows) * width, OUT_FILL)
        _check(lib.lemon_layernorm_f16x3t(_p(x), _p(gamma), _p(beta), EPS, rows, width, _p(yt), _stream()), "lemon_layernorm_f16x3t")
        torch.cuda.synchronize()
        assert _tail_intact(yt, _rows_t(rows) * width), tag + ": lemon_layernorm_f16x3t wrote past the end"
        hi, lo = _unpack(yt, rows, width)
        ehi, elo = _split(yf)
        assert torch.equal(hi.view(torch.int16), ehi.view(torch.int16)) and torch.equal(lo.view(torch.int16), elo.view(torch.int16)), tag
        worst.append(_assert_close(_value(hi, lo), ref, S + ref.abs(), every, tag + " lemon_layernorm_f16x3t", C_LN))
        # lemon_rowstats_f16x3t: the split of x itself + (rstd, -mean rstd), NaN beyond the fold's bound
        xt, aff = _words(_rows_t(rows) * width, OUT_FILL), _words(2 * rows, OUT_FILL)
        _check(lib.lemon_rowstats_f16x3t(_p(x), EPS, rows, width, _p(xt), _p(aff), _stream()), "lemon_rowstats_f16x3t")
        torch.cuda.synchronize()
        assert _tail_intact(xt, _rows_t(rows) * width) and _tail_intact(aff, 2 * rows), tag + ": lemon_rowstats_f16x3t wrote past the end"
        hi, lo = _unpack(xt, rows, width)
        ehi, elo = _split(x)
        assert torch.equal(hi.view(torch.int16), ehi.view(torch.int16)) and torch.equal(lo.view(torch.int16), elo.view(torch.int16)), tag
        worst.append(_check_row_aff(aff[:2 * rows].view(torch.float32).view(rows, 2), x64, tag + " lemon_rowstats_f16x3t"))
        if width % 256:
            print(f"[ln producers] {tag}: worst err {max(worst):.3f} x 2^-21")
            continue
        # lemon_ln_finalize on the rows' float64 (mean, M2) partials per 128 columns
        mean_g, m2_g, _ = _group_stats(x64, width)
        part = torch.stack([mean_g, m2_g], 2).float().contiguous()
        aff = _words(2 * rows, OUT_FILL)
        _check(lib.lemon_ln_finalize(_p(part), rows, width, EPS, _p(aff), _stream()), "lemon_ln_finalize")
        torch.cuda.synchronize()
        assert _tail_intact(aff, 2 * rows), tag + ": lemon_ln_finalize wrote past the end"
        worst.append(_check_row_aff(aff[:2 * rows].view(torch.float32).view(rows, 2), x64, tag + " lemon_ln_finalize"))
        print(f"[ln producers] {tag}: worst err {max(worst):.3f} x 2^-21")


def _check_row_aff(aff, x64, tag):
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    shift = mean.abs() * rstd
    far, near = shift > 1.001 * FOLD_MAX_SHIFT, shift < 0.999 * FOLD_MAX_SHIFT
    assert bool((far | near).all()), (tag, "a test row sits on the fold's bound")
    a = aff.double()
    assert not bool(torch.isfinite(a[far]).any()), tag + ": rows beyond the fold's bound must get a NaN row affine"
    assert bool(torch.isfinite(a[near]).all()), tag
    e_r = ((a[near, 0] - rstd[near]).abs() / rstd[near])
    e_m = (a[near, 1] + (mean * rstd)[near]).abs() / (rstd * (x64.abs().mean(1) + mean.abs()))[near]
    w_r = float(e_r.max()) / U if e_r.numel() else 0.0
    w_m = float(e_m.max()) / U if e_m.numel() else 0.0
    assert w_r <= C_LN, (tag + ": rstd", w_r)
    assert w_m <= C_LN, (tag + ": -mean rstd", w_m)
    return max(w_r, w_m)


# ---- tile-walk independence -----------------------------------------------------------------------------------------------
WALK_SHAPE = (4100, 1280, 64)         # 33 m-tiles x 5 n-tiles: ten super-blocks of the default walk (32 x 1), ragged under 3 x 2
WALK_FORMS = (9, 10, 5)


def _walk_outputs():
    """what forms 9, 10 and 5 owe at WALK_SHAPE, as CPU tensors (raw bits)"""
    m, n, k = WALK_SHAPE
    got = []
    for form in WALK_FORMS:
        inp = _inputs(form, m, n, k, True, FORMS[form]["act"] is None, seed=77 + form)
        outs = _launch(form, m, n, k, inp)
        for name in sorted(outs):
            buf, nw = outs[name]
            assert _tail_intact(buf, nw), (form, name)
            if name in ("op", "emit"):
                hi, lo = _unpack(buf, m, n)
                got += [hi.view(torch.int16).cpu(), lo.view(torch.int16).cpu()]
            else:
                got.append(buf[:nw].cpu())
    return got


_WALK_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from tests.test_gpu_gemm_forms import _walk_outputs
torch.save(_walk_outputs(), {path!r})
"""


def test_tile_walk_does_not_change_a_bit(hip, tmp_path):
    # LEMON_GEMM_WALK=gm,gn is read once per process: fresh children run the same forms under another super-block shape
    mine = _walk_outputs()
    for walk in ("1,1", "3,2"):
        path = str(tmp_path / f"walk_{walk.replace(',', '_')}.pt")
        env = dict(os.environ, LEMON_GEMM_WALK=walk)
        r = subprocess.run([sys.executable, "-c", _WALK_CHILD.format(root=ROOT, path=path)], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (walk, r.returncode, r.stderr[-3000:])
        theirs = torch.load(path)
        assert len(theirs) == len(mine)
        for i, (a, b) in enumerate(zip(mine, theirs)):
            assert torch.equal(a, b), (walk, i, int((a != b).sum()))
