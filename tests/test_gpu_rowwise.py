"""GPU: the row-wise scoring kernels (lemon_amd/csrc/rowwise.hip: k_normalize_rows, k_rowchain<1..5>, k_d1_normalized,
k_class_confidence, k_score) and the two token-assembly kernels (lemon_amd/csrc/encoder.hip: k_vision_tokens_ln,
k_text_tokens), called through the C ABI on buffers this file allocates itself, against the float64 references of
tests/rowwise_ref.py (verified without a GPU by tests/test_rowwise_host.py).

Poisoning, as in tests/test_gpu_gemm_forms.py: every output is filled with a NaN bit pattern and followed by a 4 KB canary
tail before the call; every element owed must come out finite and within its bound, every tail word must keep its bits, and
a refused call must leave the whole output as it was.  Inputs lie INSIDE larger NaN-filled buffers (rowwise.hip reads
scalars, so they start 4 bytes off a 16-byte boundary; the token kernels read float4, so theirs start 16 bytes in): a read
before the start or past the end reaches a result.

Bars.  normalize: 2 ulp of the float64 value (derived below).  Paired modes 1, 2 and d1_normalized: the numeric contract's
float32 chain -- bit-identical to the oracle (modes 1, 2) and inside the chain bound d 2^-24 sum |terms| + 2 ulp.  Paired
modes 3-5 and class_confidence have no chain to match: their bar is the float32 reference's own error against float64 (sklearn
pairwise on float32 + scipy softmax, the reference project's route), x 4 for another summation order, floor 2 ulp.  Every case
prints kernel error, reference error and their ratio.

Measured on an MI355X, worst kernel error / bar over all cases of a kernel (beyond 1 fails); cosine | euclidean | manhattan:
    single float32 chains (before)    paired_metric 0.45 | 2.10 | 4.84     class_confidence 0.72 | 5.20 | 1441, NaN on zero rows
    float64 partial sums (now)        paired_metric 0.24 | 0.25 | 0.25     class_confidence 0.22 | 0.19 | 0.24
The float32 reference's manhattan distance is a float64 value (scipy cdist), so its error is 0 and the bar is the 2-ulp floor;
with float64 sums the kernels' only error is the last rounding to float32 (half an ulp: 0.25 of the floor).  40 cases failed
on the single chains: all 20 paired cases with n >= 63 and d >= 63 (manhattan in each, euclidean at the larger d), class_confidence
euclidean in 8 and manhattan in 11 of its 12 tests (both d = 512 cases included), and the zero-row case."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rowwise_ref as R
from tests.test_gpu_gemm_forms import C_LN, OUT_FILL, TAIL, _assert_close, _ln_bound, _std_rows, _tail_intact, _words

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _lib():
    from lemon_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check(rc, what):
    _lib().check(rc, what)


_FILL = {torch.float32: float("nan"), torch.int32: 0x7FFFFFFF, torch.int64: 2 ** 40}


def _embed(a, lead=1, pad=64):
    """the array on the GPU, `lead` elements into a buffer that holds NaN (floats) or an out-of-range number (labels, ids)
    everywhere else; the view keeps the buffer alive"""
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).contiguous()
    buf = torch.full((lead + t.numel() + pad,), _FILL[t.dtype], dtype=t.dtype, device="cuda")
    buf[lead:lead + t.numel()] = t.reshape(-1).cuda()
    return buf[lead:lead + t.numel()].view(t.shape)


def _out(n):
    """n poisoned int32 words + the canary tail"""
    return _words(n, OUT_FILL)


def _f32(buf, n):
    return buf[:n].view(torch.float32)


def _f64(buf, n):
    return buf[:2 * n].view(torch.float64)


def _untouched(buf, n):
    return bool((buf[:n + TAIL] == OUT_FILL).all())


def _ratio(err, bar):
    """worst err / bar; an exact result under a bar of zero counts as 0"""
    err, bar = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64))
    return float(np.where(err == 0.0, 0.0, err / np.maximum(bar, 1e-300)).max())


SUBNORMAL = 2.0 ** -149          # one step of the float32 output format: no float32 result is closer to a tiny value


def _finite(x, what):
    assert np.isfinite(x).all(), f"{what}: {int((~np.isfinite(x)).sum())} elements not written or not finite"


# ---- lemon_normalize_rows ------------------------------------------------------------------------------------------------
def _normalize(x, n, d, x_lead, y_lead, inplace=False):
    lib = _lib().load()
    xd = _embed(x, lead=x_lead)
    if inplace:
        _check(lib.lemon_normalize_rows(_p(xd), n, d, _p(xd), _stream()), "lemon_normalize_rows")
        torch.cuda.synchronize()
        base = xd._base
        assert bool(torch.isnan(base[:x_lead]).all()) and bool(torch.isnan(base[x_lead + n * d:]).all()), "in place: wrote around x"
        return xd.cpu().numpy()
    y = _out(y_lead + n * d)
    _check(lib.lemon_normalize_rows(_p(xd), n, d, ctypes.c_void_p(y.data_ptr() + 4 * y_lead), _stream()), "lemon_normalize_rows")
    torch.cuda.synchronize()
    assert _tail_intact(y, y_lead + n * d) and bool((y[:y_lead] == OUT_FILL).all()), "lemon_normalize_rows wrote outside y"
    return _f32(y[y_lead:], n * d).view(n, d).cpu().numpy()


@pytest.mark.parametrize("n,d", [(1, 1), (5, 4), (6, 256), (9, 260), (4, 3), (7, 1000)])
def test_normalize_rows_within_2_ulp_on_every_path(hip, n, d):
    """den is the float32 rounding of a float64 root (relative error 2^-24) and each element one float32 division (half an
    ulp): x / den is within 1 + 1/2 + second-order < 2 ulp of the float64 x / max(|x|, 1e-12) rounded to float32."""
    rng = np.random.default_rng(n * 1009 + d)
    x = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    if n >= 4:
        x[0] = 0.0
        x[1] = 1e-20                      # norm below the 1e-12 floor: divided by 1e-12
        x[2] = 1e30
        x[3, d // 2] = 1e-40              # a float32 subnormal
    ref = R.normalize_rows(x)
    # 0 / 4 elements in: both 16-byte aligned (the float4 path when d % 4 == 0); 1 element in: 4 bytes off (scalar path)
    runs = {"aligned": _normalize(x, n, d, 0, 0), "aligned+16": _normalize(x, n, d, 4, 4), "x off": _normalize(x, n, d, 1, 0),
            "y off": _normalize(x, n, d, 0, 1), "both off": _normalize(x, n, d, 1, 1),
            "in place": _normalize(x, n, d, 0, 0, inplace=True), "in place off": _normalize(x, n, d, 1, 0, inplace=True)}
    worst = 0.0
    for name, got in runs.items():
        _finite(got, f"normalize {n}x{d} {name}")
        e = R.ulps(got, ref)
        assert e.max() <= 2.0, (name, float(e.max()), np.unravel_index(e.argmax(), e.shape))
        worst = max(worst, float(e.max()))
        # the scalar path on a misaligned pointer and the in-place call give the bits of the aligned call
        assert np.array_equal(got.view(np.int32), runs["aligned"].view(np.int32)), name
    if n >= 4:
        assert np.all(runs["aligned"][0] == 0.0) and np.all(runs["aligned"][1] == np.float32(1e-20) / np.float32(1e-12))
    print(f"[rowwise] normalize n={n} d={d}: worst {worst:.2f} ulp over {len(runs)} paths")


# ---- lemon_paired_distance / lemon_paired_metric -------------------------------------------------------------------------
def _paired(mode, a_dev, b_dev, n, d):
    lib = _lib().load()
    out = _out(n)
    if mode in (1, 2):
        _check(lib.lemon_paired_distance(mode - 1, _p(a_dev), _p(b_dev), n, d, _p(out), _stream()), "lemon_paired_distance")
    else:
        _check(lib.lemon_paired_metric(R.KIND_OF_MODE[mode], _p(a_dev), _p(b_dev), n, d, _p(out), _stream()), "lemon_paired_metric")
    torch.cuda.synchronize()
    assert _tail_intact(out, n), f"paired mode {mode}: write past the end"
    got = _f32(out, n).cpu().numpy()
    _finite(got, f"paired mode {mode} n={n} d={d}")
    return got


@pytest.mark.parametrize("d", [1, 63, 64, 65, 129, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_paired_modes_against_float64(hip, oracle, n, d):
    rng = np.random.default_rng(n * 1000 + d)
    a = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    b = (rng.standard_normal((n, d)) * 0.5).astype(np.float32)
    a_dev, b_dev = _embed(a), _embed(b)
    beyond = []                                      # (every figure is printed before anything is asserted on it)
    for mode in (1, 2, 3, 4, 5):
        got = _paired(mode, a_dev, b_dev, n, d)
        ref = R.paired(mode, a, b)
        err = np.abs(got.astype(np.float64) - ref)
        bound = R.paired_chain_bound(mode, a, b)
        assert np.all(err <= bound), (mode, "chain bound", float((err / bound).max()))
        if mode in (1, 2):
            # the numeric contract's chain: bit for bit the oracle's
            want = oracle.paired_distance("cosine" if mode == 1 else "euclidean", a, b)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (mode, "not the contract's chain")
            continue
        kind = R.KIND_OF_MODE[mode]
        ref_err = float(np.abs(R.sk_paired_metric(kind, a, b).astype(np.float64) - ref).max())
        # (the floor's scale: the value itself; for the cosine distance the similarity ~ 1 it is subtracted from)
        bar = R.reference_bar(ref_err, np.maximum(np.abs(ref), 1.0) if kind == 0 else np.abs(ref))
        ratio = _ratio(err, bar)
        print(f"[rowwise] paired_metric {R.KIND_NAMES[kind]} n={n} d={d}: kernel err {err.max():.3e}  float32 reference err {ref_err:.3e}"
              f"  kernel/reference {err.max() / ref_err if ref_err else float('inf'):.2f}  kernel/bar {ratio:.3f}")
        if not ratio <= 1.0:
            beyond.append((R.KIND_NAMES[kind], ratio))
    assert not beyond, (n, d, "kernel error / bar", beyond)


def test_paired_metric_edge_rows(hip):
    n, d = 65, 65
    rng = np.random.default_rng(11)
    a = rng.standard_normal((n, d)).astype(np.float32)
    b = rng.standard_normal((n, d)).astype(np.float32)
    same, za, zb, zab = [0, 31, 64], [1, 63], [2], [3]
    b[same] = a[same]
    a[za] = 0.0
    b[zb] = 0.0
    a[zab] = 0.0
    b[zab] = 0.0
    a_dev, b_dev = _embed(a), _embed(b)
    eu, ma, co = (_paired(m, a_dev, b_dev, n, d) for m in (3, 4, 5))
    assert np.all(eu[same] == 0.0) and np.all(ma[same] == 0.0), "a == b: euclidean and manhattan are exactly 0"
    assert np.all(np.abs(co[same]) <= 2.0 ** -22), ("a == b: cosine", co[same])
    assert np.all(co[za + zb + zab] == 1.0), ("a zero row has cosine distance exactly 1, as sklearn gives", co[za + zb + zab])
    assert np.all(eu[zab] == 0.0) and np.all(ma[zab] == 0.0)
    sk = R.sk_paired_metric(0, a, b)
    assert np.all(sk[za + zb + zab] == 1.0)                       # (what the reference's route gives here)
    # the cosine does not depend on the rows' scale
    ref, bound = R.paired(5, a, b), R.paired_chain_bound(5, a, b)
    for s in (1e-10, 1e10):
        for t in (1e-10, 1e10):
            got = _paired(5, _embed(a * np.float32(s)), _embed(b * np.float32(t)), n, d)
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= bound), (s, t, float((err / bound).max()))


# ---- lemon_d1_normalized / lemon_class_confidence ------------------------------------------------------------------------
FNS = ("d1-ip", "d1-l2", "conf-cosine", "conf-euclidean", "conf-manhattan")


def _class_call(fn, img_dev, n, d, cls_dev, C, lab_dev, expect=0):
    """one call on a poisoned output: float32 [n]; expect != 0: the call must be refused with that code and write nothing"""
    lib = _lib().load()
    out = _out(max(n, 1))
    if fn.startswith("d1"):
        rc = lib.lemon_d1_normalized(0 if fn == "d1-ip" else 1, _p(img_dev), n, d, _p(cls_dev), C, _p(lab_dev), _p(out), _stream())
    else:
        rc = lib.lemon_class_confidence(R.KIND_NAMES.index(fn[5:]), _p(img_dev), n, d, _p(cls_dev), C, _p(lab_dev), _p(out), _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (fn, rc)
        assert _untouched(out, max(n, 1)), f"{fn}: a refused call wrote to its output"
        return None
    _check(rc, fn)
    assert _tail_intact(out, n), f"{fn}: write past the end"
    return _f32(out, n).cpu().numpy()


def _slot_labels(C, n):
    """labels that read every lane slot: class 0, the last class, 63, 64 and the first class of the last slot"""
    want = [0, C - 1, 63, 64, 64 * ((C - 1) // 64)]
    lab = [min(c, C - 1) for c in want]
    return np.array(lab[:n] if n > 1 else [C - 1], dtype=np.int32)


def _class_inputs(fn, C, d, n, scale, seed):
    rng = np.random.default_rng(seed)
    img, cls = rng.standard_normal((n, d)), rng.standard_normal((C, d))
    if fn.startswith("d1"):                              # run_lemon.py normalises both sides first
        img, cls = R.normalize_rows(img), R.normalize_rows(cls)
    elif scale == "ten":                                 # |row| ~ 10: raw CLIP embeddings
        img, cls = img * (10 / d ** 0.5), cls * (10 / d ** 0.5)
    else:                                                # the scale of tests/golden/zero_shot.npz (tools/make_golden.py)
        img, cls = img * rng.uniform(0.5, 3, (n, 1)), cls * rng.uniform(0.5, 3, (C, 1))
    return img.astype(np.float32), cls.astype(np.float32)


def _class_check(fn, img, cls, lab, got, tag):
    """the float64 comparison of one call: (worst relative error, worst error / bar, the float32 reference's worst relative
    error or None, bar).  Relative errors are taken after one float32 subnormal step has been allowed: a confidence below
    1.2e-38 has no float32 neighbour within 2 ulp relative."""
    _finite(got, tag)

    def rel_err(x, ref):
        return np.maximum(np.abs(np.asarray(x, np.float64) - ref) - SUBNORMAL, 0.0) / ref

    if fn.startswith("d1"):
        metric = fn[3:]
        ref = R.d1_normalized(metric, img, cls, lab)
        rel, bar = rel_err(got, ref), R.d1_chain_bound(metric, img, cls)
        return float(rel.max()), _ratio(rel, bar), None, bar
    kind = R.KIND_NAMES.index(fn[5:])
    ref = R.class_confidence(kind, img, cls, lab)
    rel = rel_err(got, ref)
    ref_err = float(rel_err(R.sk_class_confidence(kind, img, cls, lab), ref).max())
    bar = R.reference_bar(ref_err, 1.0)
    return float(rel.max()), _ratio(rel, bar), ref_err, bar


def _run_class_case(fn, C, d, n, scale, oracle=None):
    """one call, its figures printed; returns the list of (case, kernel error / bar) beyond the bar"""
    img, cls = _class_inputs(fn, C, d, n, scale, seed=C * 7919 + d * 31 + n + len(scale))
    lab = _slot_labels(C, n)
    got = _class_call(fn, _embed(img), n, d, _embed(cls), C, _embed(lab))
    tag = f"{fn} C={C} d={d} n={n} {scale}"
    err, ratio, ref_err, bar = _class_check(fn, img, cls, lab, got, tag)
    if ref_err is None:
        print(f"[rowwise] {tag}: kernel rel err {err:.3e}  chain bound {float(np.max(bar)):.3e}  kernel/bound {ratio:.3f}")
        want = oracle.d1_normalized("cosine" if fn == "d1-ip" else "euclidean", img, cls, lab)
        assert np.abs(got - want).max() <= 1e-6, (tag, "oracle")
    else:
        print(f"[rowwise] {tag}: kernel rel err {err:.3e}  float32 reference rel err {ref_err:.3e}"
              f"  kernel/reference {err / ref_err if ref_err else float('inf'):.2f}  kernel/bar {ratio:.3f}")
    return [] if ratio <= 1.0 else [(tag, ratio)]


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 128, 129, 1000, 1023, 1024])
@pytest.mark.parametrize("fn", FNS)
def test_class_softmax_against_float64(hip, oracle, fn, C):
    beyond = []
    for d in (1, 3, 64):
        for n in (1, 5):
            for scale in (("unit",) if fn.startswith("d1") else ("ten", "golden")):
                beyond += _run_class_case(fn, C, d, n, scale, oracle)
    assert not beyond, ("kernel error / bar", beyond)


@pytest.mark.parametrize("C", [10, 129])
@pytest.mark.parametrize("fn", FNS)
def test_class_softmax_at_the_workload_dimension(hip, oracle, fn, C):
    # d = 512, |row| ~ 10: where a single float32 chain over d is an order of magnitude worse than the float32 reference
    beyond = [b for n in (1, 5) for b in _run_class_case(fn, C, 512, n, "unit" if fn.startswith("d1") else "ten", oracle)]
    assert not beyond, ("kernel error / bar", beyond)


@pytest.mark.parametrize("C", [1, 64, 65, 129, 1024])
@pytest.mark.parametrize("fn", FNS)
def test_class_softmax_sums_to_one_over_the_labels(hip, fn, C):
    # n = C copies of one image with labels 0 .. C-1: a class dropped or counted twice at a slot boundary shows in the sum
    d = 3
    img, cls = _class_inputs(fn, C, d, 1, "golden", seed=C)
    img = np.repeat(img, C, 0)
    lab = np.arange(C, dtype=np.int32)
    got = _class_call(fn, _embed(img), C, d, _embed(cls), C, _embed(lab))
    _finite(got, f"{fn} C={C}")
    total = float(got.astype(np.float64).sum())
    assert abs(total - 1.0) <= C * 2.0 ** -23, (fn, C, total)
    ref = R.d1_normalized(fn[3:], img, cls, lab) if fn.startswith("d1") else R.class_confidence(R.KIND_NAMES.index(fn[5:]), img, cls, lab)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-37)


@pytest.mark.parametrize("fn", FNS)
def test_class_count_limits_are_refused_and_nothing_is_written(hip, fn):
    d, n = 3, 2
    img = _embed(np.ones((n, d), np.float32))
    lab = _embed(np.zeros(n, np.int32))
    cls = _embed(np.ones((1025, d), np.float32))
    _class_call(fn, img, n, d, cls, 1025, lab, expect=E_INVALID)
    _class_call(fn, img, n, d, cls, 0, lab, expect=E_INVALID)
    assert _class_call(fn, img, n, d, cls, 1024, lab) is not None           # the limit itself is served


def test_zero_rows_give_the_reference_cosine_not_nan(hip):
    """a zero image row used to give 0 / 0 = NaN in k_class_confidence; sklearn's cosine_similarity gives similarity 0, so
    every class is at distance 1 and the confidence is 1 / C"""
    C, d, n = 65, 24, 3
    img, cls = _class_inputs("conf-cosine", C, d, n, "golden", seed=5)
    img[1] = 0.0
    cls[2] = 0.0
    cls[64] = 0.0
    lab = np.array([2, 64, 64], dtype=np.int32)
    img_dev, cls_dev = _embed(img), _embed(cls)
    got = _class_call("conf-cosine", img_dev, n, d, cls_dev, C, _embed(lab))
    err, ratio, ref_err, bar = _class_check("conf-cosine", img, cls, lab, got, "zero rows")
    print(f"[rowwise] conf-cosine zero rows: kernel rel err {err:.3e}  float32 reference rel err {ref_err:.3e}  kernel/bar {ratio:.3f}")
    assert ratio <= 1.0, (got, ratio)
    assert abs(float(got[1]) - 1.0 / C) <= 2.0 ** -24 / C * 2
    # k_rowchain<5> on the same pairs: exactly 1 for every pair with a zero row, and the same confidences from its distances
    for i in range(n):
        dist = _paired(5, _embed(np.repeat(img[i][None], C, 0)), cls_dev, C, d).astype(np.float64)
        if i == 1:
            assert np.all(dist == 1.0)
        assert dist[2] == 1.0 and dist[64] == 1.0
        conf = R.softmax_rows((1.0 - dist)[None, :])[0, lab[i]]
        # (each distance was rounded to float32: 2^-24 |dist| <= 2^-23, twice in a softmax entry, + the store's rounding)
        assert abs(float(got[i]) - conf) <= (4 * 2.0 ** -23 + 2.0 ** -24) * conf, (i, float(got[i]), conf)


def test_labels_outside_the_classes(hip):
    from lemon_amd import ops
    from lemon_amd.baselines import clip_logits_confidence
    C, d, n = 10, 8, 4
    # the C ABI does not look at the labels: one outside [0, C) matches no class and gives exactly 0 (include/lemon_hip.h)
    lab = np.array([0, C, -1, 2 ** 31 - 1], dtype=np.int32)
    for fn in FNS:
        img, cls = _class_inputs(fn, C, d, n, "golden", seed=9)
        got = _class_call(fn, _embed(img), n, d, _embed(cls), C, _embed(lab))
        assert got[0] > 0 and np.all(got[1:] == 0.0), (fn, got)
    img, cls = _class_inputs("d1-ip", C, d, n, "unit", seed=9)
    # the wrappers see the labels on the host and raise where the reference would raise (>= C) or wrap round (< 0)
    q, c = torch.from_numpy(img).cuda(), torch.from_numpy(cls).cuda()
    for bad in ([0, C, 1, 2], [0, -1, 1, 2]):
        for labels in (np.array(bad), torch.tensor(bad), torch.tensor(bad, dtype=torch.int32).cuda()):
            with pytest.raises(ValueError):
                ops.d1_normalized("cosine", q, c, labels)
            with pytest.raises(ValueError):
                clip_logits_confidence(q, c, labels, "euclidean")
    with pytest.raises(ValueError):
        ops.d1_normalized("cosine", q, c[:, :7].contiguous(), np.zeros(n, np.int64))          # mismatched d
    with pytest.raises(ValueError):
        ops.d1_normalized("cosine", q, c, np.zeros(n + 1, np.int64))                          # one label per row
    ok = np.array([0, C - 1, 3, 3])
    assert np.allclose(ops.d1_normalized("cosine", q, c, ok).cpu().numpy(), R.d1_normalized("ip", img, cls, ok), rtol=1e-5)
    assert np.allclose(clip_logits_confidence(q, c, ok, "manhattan").cpu().numpy(), R.class_confidence(2, img, cls, ok), rtol=1e-6)


# ---- lemon_score ---------------------------------------------------------------------------------------------------------
SCORE_KEYS = ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")


def _score_rec(n, k, seed):
    rng = np.random.default_rng(seed)
    rec = {"d_1": rng.random(n).astype(np.float32)}
    for nm in SCORE_KEYS[1:]:
        rec[nm] = (0.0625 + rng.random((n, k))).astype(np.float32)          # >= 2^-4: float64 sums of them are exact
    return rec


def _score(rec, hp, n, k, with_dn):
    lib = _lib().load()
    dev = [_embed(rec[nm]) for nm in SCORE_KEYS]
    s, dn, dm = _out(2 * n), _out(2 * n), _out(2 * n)
    hpc = (ctypes.c_double * 6)(*[float(h) for h in hp])
    _check(lib.lemon_score(*[_p(t) for t in dev], n, k, hpc, _p(s), _p(dn) if with_dn else None, _p(dm) if with_dn else None,
                           _stream()), "lemon_score")
    torch.cuda.synchronize()
    assert _tail_intact(s, 2 * n) and (_tail_intact(dn, 2 * n) and _tail_intact(dm, 2 * n) if with_dn else _untouched(dn, 2 * n) and _untouched(dm, 2 * n))
    return (_f64(s, n).cpu().numpy(),) + ((_f64(dn, n).cpu().numpy(), _f64(dm, n).cpu().numpy()) if with_dn else (None, None))


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_score_against_float64_and_at_its_edges(hip, n, k):
    rec = _score_rec(n, k, seed=n * 100 + k)
    hp = [5.0, 3.0, 0.1, 5.0, 1.5, 0.25]
    ref = R.score(rec, hp)
    for with_dn in (True, False):
        got = _score(rec, hp, n, k, with_dn)
        for g, r, nm in zip(got, ref, ("score", "d_n", "d_m")):
            if g is not None:
                _finite(g, f"lemon_score {nm} n={n} k={k}")
                assert np.allclose(g, r, rtol=1e-9, atol=0), (nm, with_dn, float(np.abs(g / r - 1).max()))
    # every tau zero: d_n is exactly the float64 mean of dists_n
    s, dn, dm = _score(rec, [2.0, 0.5, 0.0, 0.0, 0.0, 0.0], n, k, True)
    r = R.score(rec, [2.0, 0.5, 0.0, 0.0, 0.0, 0.0])
    assert np.array_equal(dn, r[1]) and np.array_equal(dm, r[2]) and np.allclose(s, r[0], rtol=1e-15, atol=0)
    # tau large enough to underflow every weight: the score is d_1, exactly
    s, dn, dm = _score(rec, [5.0, 3.0, 1e6, 0.0, 0.0, 1e6], n, k, True)
    assert np.array_equal(s, rec["d_1"].astype(np.float64)) and np.all(dn == 0.0) and np.all(dm == 0.0)
    # tau and a negative D that overflow to inf next to a zero dists: NaN exactly where the reference has it
    rec2 = {key: v.copy() for key, v in rec.items()}
    rec2["D_n"] = -rec2["D_n"]
    rec2["dists_n"][::3, k // 2] = 0.0
    hp2 = [5.0, 3.0, 1e6, 0.0, 0.1, 0.0]
    s, dn, dm = _score(rec2, hp2, n, k, True)
    r = R.score(rec2, hp2)
    assert np.isnan(r[1][::3]).all() and not np.isnan(np.delete(r[1], np.arange(0, n, 3))).any()
    assert np.array_equal(np.isnan(s), np.isnan(r[0])) and np.array_equal(np.isnan(dn), np.isnan(r[1]))
    assert np.allclose(s, r[0], rtol=1e-9, atol=0, equal_nan=True) and np.allclose(dn, r[1], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(dm, r[2], rtol=1e-9, atol=0)


# ---- lemon_vision_tokens_ln ----------------------------------------------------------------------------------------------
EPS = 1e-5
BATCH = 3


def _vision_inputs(width, n_tokens, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 0.5 + 2.0 * torch.rand(BATCH, n_tokens - 1, 1, generator=g, device="cuda", dtype=torch.float64)
    pos = 0.5 * torch.randn(n_tokens, width, generator=g, device="cuda", dtype=torch.float64)
    patches = torch.randn(BATCH, n_tokens - 1, width, generator=g, device="cuda", dtype=torch.float64) * scale + 0.3
    # one row with |mean| / sigma = 30: image 1, token 1
    patches[1, 0] = (_std_rows(g, 1, width)[0] + 30.0) * 0.7 - pos[1]
    cls = torch.randn(width, generator=g, device="cuda")
    gamma = 1.0 + 0.3 * torch.randn(width, generator=g, device="cuda")
    beta = 0.2 * torch.randn(width, generator=g, device="cuda")
    return patches.float(), cls, pos.float(), gamma, beta


def _vision_call(patches, cls, pos, gamma, beta, n_tokens, width, expect=0):
    lib = _lib().load()
    nw = BATCH * n_tokens * width
    y = _out(nw)
    keep = [_embed(t.cpu(), lead=4) if t is not None else None for t in (patches, cls, pos, gamma, beta)]
    rc = lib.lemon_vision_tokens_ln(*[_p(t) for t in keep], EPS, BATCH, n_tokens, width, _p(y), _stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, rc
        assert _untouched(y, nw), "a refused lemon_vision_tokens_ln wrote to its output"
        return None
    _check(rc, "lemon_vision_tokens_ln")
    assert _tail_intact(y, nw), "lemon_vision_tokens_ln wrote past the end"
    return _f32(y, nw).view(BATCH * n_tokens, width)


@pytest.mark.parametrize("n_tokens", [2, 5])
@pytest.mark.parametrize("width", [4, 36, 512, 516, 1024, 1028, 2048])
def test_vision_tokens_layernorm_against_float64(hip, width, n_tokens):
    patches, cls, pos, gamma, beta = _vision_inputs(width, n_tokens, seed=width * 10 + n_tokens)
    got = _vision_call(patches, cls, pos, gamma, beta, n_tokens, width)
    x64 = R.vision_tokens(patches, cls, pos).reshape(BATCH * n_tokens, width)
    assert abs(float(x64[n_tokens + 1].mean() / x64[n_tokens + 1].std(unbiased=False))) > 25 or width == 4
    ref = R.vision_tokens_ln(patches, cls, pos, gamma, beta, EPS).reshape(BATCH * n_tokens, width)
    every = torch.ones(BATCH * n_tokens, dtype=torch.bool, device="cuda")
    worst = _assert_close(got.double(), ref, _ln_bound(x64, gamma, beta), every, f"vision tokens width {width} n_tokens {n_tokens}", C_LN)
    print(f"[rowwise] vision_tokens_ln width={width} n_tokens={n_tokens}: worst err {worst:.3f} x 2^-21 (bound {C_LN})")


def test_vision_tokens_refusals_write_nothing(hip):
    for width, n_tokens, drop in ((2052, 2, None), (6, 2, None), (512, 1, None), (512, 2, "weight"), (512, 2, "bias")):
        g = torch.Generator().manual_seed(0)
        wpad = (width + 3) // 4 * 4
        patches = torch.randn(BATCH, max(n_tokens - 1, 1), wpad, generator=g)
        cls, pos = torch.randn(wpad, generator=g), torch.randn(max(n_tokens, 2), wpad, generator=g)
        gamma, beta = torch.ones(wpad), torch.zeros(wpad)
        _vision_call(patches, cls, pos, None if drop == "weight" else gamma, None if drop == "bias" else beta, n_tokens, width,
                     expect=E_INVALID)


# ---- lemon_text_tokens ---------------------------------------------------------------------------------------------------
VOCAB = 50


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("seq_len", [1, 7])
@pytest.mark.parametrize("width", [4, 260, 768])
def test_text_tokens_bit_equal_with_clamped_ids(hip, width, seq_len, extra):
    lib = _lib().load()
    g = torch.Generator().manual_seed(width + seq_len + extra)
    tok, pos = torch.randn(VOCAB, width, generator=g), torch.randn(seq_len, width, generator=g)
    pitch = seq_len + extra
    ids = torch.randint(0, VOCAB, (BATCH, pitch), generator=g)
    # ids on and beyond both ends of the vocabulary (with seq_len 1 the three rows take -3, vocab + 9 and vocab - 1)
    special = [-3, VOCAB + 9, VOCAB - 1, 0]
    flat = ids[:, :seq_len].reshape(-1).clone()
    flat[:min(4, flat.numel())] = torch.tensor(special[:flat.numel()])
    ids[:, :seq_len] = flat.view(BATCH, seq_len)
    ids[:, seq_len:] = 2 ** 40                                     # columns the kernel must never read
    nw = BATCH * seq_len * width
    y = _out(nw)
    ids_dev, tok_dev, pos_dev = _embed(ids, lead=2), _embed(tok, lead=4), _embed(pos, lead=4)
    _check(lib.lemon_text_tokens(_p(ids_dev), pitch, _p(tok_dev), _p(pos_dev), BATCH, seq_len, width, VOCAB, _p(y), _stream()),
           "lemon_text_tokens")
    torch.cuda.synchronize()
    assert _tail_intact(y, nw), "lemon_text_tokens wrote past the end"
    got = _f32(y, nw).view(BATCH, seq_len, width).cpu()
    assert bool(torch.isfinite(got).all())
    ref = R.text_tokens(ids, seq_len, tok, pos)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), int((got != ref).sum())
    assert torch.equal(ref, tok[ids[:, :seq_len].clamp(0, VOCAB - 1)] + pos)
