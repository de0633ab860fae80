"""GPU: lemon_eval_metrics against its host twin, every field of every record by its bits (NaN included).  Segment sizes at
the edges of the kernels -- a wave, the 256-lane density workgroup, the 1 024-lane curve workgroup and density tile, numpy's
8 192-row chunk -- alone (S = 1, the plain sort), four and 33 to a call with odd offsets and gaps, thres_from pointing forwards
and backwards, tied scores; a bad segment among good ones; the refusals.  Every call runs with the workspace and the output
inside poisoned guards that must come back untouched."""
import ctypes

import numpy as np
import pytest

from tests import evalfx as fx

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1000, 1025, 8193, 20000)
GUARD = 4096
FIELDS = ("auroc", "auprc", "thres", "counts", "status", "kde_branch", "bisect_fallback", "pad")


def _flat(rec):
    """every field of a record as integers: the floats by their bits"""
    as_bits = lambda v: int(np.float64(v).view(np.int64))
    out = []
    for name in FIELDS:
        v = getattr(rec, name)
        if name == "thres":
            out += [as_bits(t) for t in v]
        elif name == "counts":
            out += [int(c) for row in v for c in row]
        elif name in ("auroc", "auprc"):
            out.append(as_bits(v))
        else:
            out.append(int(v))
    return out


def device_records(score, y, segments, ws_bytes=None, misalign=0, null=None, S=None, total=None):
    """the raw call with the workspace and the output between poisoned guards -> (rc, records, the output's bytes)"""
    import torch
    from lemon_amd import _lib, ops
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    n_seg = len(segments)
    free = sum(1 for g in segments if g[3] == -1)
    need = lib.lemon_eval_metrics_workspace_bytes(len(score), max(1, min(n_seg, 65535)), min(free, n_seg))
    assert need > 0, need
    given = need if ws_bytes is None else ws_bytes
    score_d = torch.from_numpy(np.ascontiguousarray(score, np.float64)).to(dev)
    y_d = torch.from_numpy(np.ascontiguousarray(np.asarray(y).astype(bool).astype(np.uint8))).to(dev)
    segs_d = torch.frombuffer(bytearray(bytes(ops.eval_segments(segments))), dtype=torch.uint8).to(dev)
    ws = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out_bytes = n_seg * ctypes.sizeof(_lib.EvalRecord)
    out = torch.full((GUARD + out_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert (ws.data_ptr() + GUARD) % 256 == 0 and (out.data_ptr() + GUARD) % 8 == 0
    args = [ops.ptr(score_d), ops.ptr(y_d), len(score) if total is None else total, ops.ptr(segs_d), n_seg if S is None else S,
            ctypes.c_void_p(ws.data_ptr() + GUARD + misalign), given, ctypes.c_void_p(out.data_ptr() + GUARD)]
    if null is not None:
        args[null] = None
    with torch.cuda.device(dev):
        rc = lib.lemon_eval_metrics(*args, ops.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    ws_h, out_h = ws.cpu().numpy(), out.cpu().numpy()
    assert (ws_h[:GUARD] == 0xA5).all() and (ws_h[GUARD + need:] == 0xA5).all(), "the call wrote outside its workspace"
    assert (out_h[:GUARD] == 0xA5).all() and (out_h[GUARD + out_bytes:] == 0xA5).all(), "the call wrote outside its output"
    body = out_h[GUARD:GUARD + out_bytes].tobytes()
    if rc != 0:
        assert (ws_h == 0xA5).all() and (out_h == 0xA5).all(), "a refused call wrote something"
    return rc, list((_lib.EvalRecord * n_seg).from_buffer_copy(body)), body


def _assert_equals_twin(score, y, segments):
    rc_t, twin = fx.host_records(score, y, segments)
    rc_d, got, _ = device_records(score, y, segments)
    assert rc_t == 0 and rc_d == 0
    for s, (g, t) in enumerate(zip(got, twin)):
        assert _flat(g) == _flat(t), (s, segments[s], dict(zip(FIELDS, (getattr(g, f) for f in FIELDS))), t.status, list(t.thres))
    return got


def _layout(sizes, seed, free_every=3):
    """segments of `sizes` with odd offsets and gaps: every free_every-th is free (the second first), a fixed one takes the
    thresholds of the nearest free one in front of it, or behind it where there is none in front"""
    rng = np.random.default_rng(seed)
    free = [s for s in range(len(sizes)) if s % free_every == 1]
    parts_s, parts_y, segments, at = [], [], [], 1
    parts_s.append(np.full(1, 7.0)); parts_y.append(np.zeros(1, bool))
    for s, n in enumerate(sizes):
        score, y = fx.mixture(n, 1000 * seed + s, centres=(0.0, 3.0 + (s % 3)))
        if s % 4 == 2:
            score = np.round(score, 1)
        if n >= 2:
            y[:2] = [True, False]
        gap = 1 + 2 * int(rng.integers(0, 3))
        before = [f for f in free if f < s]
        thres_from = -1 if s in free else (before[-1] if before else free[0])
        segments.append((at, n, float(y.sum() / n), thres_from))
        parts_s += [score, np.full(gap, -3.0)]; parts_y += [y, np.ones(gap, bool)]
        at += n + gap
    return np.concatenate(parts_s), np.concatenate(parts_y), segments


@pytest.mark.parametrize("n", SIZES)
def test_one_free_segment_equals_the_twin(hip, n):
    score, y = fx.mixture(n + 3, 50 + n)
    y[1:3] = [True, False]
    (rec,) = _assert_equals_twin(score, y, [(1, n, float(y[1:1 + n].sum() / n), -1)])
    assert rec.status == 0 and rec.kde_branch in (1, 2, 3, 4)


def test_ties_at_the_maximum_fall_back_to_fminbound(hip):
    score, y = fx.mixture(300, 21)
    score[:120] = score.max() + 1.0                      # 120 rows tied at the maximum > prevalence * n: bisect's sign error
    (rec,) = _assert_equals_twin(score, y, [(0, 300, 0.3, -1)])
    assert rec.bisect_fallback == 1


def test_four_segments_with_thresholds_from_behind_and_in_front(hip):
    score, y, segments = _layout((257, 1000, 63, 1025), 2, free_every=2)      # free: 1, 3 -> 0 looks forwards, 2 backwards
    assert [g[3] for g in segments] == [1, -1, 1, -1] and all(g[0] % 2 == 1 for g in segments[:1])
    got = _assert_equals_twin(score, y, segments)
    assert [r.status for r in got] == [0, 0, 0, 0]
    assert list(got[0].thres) == list(got[1].thres) == list(got[2].thres)


def test_thirty_three_segments(hip):
    sizes = [(2, 3, 63, 64, 65, 255, 256, 257, 1000, 1025, 5, 130)[s % 12] for s in range(33)]
    score, y, segments = _layout(sizes, 3)
    assert {g[3] for g in segments if g[3] != -1} >= {1, 4} and segments[0][3] == 1
    got = _assert_equals_twin(score, y, segments)
    assert all(r.status == 0 for r in got)


def test_a_bad_segment_leaves_the_good_ones_alone(hip):
    from lemon_amd import _lib
    score, y, segments = _layout((300, 64, 200, 12, 90, 1, 40, 30), 4, free_every=2)     # free: 1, 3, 5, 7
    good = [r for r in _assert_equals_twin(score, y, [segments[0], segments[1]])]
    off = {s: segments[s][0] for s in range(8)}
    score[off[2] + 7] = np.nan                           # fixed, a NaN
    score[off[3]:off[3] + 12] = 0.5                      # free, zero variance; 4 takes its thresholds from 3
    y[off[6]:off[6] + 40] = True                         # fixed, one class
    got = _assert_equals_twin(score, y, segments)        # 5: free with one row
    assert [r.status for r in got] == [0, 0, _lib.EVAL_NONFINITE, _lib.EVAL_ZERO_VARIANCE, _lib.EVAL_SOURCE, _lib.EVAL_FEW_ROWS,
                                       _lib.EVAL_ONE_CLASS, 0]
    for s in (0, 1):
        assert _flat(got[s]) == _flat(good[s])


def test_ops_eval_metrics_returns_the_host_paths_dicts(hip):
    import torch
    from lemon_amd import metrics as M, ops
    score, y = fx.mixture(700, 31)
    y[:2] = [True, False]
    holds, _ = fx.kde_separated(score[:200])
    assert holds
    dev = torch.device("cuda", torch.cuda.current_device())
    cat_s, cat_y = np.concatenate([score[:200], score]), np.concatenate([y[:200], y])
    prevalence = y[:200].sum() / 200
    segments = [(0, 200, prevalence, -1), (200, 200, prevalence, 0), (400, 500, prevalence, 0)]
    got = ops.eval_metrics(torch.from_numpy(cat_s).to(dev), torch.from_numpy(cat_y.astype(np.uint8)).to(dev), segments)
    free = M.eval_metrics(y[:200], score[:200], prevalence)
    want = [free, M.eval_metrics(y[:200], score[:200], prevalence, fix_thress=free),
            M.eval_metrics(y[200:], score[200:], prevalence, fix_thress=free)]
    for g, w, n in zip(got, want, (200, 200, 500)):
        fx.same_dict(g, w, auc_bound=n * 2.0 ** -52)
    cat_s[3] = np.inf
    with pytest.raises(ValueError):
        ops.eval_metrics(torch.from_numpy(cat_s).to(dev), torch.from_numpy(cat_y.astype(np.uint8)).to(dev), segments)
    with pytest.raises(Exception):
        ops.eval_metrics(torch.from_numpy(cat_s), torch.from_numpy(cat_y.astype(np.uint8)), segments)      # host tensors


def test_refusals_write_nothing(hip):
    score, y = fx.mixture(50, 15)
    good = [(0, 30, 0.3, -1), (31, 19, 0.3, 0)]
    assert device_records(score, y, good)[0] == 0
    for null in (0, 1, 3, 5, 7):
        assert device_records(score, y, good, null=null)[0] == -1, null
    assert device_records(score, y, good, S=0)[0] == -1 and device_records(score, y, good, S=65536)[0] == -1
    assert device_records(score, y, good, total=0)[0] == -1 and device_records(score, y, good, total=49)[0] == -1
    for bad in ([(-1, 10, 0.3, -1)], [(0, -5, 0.3, -1)], [(0, 0, 0.3, -1)], [(45, 6, 0.3, -1)], [(0, 30, 0.3, -1), (29, 10, 0.3, 0)],
                [(0, 30, 0.3, -1), (30, 20, 0.3, 1)], [(0, 30, 0.3, -1), (30, 20, 0.3, 2)], [(0, 30, 0.3, -2)], [(0, 30, 0.3, 0)]):
        assert device_records(score, y, bad)[0] == -1, bad
    from lemon_amd import _lib
    need = _lib.load().lemon_eval_metrics_workspace_bytes(50, 2, 1)
    assert device_records(score, y, good, ws_bytes=need - 1)[0] == -1
    assert device_records(score, y, good, misalign=8)[0] == -1
