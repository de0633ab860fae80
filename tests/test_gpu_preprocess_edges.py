"""GPU: the image preprocessing kernels (lemon_amd/csrc/preprocess.hip: k_preprocess_u8, k_ragged_h, k_ragged_v) through the
C ABI alone (lemon_preprocess_u8, lemon_preprocess_u8_f16x3t, lemon_preprocess_ragged) on buffers, tap tables, plans and
descriptors this file builds itself, against tests/preprocess_ref.py (int64 passes + float32 epilogue in numpy, pinned
against PIL + torch without a GPU by tests/test_preprocess_host.py).  The bar is bit equality everywhere.

Poisoning, as in tests/test_gpu_gemm_forms.py and tests/test_gpu_rowwise.py: every output is OUT_FILL words followed by a
4 KB canary tail.  The whole buffer is compared with one expected buffer: the reference's bits in every word owed, the poison
in every other word -- the tail, the padding rows of a tile-major operand up to the next multiple of 128, and any half-word
of it that _tiled_index of the owed rows does not address.  The ragged kernels' intermediate (`work`) is poisoned bytes with
a tail and compared the same way: each good image's slice holds the reference's horizontal pass, every other byte its poison.
A refused call leaves every word as it was.

Two surrounds.  Images are uint8 and cannot hold a NaN, so a read outside them cannot be made loud; instead each case runs
twice, the image bytes at an ODD byte offset inside a buffer of 0x00 and then of 0xFF, the tap and bound tables inside int32
buffers whose other entries are LEGAL ones: 0 (a window of no taps at input 0) in the first run, tap 1 << 22 and bound
(0, 1) in the second.  A stray read changes a value, never an address; both runs must give the reference's bits.

Shapes (batch 3 unless stated, so that the workgroup -> image map matters; axis tables are built independently per axis):

    same-shape kernel
    blocks     5x5 -> 12 and -> 10, R in 1, 2, 4, 5, 8, 16      every row-block count, tails of 2 and 4 rows, R > S; the 4-pixel
                                                               (S = 12) and 1-pixel (S = 10) vertical form; max_rows = true span
    taps       sides 1, 2, 3 on each axis -> 8                 windows clipped at both ends (1 to 3 taps of 5)
               8x5, 5x8, 8x8 -> 8                              the identity table on one axis and on both
               508x4 -> 4 at R = 1                             509 vertical taps: 511 of the window table's 512 ints
               4x508 -> 4                                      509 horizontal taps
               40x56: rows [9, 21) of 30, columns [15, 27) of 42   a crop on both axes: vmin > 0 and xmin > 0, down-scaling
    layouts    5x7 -> 12 with P in 0, 4, 12, 6, 3              4-pixel form: NCHW, patches, one patch; 1-pixel form WITH patches
               5x7 -> 10 with P in 0, 5, 2; 9x11 -> 28, P = 14 at S % 4 == 0 (6, 3, 14: the ViT-L/14 case) and at S % 4 != 0
    operand    S = 12, P = 4 (K = 48): batch 3 and 15          27 rows + 101 pad rows; 135 rows across a tile + 121 pad rows
               S = 16, P = 8 (K = 192), batch 9                36 rows, twelve k16 steps
    ragged kernels
    launch     S = 20 and S = 18: 1x1, 3x2, 5x7, 5x7, SxS,     clipped windows, a shared plan, the identity, 2 vertical blocks with a
               64x48, 40x90, at odd offsets in the packed      tail, 3-4 horizontal blocks with a tail (> 16 input rows); every
               buffer                                          output form: NCHW, patches in both vertical forms, the operand
    taps       4092x4 -> 4 at R = 1                            4093 vertical taps: 4095 of k_ragged_v's 4096 ints
    sub-batch  descriptors 4, 1, 1, 6, 0 of the S = 20 launch  a permutation with a repeat gives the rows of the full batch
    guard      one of 5 descriptors bad in each way ragged_ok   that image NaN wherever owed in all three forms, its work slice
               checks                                          poison, the other four images as in the unbroken batch

Content: {0, 255} noise on the up-scaling block and layout cases, where the test asserts that the REFERENCE's values before
the clip go below 0 and above 255 in both passes (an axis of one pixel cannot overshoot: its weights sum to one tap);
smooth content plus noise elsewhere."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests.test_gpu_gemm_forms import OUT_FILL, TAIL, TM, _words

pytestmark = pytest.mark.gpu

E_INVALID = -1
LEAD = 13                     # bytes in front of an embedded image: odd
T_LEAD, T_PAD = 6, 64         # ints around an embedded table (even, so that stray bound pairs stay pairs)
WORK_FILL, WORK_TAIL = 0xA5, 4096
ONE = 1 << 22                 # the identity tap
MEAN = (ctypes.c_float * 3)(*[float(v) for v in PR.MEAN])
STD = (ctypes.c_float * 3)(*[float(v) for v in PR.STD])
SURROUNDS = ((0x00, False), (0xFF, True))      # (image surround byte, tables surrounded by (ONE, (0, 1)) instead of 0)


def _lib():
    from lemon_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _noise01(seed, shape):
    return np.random.default_rng(seed).choice(np.array([0, 255], np.uint8), shape)


def _smooth(seed, shape):
    """[B, H, W, 3]: a ramp in both directions, another per channel and image, plus noise"""
    rng = np.random.default_rng(seed)
    B, H, W, _ = shape
    ramp = np.add.outer(np.arange(H) * 7, np.arange(W) * 11)[None, :, :, None] + np.arange(3) * 50 + np.arange(B)[:, None, None, None] * 23
    return ((ramp + rng.integers(0, 40, shape)) % 256).astype(np.uint8)


def _embed_u8(a, surround):
    """the bytes LEAD into a device buffer of `surround` -> (buffer, byte offset)"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1)
    host = np.full(LEAD + a.size + 256, surround, np.uint8)
    host[LEAD:LEAD + a.size] = a
    return torch.from_numpy(host).cuda(), LEAD


def _table_fill(n, bound, legal):
    """n ints of legal surround for a tap table (bound False) or a bound table (True), phase 0 at a table's first entry"""
    if not legal:
        return np.zeros(n, np.int32)
    return (np.arange(n) % 2).astype(np.int32) if bound else np.full(n, ONE, np.int32)


def _embed_table(t, bound, legal):
    t = np.ascontiguousarray(t, np.int32).reshape(-1)
    host = np.concatenate([_table_fill(T_LEAD, bound, legal), t, _table_fill(T_PAD + t.size % 2, bound, legal)[t.size % 2:]])
    return torch.from_numpy(host).cuda(), 4 * T_LEAD


# ---- expected buffers -------------------------------------------------------------------------------------------------------
def _expect(fs, P, operand):
    """the int32 words of the output owed for float32 [S, S, 3] results `fs` (one per batch position) + the canary tail"""
    if operand:
        body = PR.operand(np.concatenate([PR.patch_major(f, P) for f in fs]), OUT_FILL)
    else:
        body = np.concatenate([(PR.patch_major(f, P) if P else PR.nchw(f)).reshape(-1) for f in fs]).view(np.int32)
    return np.concatenate([body, np.full(TAIL, OUT_FILL, np.int32)])


def _same_words(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    n = len(want) - TAIL
    owed = want[:n] != OUT_FILL
    i = int(bad[0])
    where = "canary tail" if i >= n else ("a word owed" if owed[i] else "a word NOT owed (padding)")
    raise AssertionError(f"{what}: {len(bad)} of {len(want)} words differ; first at {i} ({where}): got {int(got[i]) & 0xFFFFFFFF:#010x}, "
                         f"want {int(want[i]) & 0xFFFFFFFF:#010x}; {int((bad >= n).sum())} in the tail")


def _out_words(B, S, P, operand):
    if operand:
        return (B * (S // P) ** 2 + TM - 1) // TM * TM * 3 * P * P
    return B * 3 * S * S


def _clip_coverage(refs, what):
    """the condition on the inputs: the reference clips on both sides in both passes"""
    for key in ("h_pre", "v_pre"):
        lo = sum(int((r[key] < 0).sum()) for r in refs)
        hi = sum(int((r[key] > 255).sum()) for r in refs)
        assert lo > 0 and hi > 0, (what, key, "the inputs do not reach the clip", lo, hi)


# ---- the same-shape kernel ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """images [B, H, W, 3], the two axes' tables, S and the reference of every image: computed once, never modified"""
    def mk(imgs, th, tv):
        refs = [PR.resample(im, th, tv) for im in imgs]
        for a in (imgs, *th, *tv):
            a.setflags(write=False)
        return dict(imgs=imgs, th=th, tv=tv, S=len(tv[1]), refs=refs, fs=[r["f"] for r in refs])
    kind, h, w, S, B = name
    seed = h * 100003 + w * 101 + S
    if kind == "up":                                   # h -> S and w -> S independently, {0, 255} noise
        return mk(_noise01(seed, (B, h, w, 3)), PR.axis_table(w, S, 0, S), PR.axis_table(h, S, 0, S))
    if kind == "smooth":
        return mk(_smooth(seed, (B, h, w, 3)), PR.axis_table(w, S, 0, S), PR.axis_table(h, S, 0, S))
    assert kind == "crop" and (h, w, S) == (40, 56, 12)
    return mk(_smooth(seed, (B, h, w, 3)), PR.axis_table(56, 42, 15, 12), PR.axis_table(40, 30, 9, 12))


def _call_same(c, R, P, surround, operand=False, B=None, **over):
    """one call of lemon_preprocess_u8 / _f16x3t on a poisoned output -> (return code, every word of the output buffer);
    `over`: max_rows, out_shift (bytes), null (a table's name): the arguments a refusal case changes"""
    lib = _lib().load()
    byte, legal = surround
    imgs, S = c["imgs"], c["S"]
    B = len(imgs) if B is None else B
    img, off = _embed_u8(imgs, byte)
    tabs = {}
    for name, t, bound in (("kk_h", c["th"][0], False), ("bnd_h", c["th"][1], True), ("kk_v", c["tv"][0], False), ("bnd_v", c["tv"][1], True)):
        buf, o = _embed_table(t, bound, legal)
        tabs[name] = None if over.get("null") == name else _p(buf, o)
        tabs[name + "_keep"] = buf
    ks_h, ks_v = c["th"][0].shape[1], c["tv"][0].shape[1]
    max_rows = over.get("max_rows", max(PR.block_spans(c["tv"][1], R)))
    n = _out_words(len(imgs), S, P, operand) if not over.get("words") else over["words"]
    out = _words(n + 4, OUT_FILL)                                      # (+ 4 words: room for a call that is shifted by 4 bytes)
    fn = lib.lemon_preprocess_u8_f16x3t if operand else lib.lemon_preprocess_u8
    rc = fn(_p(img, off), B, imgs.shape[1], imgs.shape[2], tabs["kk_h"], tabs["bnd_h"], ks_h, tabs["kk_v"], tabs["bnd_v"], ks_v, S,
            max_rows, R, MEAN, STD, P, _p(out, over.get("out_shift", 0)), _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:n + 4] == OUT_FILL), "write past the end"
    return rc, np.concatenate([got[:n], got[n + 4:]])


def _check_same(c, R, P, operand=False, what=""):
    want = _expect(c["fs"], P, operand)
    for s in SURROUNDS:
        rc, got = _call_same(c, R, P, s, operand)
        _lib().check(rc, "lemon_preprocess_u8")
        _same_words(got, want, f"{what} R={R} P={P} operand={operand} surround {s[0]:#04x}")


@pytest.mark.parametrize("R", [1, 2, 4, 5, 8, 16])
@pytest.mark.parametrize("S", [12, 10])
def test_every_row_block_geometry(hip, S, R):
    c = _case(("up", 5, 5, S, 3))
    _clip_coverage(c["refs"], f"5x5 -> {S}")
    _check_same(c, R, 0, what=f"5x5 -> {S}")


TAP_CASES = ([(("up", h, w, 8, 3), 16) for h in (1, 2, 3) for w in (1, 2, 3)] +
             [(("smooth", 8, 5, 8, 3), 16), (("smooth", 5, 8, 8, 3), 16), (("smooth", 8, 8, 8, 3), 16), (("smooth", 8, 8, 8, 3), 3),
              (("smooth", 508, 4, 4, 3), 1), (("smooth", 4, 508, 4, 3), 4), (("smooth", 4, 508, 4, 3), 1),
              (("crop", 40, 56, 12, 3), 16), (("crop", 40, 56, 12, 3), 5)])


@pytest.mark.parametrize("name,R", TAP_CASES, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else f"R{v}")
def test_tap_window_edges(hip, name, R):
    c = _case(name)
    kind, h, w, S, _ = name
    (kk_h, b_h), (kk_v, b_v) = c["th"], c["tv"]
    if kind == "up":                       # the windows are clipped at both ends: fewer taps than the table is wide
        assert kk_v.shape[1] == kk_h.shape[1] == 5 and b_v[:, 1].max() == h < 5 and b_h[:, 1].max() == w < 5
    if (h, w) == (508, 4):
        assert kk_v.shape[1] == 509 and R * (2 + 509) == 511 and kk_h.shape[1] == 1
    if (h, w) == (4, 508):
        assert kk_h.shape[1] == 509 and kk_v.shape[1] == 1
    if kind == "crop":
        assert b_v[:, 0].min() > 0 and b_h[:, 0].min() > 0 and kk_v.shape[1] > 5 and kk_h.shape[1] > 5
    _check_same(c, R, 0, what=str(name))


@pytest.mark.parametrize("h,w,S,P", [(5, 7, 12, 0), (5, 7, 12, 4), (5, 7, 12, 12), (5, 7, 12, 6), (5, 7, 12, 3),
                                     (5, 7, 10, 0), (5, 7, 10, 5), (5, 7, 10, 2), (9, 11, 28, 14)])
def test_every_output_layout_in_both_vertical_forms(hip, h, w, S, P):
    c = _case(("up", h, w, S, 3))
    _clip_coverage(c["refs"], f"{h}x{w} -> {S}")
    for R in (5, 16):
        _check_same(c, R, P, what=f"{h}x{w} -> {S}")


@pytest.mark.parametrize("S,P,B,R", [(12, 4, 3, 5), (12, 4, 15, 16), (16, 8, 9, 5)])
def test_operand_form_owes_its_rows_and_nothing_else(hip, S, P, B, R):
    """hi and lo planes = _split of the reference floats where _tiled_index puts them; the padding rows keep their poison"""
    c = _case(("up", 5, 7, S, B))
    _clip_coverage(c["refs"], f"5x7 -> {S}")
    rows, K = B * (S // P) ** 2, 3 * P * P
    want = _expect(c["fs"], P, True)
    assert len(want) - TAIL == (rows + TM - 1) // TM * TM * K
    assert int((want[:-TAIL] != OUT_FILL).sum()) == rows * K          # a word holds two halves of one row: rows K words are owed
    _check_same(c, R, P, operand=True, what=f"operand S={S} P={P} batch {B}")
    # ... and the float form of the same case, for the same bits before the split
    _check_same(c, R, P, what=f"patch-major S={S} P={P} batch {B}")


def test_same_shape_refusals_leave_the_output_untouched(hip):
    c = _case(("up", 5, 7, 12, 3))
    c10 = _case(("up", 5, 7, 10, 3))
    ident = _case(("smooth", 8, 8, 8, 3))
    s = SURROUNDS[0]
    cases = [("out misaligned by 4 bytes", c, dict(R=5, P=0, out_shift=4)),
             ("operand misaligned by 4 bytes", c, dict(R=5, P=4, operand=True, out_shift=4)),
             ("R (2 + ks_v) = 513", ident, dict(R=171, P=0)),
             ("R (2 + ks_v) = 518", c, dict(R=74, P=0)),
             ("max_rows S 3 > 56 KB", c, dict(R=5, P=0, max_rows=56 * 1024 // 36 + 1)),
             ("patch does not divide S", c, dict(R=5, P=5)),
             ("operand with P = 6", c, dict(R=5, P=6, operand=True, words=128 * 108)),
             ("operand with S = 10", c10, dict(R=5, P=2, operand=True, words=128 * 12)),
             ("operand with P = 0", c, dict(R=5, P=0, operand=True, words=128 * 48))]
    cases += [(f"null {t}", c, dict(R=5, P=4, operand=op, null=t)) for t in ("kk_h", "bnd_h", "kk_v", "bnd_v") for op in (False, True)]
    assert 171 * (2 + ident["tv"][0].shape[1]) == 513 and 73 * (2 + c["tv"][0].shape[1]) <= 512 < 74 * (2 + c["tv"][0].shape[1])
    assert (56 * 1024 // 36 + 1) * 36 > 56 * 1024 >= (56 * 1024 // 36) * 36
    for what, case, kw in cases:
        rc, got = _call_same(case, kw.pop("R"), kw.pop("P"), s, **kw)
        assert rc == E_INVALID, (what, rc)
        assert np.all(got == OUT_FILL), f"{what}: a refused call wrote to its output"
    # the bounds themselves are accepted: 511 ints at R = 73, 56 KB exactly is covered by the LDS limit's own arithmetic
    rc, got = _call_same(c, 73, 0, s)
    _lib().check(rc, "R = 73")
    _same_words(got, _expect(c["fs"], 0, False), "R = 73")
    for op in (False, True):
        rc, got = _call_same(c, 5, 4, s, operand=op, B=0)
        assert rc == 0 and np.all(got == OUT_FILL), ("batch 0", op, rc)


# ---- the ragged kernels -----------------------------------------------------------------------------------------------------
PL_INTS = 16


class _Ragged:
    """A ragged batch as lemon_preprocess_ragged reads it, built here: `shapes` the distinct (h, w) with their tables (th, tv),
    `imgs` with `plan_of` their plan indices.  Images lie at odd offsets in the packed buffer with `byte` between them; every
    table of the tap buffer has legal entries in front of it and behind it."""

    def __init__(self, imgs, tables, S, surround, extra_plans=()):
        byte, legal = surround
        self.S, self.imgs = S, imgs
        shapes = {}
        self.plan_of = [shapes.setdefault(im.shape[:2], len(shapes)) for im in imgs]
        taps, hdrs = [], []
        self.tabs = []
        for (h, w) in shapes:
            th, tv = tables(h, w)
            offs, base = [], sum(len(t) for t in taps)
            for t, bound in ((th[0], False), (th[1], True), (tv[0], False), (tv[1], True)):
                t = np.ascontiguousarray(t, np.int32).reshape(-1)
                lead, trail = _table_fill(8, bound, legal), _table_fill(8 + t.size % 2, bound, legal)[t.size % 2:]
                offs.append(base + len(lead))
                taps += [lead, t, trail]
                base += len(lead) + len(t) + len(trail)
            ks_v = tv[0].shape[1]
            R = min(16, 4096 // (2 + ks_v))
            vmin = int(tv[1][:, 0].min())
            rows = int(tv[1].sum(1).max()) - vmin
            hdr = np.zeros(PL_INTS, np.int32)
            hdr[:13] = (h, w, offs[0], offs[1], offs[2], offs[3], th[0].shape[1], ks_v, R, -(-S // R), vmin, rows, -(-rows // 16))
            hdrs.append(hdr)
            self.tabs.append((th, tv))
        for src, changes in extra_plans:               # copies of a plan with some header ints changed (the guard cases)
            hdr = hdrs[src].copy()
            for k, v in changes.items():
                hdr[k] = v
            hdrs.append(hdr)
        self.hdr = np.stack(hdrs)
        self.taps = torch.from_numpy(np.concatenate(taps)).cuda()
        self.plans = torch.from_numpy(self.hdr).cuda()
        desc, off, chunks = [], 0, []
        for im, pl in zip(imgs, self.plan_of):
            gap = LEAD if not desc else 3 - off % 2          # the next offset is odd
            chunks.append(np.full(gap, byte, np.uint8))
            off += gap
            assert off % 2 == 1
            desc.append((off, im.shape[0], im.shape[1], pl))
            chunks.append(np.ascontiguousarray(im).reshape(-1))
            off += im.size
        self.data_bytes = off
        chunks.append(np.full(256, byte, np.uint8))
        self.data = torch.from_numpy(np.concatenate(chunks)).cuda()
        self.desc = np.array(desc, np.int64)
        self.refs = [PR.resample(im, *self.tabs[pl]) for im, pl in zip(imgs, self.plan_of)]

    def call(self, P, operand, sel=None, desc=None, data_bytes=None, **over):
        """one call -> (return code, output words + tail, work bytes + tail, (ioff, rows) of the batch positions)"""
        lib = _lib().load()
        S = self.S
        desc = (self.desc if desc is None else desc)[list(range(len(self.desc))) if sel is None else sel]
        B = len(desc)
        ph = self.hdr[desc[:, 3]]
        rows = ph[:, 11].astype(np.int64)
        hpre = np.concatenate([[0], np.cumsum(ph[:, 12], dtype=np.int64)])
        vpre = np.concatenate([[0], np.cumsum(ph[:, 9], dtype=np.int64)])
        ioff = np.concatenate([[0], np.cumsum(rows * 3 * S)])
        aux = torch.from_numpy(np.concatenate([desc.ravel(), hpre, vpre, ioff[:-1], np.zeros(8, np.int64)]).astype(np.int64)).cuda()
        nwork = int(ioff[-1])
        assert nwork % 4 == 0
        work = torch.full((nwork + WORK_TAIL,), WORK_FILL, dtype=torch.uint8, device="cuda")
        n = over.get("words") or _out_words(B, S, P, operand)
        out = _words(n + 4, OUT_FILL)
        rc = lib.lemon_preprocess_ragged(None if over.get("null") == "data" else _p(self.data), self.data_bytes if data_bytes is None else data_bytes,
                                         over.get("batch", B), _p(aux), int(hpre[-1]), over.get("v_blocks", int(vpre[-1])),
                                         None if over.get("null") == "plans" else _p(self.plans), None if over.get("null") == "taps" else _p(self.taps),
                                         _p(work, over.get("work_shift", 0)), S, MEAN, STD, P, int(operand), _p(out, over.get("out_shift", 0)), _stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[n:n + 4] == OUT_FILL), "write past the end"
        return rc, np.concatenate([got[:n], got[n + 4:]]), work.cpu().numpy(), (ioff, rows)

    def expect_work(self, sel, ioff, rows, skip=()):
        want = np.full(int(ioff[-1]) + WORK_TAIL, WORK_FILL, np.uint8)
        for pos, i in enumerate(sel):
            if pos in skip:
                continue
            vmin = int(self.hdr[self.plan_of[i], 10])
            want[ioff[pos]:ioff[pos + 1]] = self.refs[i]["h"][vmin:vmin + int(rows[pos])].reshape(-1)
        return want


def _same_bytes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} work bytes differ; first at {int(bad[0])}: got {int(got[bad[0]])}, "
                             f"want {int(want[bad[0]])}; {int((bad >= len(want) - WORK_TAIL).sum())} in the tail")


def _ragged_images(S):
    shapes = [(1, 1), (3, 2), (5, 7), (5, 7), (S, S), (64, 48), (40, 90)]
    return [(_noise01 if h * w < 100 else _smooth)(1000 * S + 10 * i + h, (1, h, w, 3))[0] for i, (h, w) in enumerate(shapes)]


FORMS = {20: [(0, False), (4, False), (5, False), (4, True)], 18: [(0, False), (6, False), (9, False)]}


@pytest.mark.parametrize("S", [20, 18])
def test_ragged_launch_in_every_output_form(hip, S):
    imgs = _ragged_images(S)
    for s in SURROUNDS:
        r = _Ragged(imgs, lambda h, w: PR.transform_tables(h, w, S), S, s)
        # what the shapes are for: a shared plan, the identity, several vertical blocks with a tail, horizontal blocks with a tail
        assert r.plan_of[2] == r.plan_of[3] and len(r.hdr) == 6
        assert tuple(r.hdr[r.plan_of[4], 6:8]) == (1, 1) and np.all(r.hdr[:, 8] == 16) and np.all(r.hdr[:, 9] == 2) and S % 16
        assert r.hdr[r.plan_of[5], 12] >= 3 and r.hdr[r.plan_of[5], 11] % 16 and r.hdr[r.plan_of[6], 12] >= 3 and r.hdr[r.plan_of[6], 11] % 16
        assert all(int(d[0]) % 2 == 1 for d in r.desc)
        for P, operand in FORMS[S]:
            what = f"ragged S={S} P={P} operand={operand} surround {s[0]:#04x}"
            rc, got, work, (ioff, rows) = r.call(P, operand)
            _lib().check(rc, what)
            _same_words(got, _expect([x["f"] for x in r.refs], P, operand), what)
            _same_bytes(work, r.expect_work(range(len(imgs)), ioff, rows), what)
    # the same bits as the same-shape reference of generic_transform
    assert np.array_equal(PR.nchw(r.refs[6]["f"]), PR.generic_transform(imgs[6], S))


def test_ragged_4093_vertical_taps(hip):
    """a hand-built plan: 4092 -> 4 vertically (R = 1: 4095 of the window table's 4096 ints), the identity horizontally"""
    S = 4
    imgs = list(_smooth(7, (3, 4092, 4, 3)))
    tables = lambda h, w: (PR.axis_table(4, 4, 0, 4), PR.axis_table(4092, 4, 0, 4))
    for s in SURROUNDS:
        r = _Ragged(imgs, tables, S, s)
        assert len(r.hdr) == 1 and tuple(r.hdr[0, 6:10]) == (1, 4093, 1, 4) and 1 * (2 + 4093) == 4095
        for P, operand in [(0, False), (2, False), (4, True)]:
            what = f"4092x4 P={P} operand={operand} surround {s[0]:#04x}"
            rc, got, work, (ioff, rows) = r.call(P, operand)
            _lib().check(rc, what)
            _same_words(got, _expect([x["f"] for x in r.refs], P, operand), what)
            _same_bytes(work, r.expect_work(range(3), ioff, rows), what)


def test_ragged_permuted_sub_batch_with_a_repeat(hip):
    S, sel = 20, [4, 1, 1, 6, 0]
    r = _Ragged(_ragged_images(S), lambda h, w: PR.transform_tables(h, w, S), S, SURROUNDS[1])
    for P, operand in FORMS[S]:
        rc, got, work, (ioff, rows) = r.call(P, operand, sel=sel)
        _lib().check(rc, "sub-batch")
        _same_words(got, _expect([r.refs[i]["f"] for i in sel], P, operand), f"sub-batch P={P} operand={operand}")
        _same_bytes(work, r.expect_work(sel, ioff, rows), "sub-batch")


GUARD_FORMS = [(0, False), (5, False), (4, True)]          # NCHW (4-pixel form), patches (1-pixel form), the operand


@pytest.mark.parametrize("bad", ["plan H", "plan W", "another plan", "negative offset", "beyond data_bytes", "rows beyond H", "R = 0"])
def test_ragged_guard_makes_one_image_nan_and_leaves_the_rest(hip, bad):
    """Every way ragged_ok refuses an image.  Nothing here can reach unmapped memory: the refused image is never read, the
    plan index stays valid, data_bytes shrinks while the allocation does not, and `work` has room for the rows the bad plan
    names."""
    S = 20
    shapes = [(3, 2), (5, 7), (40, 90), (5, 7), (64, 48)]
    imgs = [_smooth(50 + i, (1, h, w, 3))[0] for i, (h, w) in enumerate(shapes)]
    victim = 4 if bad == "beyond data_bytes" else 2
    for s in SURROUNDS:
        # plans 0..3 are the shapes'; 4 and 5 copy the victim's with one header int wrong
        h_v = shapes[victim][0]
        r0 = _Ragged(imgs, lambda h, w: PR.transform_tables(h, w, S), S, s)
        pv = r0.plan_of[victim]
        vmin, rows = int(r0.hdr[pv, 10]), int(r0.hdr[pv, 11])
        r = _Ragged(imgs, lambda h, w: PR.transform_tables(h, w, S), S, s,
                    extra_plans=[(pv, {11: h_v - vmin + 1, 12: -(-(h_v - vmin + 1) // 16)}), (pv, {8: 0})])
        assert len(r.hdr) == 6 and vmin + rows <= h_v
        desc, data_bytes = r.desc.copy(), r.data_bytes
        if bad == "plan H":
            desc[victim, 1] += 1
        elif bad == "plan W":
            desc[victim, 2] -= 1
        elif bad == "another plan":
            desc[victim, 3] = r.plan_of[0]
        elif bad == "negative offset":
            desc[victim, 0] = -7
        elif bad == "beyond data_bytes":
            assert desc[victim, 0] + imgs[victim].size == data_bytes and r.data.numel() > data_bytes
            data_bytes -= 1
        elif bad == "rows beyond H":
            desc[victim, 3] = 4
        else:
            desc[victim, 3] = 5
        for P, operand in GUARD_FORMS:
            what = f"guard {bad} P={P} operand={operand} surround {s[0]:#04x}"
            rc0, good, _, _ = r.call(P, operand)
            _lib().check(rc0, what)
            fs = [x["f"] for x in r.refs]
            _same_words(good, _expect(fs, P, operand), what + " (unbroken)")
            rc, got, work, (ioff, rows_) = r.call(P, operand, desc=desc, data_bytes=data_bytes)
            _lib().check(rc, what)
            # the words owed to the victim: those that change with its values (hi words and lo words both differ)
            a, b = list(fs), list(fs)
            a[victim], b[victim] = np.full((S, S, 3), 1.0, np.float32), np.full((S, S, 3), 2.0 + 2.0 ** -12, np.float32)
            mine = _expect(a, P, operand) != _expect(b, P, operand)
            assert int(mine.sum()) == 3 * S * S and not mine[-TAIL:].any()
            assert np.array_equal(got[~mine], good[~mine]), what + ": another image, a padding word or the tail changed"
            owed = got[mine]
            nan = np.isnan(owed.view(np.float16)).reshape(-1, 2).all(1) if operand else np.isnan(owed.view(np.float32))
            assert nan.all(), f"{what}: {int((~nan).sum())} of {len(nan)} words owed to the refused image are not NaN"
            _same_bytes(work, r.expect_work(range(5), ioff, rows_, skip={victim}), what)


def test_ragged_refusals_leave_output_and_work_untouched(hip):
    S = 20
    r = _Ragged(_ragged_images(S), lambda h, w: PR.transform_tables(h, w, S), S, SURROUNDS[0])
    r18 = _Ragged(_ragged_images(18), lambda h, w: PR.transform_tables(h, w, 18), 18, SURROUNDS[0])
    cases = [("out misaligned by 4 bytes", r, dict(P=0, operand=False, out_shift=4)),
             ("operand misaligned by 4 bytes", r, dict(P=4, operand=True, out_shift=4)),
             ("work misaligned", r, dict(P=0, operand=False, work_shift=1)),
             ("work misaligned by 2", r, dict(P=4, operand=True, work_shift=2)),
             ("patch does not divide S", r, dict(P=6, operand=False)),
             ("operand with P = 5", r, dict(P=5, operand=True, words=128 * 75)),
             ("operand with P = 6", r18, dict(P=6, operand=True, words=128 * 108)),
             ("operand with S = 18", r18, dict(P=2, operand=True, words=128 * 12 * 5)),
             ("operand with P = 0", r, dict(P=0, operand=True, words=128 * 48)),
             ("v_blocks < batch", r, dict(P=0, operand=False, v_blocks=6)),
             ("null data", r, dict(P=0, operand=False, null="data")),
             ("null plans", r, dict(P=4, operand=True, null="plans")),
             ("null taps", r, dict(P=4, operand=False, null="taps"))]
    for what, rr, kw in cases:
        rc, got, work, _ = rr.call(kw.pop("P"), kw.pop("operand"), **kw)
        assert rc == E_INVALID, (what, rc)
        assert np.all(got == OUT_FILL) and np.all(work == WORK_FILL), f"{what}: a refused call wrote"
    for P, operand in FORMS[S]:
        rc, got, work, _ = r.call(P, operand, batch=0)
        assert rc == 0 and np.all(got == OUT_FILL) and np.all(work == WORK_FILL), ("batch 0", P, operand, rc)
