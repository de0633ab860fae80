"""Records what the JPEG host passes say about a table of small files and their mutants: tests/golden/jpeg_verdicts.npz, which
tests/test_jpeg_verdicts_host.py replays.  The fixture holds the base files' bytes (PIL's encoder may differ between machines,
so they are not regenerated), every mutant as explicit (offset, kind, value) steps, and for every case and every entry point of
lemon_amd/jpeg_host.py the status, the Info fields and a SHA-256 of the packet or record written with status 0
(tests/jpegverdictfx.py), plus the looped-device statuses of packets with a tampered Huffman specification.

Run it BEFORE a change to lemon_amd/csrc/jpeg* that must not move a verdict, never after:
  python tools/make_golden_jpeg.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import jpegfx, jpegprogfx                                       # noqa: E402
from tests import jpegverdictfx as fx                                      # noqa: E402

N_SCAN, N_HEADER = 110, 60


def base_files(seed=20261019):
    from PIL import Image
    rng = np.random.default_rng(seed)
    px = jpegfx.pixels
    exif = Image.Exif()
    exif[0x010E] = "x" * 300
    specs = [("17x24_420", px(17, 24, rng), dict(quality=75, subsampling=2)),
             ("37x53_444", px(37, 53, rng), dict(quality=90, subsampling=0)),
             ("gray_41x67", px(41, 67, rng, channels=1), dict(quality=90)),
             ("gray_1x1", px(1, 1, rng, noise=True, channels=1).reshape(1, 1), dict(quality=75)),
             ("rst_blocks1", px(100, 75, rng), dict(quality=50, subsampling=0, restart_marker_blocks=1)),
             ("rst_blocks3", px(100, 75, rng), dict(quality=85, subsampling=2, restart_marker_blocks=3)),
             ("rst_rows", px(100, 75, rng), dict(quality=85, subsampling=1, restart_marker_rows=1)),
             ("optimize", px(37, 53, rng, noise=True), dict(quality=95, subsampling=0, optimize=True)),
             ("exif_com", px(33, 21, rng), dict(quality=90, subsampling=2, exif=exif, comment=b"c" * 300))]
    out = []
    for prog in (False, True):
        for name, pixels, kw in specs:
            out.append((("prog_" if prog else "base_") + name, jpegfx.jpeg_bytes(pixels, progressive=prog, **kw)))
    return out


def segments(raw):
    """[(marker, first payload byte, end)] of every marker segment of a file PIL wrote, and [(first, end)] of its scans' bytes."""
    segs, scans, p = [], [], 2
    while raw[p + 1] != 0xD9:
        assert raw[p] == 0xFF, p
        n = (raw[p + 2] << 8) | raw[p + 3]
        segs.append((raw[p + 1], p + 4, p + 2 + n))
        q = p + 2 + n
        if raw[p + 1] == 0xDA:
            while not (raw[q] == 0xFF and raw[q + 1] != 0 and not 0xD0 <= raw[q + 1] <= 0xD7):
                q += 1
            scans.append((p + 2 + n, q))
        p = q
    return segs, scans


def scan_mutants(raw, rng, n):
    """As tests/test_jpeg_entropy_par.py::mutants: one to three steps inside the entropy-coded bytes."""
    _, scans = segments(raw)
    lo, hi = scans[0][0], scans[-1][1]
    out = []
    for _ in range(n):
        ops, size = [], len(raw)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(lo, max(lo + 1, min(hi, size))))
            kind = int(rng.integers(0, 4))
            if at >= size:                                              # (an earlier step cut the file in front of it)
                continue
            if kind == 0:
                ops.append((at, fx.XOR, 1 << int(rng.integers(0, 8))))
            elif kind == 1:
                ops.append((at, fx.DEL, 0))
                size -= 1
            elif kind == 2:
                eoi = int(rng.integers(0, 2))
                ops.append((at, fx.CUT, eoi))
                size = at + 2 * eoi
            else:
                ops.append((at, fx.INS_MARKER, int(rng.choice([0xD0 + int(rng.integers(0, 8)), 0xD9, 0xFF, 0x00, 0xC4, 0xDA]))))
                size += 2
        out.append(ops)
    return out


def header_mutants(raw, rng, n):
    """Targeted and random steps inside the DHT, DQT, DRI, SOF and SOS segments (length bytes included)."""
    segs, _ = segments(raw)
    out = []
    for m, a, b in segs:
        if m == 0xC4:                                                   # every table of the segment: counts and values
            o = a
            while o < b:
                total = sum(raw[o + 1:o + 17])
                first = next(l for l in range(16) if raw[o + 1 + l])
                out += [[(o + 1, fx.SET, 3)], [(o + 1 + first, fx.SET, raw[o + 1 + first] + 1)], [(o + 15, fx.SET, 255), (o + 16, fx.SET, 255)],
                        [(o + 16, fx.SET, 200)], [(o, fx.SET, raw[o] | 0x04)], [(o, fx.SET, 0x20)], [(o + 17, fx.SET, 12)],
                        [(o + 17, fx.SET, 0xF1)], [(o + 17 + total - 1, fx.XOR, 0x0F)], [(o + 2, fx.SET, 5)]]
                o += 17 + total
        elif m == 0xDB:
            out += [[(a, fx.SET, 0x10)], [(a, fx.SET, 0x04)], [(a + 1, fx.SET, 255)], [(a + 64, fx.SET, 0)], [(a - 1, fx.XOR, 1)]]
        elif m == 0xDD:
            out += [[(a + 1, fx.SET, v)] for v in (0, 1, 2, 7, 255)] + [[(a - 1, fx.SET, 3)], [(a, fx.SET, 1)]]
        elif m in (0xC0, 0xC2):
            nc = raw[a + 5]
            out += [[(a, fx.SET, 12)], [(a + 2, fx.SET, 0)], [(a + 1, fx.SET, 1)], [(a + 3, fx.SET, 2)], [(a + 4, fx.SET, 0)],
                    [(a + 5, fx.SET, 2)], [(a + 5, fx.SET, 4)], [(a + 7, fx.SET, 0x22)], [(a + 7, fx.SET, 0x41)], [(a + 7, fx.SET, 0x12)],
                    [(a + 8, fx.SET, 4)], [(a + 8, fx.SET, 1)], [(a + 6, fx.SET, 9)], [(a - 3, fx.SET, 0xC1)], [(a - 3, fx.SET, 0xC9)]]
            if nc == 3:
                out += [[(a + 10, fx.SET, 0x21)], [(a + 9, fx.SET, 7)], [(a + 14, fx.SET, 3)]]
        elif m == 0xDA:
            ns = raw[a]
            out += [[(a, fx.SET, 2)], [(a + 1, fx.SET, 9)], [(a + 2, fx.SET, 0x22)], [(a + 2, fx.SET, 0x40)], [(a + 1 + 2 * ns, fx.SET, 1)],
                    [(a + 2 + 2 * ns, fx.SET, 62)], [(a + 3 + 2 * ns, fx.SET, 0x10)], [(a - 1, fx.SET, 9)]]
    out.append([(2, fx.INS_MARKER, 0xD0)])
    out.append([(2, fx.INS_MARKER, 0xD8)])
    out.append([(2, fx.INS_BYTE, 0)])
    out.append([(0, fx.SET, 0x89)])
    spans = [(a - 2, b) for m, a, b in segs if m in (0xC4, 0xDB, 0xDD, 0xC0, 0xC2, 0xDA)]
    big = {a + k for m, a, b in segs if m in (0xC0, 0xC2) for k in (1, 3)}     # high bytes of the dimensions: records of 10s of MB
    while n > 0:
        a, b = spans[int(rng.integers(0, len(spans)))]
        at = int(rng.integers(a, b))
        if at in big:
            continue
        n -= 1
        out.append([(at, fx.XOR, 1 << int(rng.integers(0, 8)))] if rng.integers(0, 2) else [(at, fx.SET, int(rng.integers(0, 256)))])
    return out


def sos_mutants(raw):
    """jpegprogfx.patched_sos and cut_after_scans as steps (checked against those functions)."""
    sos = jpegprogfx.sos_offsets(raw)
    out = []
    for s in range(len(sos)):
        for kw in (dict(ah=1), dict(al=14), dict(al=0), dict(al=1), dict(ss=6, se=5), dict(se=64), dict(se=5), dict(ss=1), dict(ss=0, se=0)):
            want = jpegprogfx.patched_sos(raw, s, **kw)
            ops = [(i, fx.SET, want[i]) for i in range(len(raw)) if want[i] != raw[i]]
            if ops:
                out.append(ops)
        at = sos[s]
        if raw[at + 4] == 1:
            ops = [(at + 3, fx.SET, 12), (at + 4, fx.SET, 3), (at + 5, fx.SET, 1), (at + 7, fx.INS_BYTE, 2), (at + 8, fx.INS_BYTE, 0x11),
                   (at + 9, fx.INS_BYTE, 3), (at + 10, fx.INS_BYTE, 0x11)]
            assert fx.apply(raw, ops) == jpegprogfx.patched_sos(raw, s, ns3=True)
            out.append(ops)
        if s:
            want = jpegprogfx.cut_after_scans(raw, s)
            ops = [(len(want) - 2, fx.CUT, 1)]
            assert fx.apply(raw, ops) == want
            out.append(ops)
    return out


def main():
    from lemon_amd import jpeg_host
    rng = np.random.default_rng(20261019)
    bases = base_files()
    cases = []                                                          # (base index, steps)
    for b, (name, raw) in enumerate(bases):
        cases.append((b, []))
        cases += [(b, ops) for ops in scan_mutants(raw, rng, N_SCAN) + header_mutants(raw, rng, N_HEADER)]
        if name.startswith("prog_"):
            cases += [(b, ops) for ops in sos_mutants(raw)]
    M, E, F = len(cases), len(fx.ENTRY_POINTS), len(fx.INFO_FIELDS)
    mut_ops = np.full((M, fx.MAX_OPS, 3), -1, np.int32)
    status = np.zeros((M, E), np.int8)
    info = np.zeros((M, E, F), np.int64)
    digest_idx = np.full((M, E), -1, np.int32)
    digests, native = {}, []
    for k, (b, ops) in enumerate(cases):
        assert len(ops) <= fx.MAX_OPS
        if ops:
            mut_ops[k, :len(ops)] = ops
        st, fields, dg = fx.evaluate(fx.apply(bases[b][1], ops))
        status[k], info[k] = st, fields
        for e, d in enumerate(dg):
            if d is not None:
                digest_idx[k, e] = digests.setdefault(d, len(digests))
        native.append(st[fx.ENTRY_POINTS.index("prog_entropy" if bases[b][0].startswith("prog_") else "entropy")])
    for b in range(len(bases)):                                         # every base file is accepted by its own passes
        k = next(i for i, c in enumerate(cases) if c == (b, []))
        assert native[k] == 0, (bases[b][0], native[k])
    # the table is not trivial: counted on the whole host pass of each case's own process (entropy / prog_entropy)
    count = np.bincount(np.asarray(native), minlength=18)
    print("cases", M, "statuses of the whole host pass", {s: int(c) for s, c in enumerate(count) if c})
    assert all(count[s] >= 20 for s in (0, 8, 10, 11)), count
    assert all(count[s] >= 1 for s in (9, 15, 17)), count
    assert count.max() <= 0.7 * M, count
    tamper_names, tamper_status = [], []
    for name, raw in bases:
        if name in fx.TAMPER_BASES:
            for tname, pk in fx.tampered_packets(name, raw):
                tamper_names.append(tname)
                tamper_status.append(fx.tampered_status(tname, pk, jpeg_host.info(raw, progressive=True).record_bytes)[0])
    print("tampered packets", dict(zip(tamper_names, tamper_status)))
    dg = np.zeros((len(digests), 32), np.uint8)
    for d, i in digests.items():
        dg[i] = np.frombuffer(d, np.uint8)
    off = np.cumsum([0] + [len(r) for _, r in bases]).astype(np.int64)
    np.savez_compressed(fx.GOLDEN, base_names=np.array([n for n, _ in bases]), base_off=off,
                        base_bytes=np.frombuffer(b"".join(r for _, r in bases), np.uint8), entry_points=np.array(fx.ENTRY_POINTS),
                        info_fields=np.array(fx.INFO_FIELDS), mut_base=np.array([b for b, _ in cases], np.int16), mut_ops=mut_ops,
                        status=status, info=info, digest_idx=digest_idx, digests=dg, tamper_names=np.array(tamper_names),
                        tamper_status=np.array(tamper_status, np.int32))
    print(fx.GOLDEN, os.path.getsize(fx.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
