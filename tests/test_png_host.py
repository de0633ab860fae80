"""CPU: the workers' half of the PNG decode (csrc/png_core.hpp's chunk walk in liblemon_jpeg_host.so, lemon_amd/png_host.py's
inflate) and the device schedule looped on the host (lemon_png_decode_host): bit-equality with PIL on files written filter by
filter (tests/pngfx.py), every decline status, the two device verdicts, the mimiccxr path rule, the LEMON_PNG knob, the batch
layout, and the decode pool delivering records."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import pngfx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def accepted():
    return pngfx.accepted_cases()


def test_writer_files_read_back_through_pil_as_convert_rgb():
    # the fixture itself: all five filters cycling, every colour type -> grey-replicate, RGB, alpha-drop, palette-lookup
    rng = np.random.default_rng(5)
    for ct in pngfx.COLOUR_TYPES:
        plte = pngfx.palette(7, rng) if ct == 3 else None
        pix = pngfx.pixels(23, 19, ct, rng, plte_count=7)
        raw = pngfx.png_bytes(pix, ct, plte=plte)
        assert np.array_equal(pngfx.pil_rgb(raw), pngfx.expected_rgb(pix, ct, plte)), ct


def test_inflate_plus_looped_device_schedule_equal_pil_bit_for_bit(accepted):
    from lemon_amd import png_host
    names = [c[0] for c in accepted]
    assert len(accepted) >= 110 and {f"ct{ct}_f{ft}" for ct in pngfx.COLOUR_TYPES for ft in range(5)} <= set(names)
    assert {f"w{w}_h{h}" for w in pngfx.WIDTHS for h in pngfx.HEIGHTS} == {n.rsplit("_", 1)[0] for n in names if n.startswith("w")}
    for name, raw in accepted:
        rec, info = png_host.decode_record(raw)
        assert rec is not None, (name, info.status, png_host.STATUS.get(info.status))        # none of these may be declined
        ref = pngfx.pil_rgb(raw)
        assert (rec.h, rec.w) == ref.shape[:2], name
        assert info.stride == rec.w * rec.channels and info.record_bytes == 1024 + rec.h * (info.stride + 1) == rec.data.size, name
        got, status = png_host.decode_host(rec)
        assert status == 0, (name, status)
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_record_holds_the_palette_and_the_scanlines_as_inflated():
    from lemon_amd import png_host
    rng = np.random.default_rng(6)
    plte = pngfx.palette(5, rng)
    pix = pngfx.pixels(6, 9, 3, rng, plte_count=5)
    filters = [4, 3, 2, 1, 0, 3]
    raw = pngfx.png_bytes(pix, 3, filters, plte=plte, splits=3)
    rec, info = png_host.decode_record(raw)
    assert (info.plte_count, info.idat_spans > 1, info.channels, info.colour_type) == (5, True, 1, 3)
    pal = rec.data[:1024].reshape(256, 4)
    assert np.array_equal(pal[:5, :3], plte) and not pal[5:].any() and not pal[:, 3].any()
    assert rec.data[1024:].tobytes() == pngfx.filter_rows(pix, filters)
    grey, _ = png_host.decode_record(pngfx.png_bytes(pngfx.pixels(4, 4, 0, rng), 0))
    assert not grey.data[:1024].any()
    # a record buffer that is too small is refused, not overrun
    small = np.zeros(100, np.uint8)
    none, info = png_host.decode_record(raw, small)
    assert none is None and info.status == png_host.BUFFER and not small.any()


PIL_RAISES = {"adam7", "crc_ihdr", "idat_split_by_chunk", "stream_short", "truncated", "zero_width", "not_png"}


def test_each_defect_is_declined_with_its_own_status():
    from lemon_amd import png_host
    cases = pngfx.declined_cases()
    names = {c[0] for c in cases}
    assert {"depth16", "depth1", "depth2", "depth4", "adam7", "crc_ihdr", "crc_idat", "crc_iend", "plte_missing", "plte_after_idat",
            "idat_split_by_chunk", "actl", "stream_short", "stream_long", "stream_garbage", "truncated", "zero_width"} <= names
    for name, raw, want in cases:
        rec, info = png_host.decode_record(raw)
        assert rec is None and info.status == want, (name, info.status, want)
        head = png_host.info(raw)
        assert head.status == (0 if want == png_host.STREAM else want), (name, head.status)   # STREAM is the inflate step's verdict
        if name in PIL_RAISES:
            with pytest.raises(Exception):
                pngfx.pil_rgb(raw)
    # the header statuses the list above does not reach
    rng = np.random.default_rng(7)
    g = pngfx.pixels(5, 5, 0, rng)
    for kw, want in ((dict(header=dict(depth=3)), png_host.HEADER), (dict(header=dict(compression=1)), png_host.HEADER),
                     (dict(header=dict(interlace=2)), png_host.HEADER), (dict(header=dict(h=0)), png_host.DIMENSION),
                     (dict(header=dict(w=70000)), png_host.DIMENSION), (dict(header=dict(w=20000, h=20000)), png_host.DIMENSION),
                     (dict(plte=np.zeros((2, 3), np.uint8)), png_host.PALETTE), (dict(before_idat=[(b"ABCD", b"")]), png_host.HEADER),
                     (dict(before_idat=[(b"IHDR", b"\0" * 13)]), png_host.CHUNK_ORDER)):
        assert png_host.info(pngfx.png_bytes(g, 0, **kw)).status == want, kw
    assert png_host.info(pngfx.png_bytes(pngfx.pixels(5, 5, 3, rng), 3, plte=np.zeros((257, 3), np.uint8))).status == png_host.PALETTE
    assert png_host.info(b"").status == png_host.NOT_PNG and png_host.info(pngfx.SIGNATURE[:5]).status == png_host.TRUNCATED
    assert png_host.info(pngfx.SIGNATURE).status == png_host.TRUNCATED


def test_device_verdicts_filter_byte_above_4_and_index_beyond_plte():
    from lemon_amd import png_host
    rng = np.random.default_rng(8)
    rgb = pngfx.pixels(70, 9, 2, rng)
    for row in (0, 3, 64, 69):
        filters = [r % 5 for r in range(70)]
        filters[row] = 5
        raw = pngfx.png_bytes(rgb, 2, filters)
        rec, info = png_host.decode_record(raw)
        assert rec is not None                       # the host does not look inside the scanlines
        assert png_host.decode_host(rec)[1] == png_host.FILTER == 13, row
        with pytest.raises(OSError):
            pngfx.pil_rgb(raw)
    plte = pngfx.palette(4, rng)
    idx = pngfx.pixels(66, 11, 3, rng, plte_count=4)
    rec, _ = png_host.decode_record(pngfx.png_bytes(idx, 3, plte=plte))
    got, st = png_host.decode_host(rec)
    assert st == 0 and np.array_equal(got, plte[idx[:, :, 0]])
    for at in ((0, 0), (65, 10), (64, 3)):
        bad = idx.copy()
        bad[at] = 4
        rec, _ = png_host.decode_record(pngfx.png_bytes(bad, 3, plte=plte))
        assert png_host.decode_host(rec)[1] == png_host.INDEX == 14, at
    # bad arguments are refused before anything is read
    with pytest.raises(ValueError):
        png_host.decode_host(rec._replace(h=rec.h + 1))
    with pytest.raises(ValueError):
        png_host.decode_host(rec._replace(colour_type=1))


def test_both_libraries_export_the_same_parser_and_the_host_library_links_no_hip(accepted):
    from lemon_amd import _lib, png_host
    hip = ctypes.CDLL(_lib.SO_PATH)
    hip.lemon_png_info.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(png_host.Info)]
    for name, raw in accepted[::7] + [(c[0], c[1]) for c in pngfx.declined_cases()]:
        a, b = png_host.info(raw), png_host.Info()
        hip.lemon_png_info(raw, len(raw), ctypes.byref(b))
        assert bytes(a) == bytes(b), name
    out = subprocess.run(["ldd", png_host.SO_PATH], capture_output=True, text=True).stdout
    assert "amdhip" not in out and "hsa" not in out and "torch" not in out and "libz" not in out, out


def test_mimic_image_path_rule_and_the_dataset_hands_out_the_png_paths(tmp_path):
    import pandas as pd
    from lemon_amd.data import get_dataset, mimic_image_path
    root = str(tmp_path / "mimic")
    rel = ["files/p10/p1000/s500/a.jpg", "files/p10/p1000/s501/b.jpg", "files/p11/p1100/s502/c.jpg"]
    for r in rel:
        os.makedirs(os.path.dirname(os.path.join(root, r)), exist_ok=True)
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(root, r))
    small = os.path.join(root, "downsampled_files/p10/p1000/s500/a.png")
    os.makedirs(os.path.dirname(small))
    Image.fromarray(np.zeros((4, 4), np.uint8)).save(small)
    assert mimic_image_path(os.path.join(root, rel[0])) == small                      # PNG present: the PNG
    assert mimic_image_path(os.path.join(root, rel[1])) == os.path.join(root, rel[1])  # absent: the original path
    assert mimic_image_path("a.jpg") == "a.jpg"                                        # fewer than five components
    n = 30
    df = pd.DataFrame({"path": [os.path.join(root, rel[i % 3]) for i in range(n)], "sentence": [f"finding {i}" for i in range(n)],
                       "gold_sentence": [f"finding {i}" for i in range(n)], "split": ["train", "val", "test"] * (n // 3),
                       "cat_labels": [[i % 4] for i in range(n)], "nouns_int": [[i % 5] for i in range(n)]})
    df.to_pickle(os.path.join(root, "multimodal_mislabel_split.pkl"))
    sets = get_dataset("mimiccxr_caption", 0, flip_type="random", data_root=root)
    seen = [p for s in sets for p in s.images]
    assert len(seen) == n and seen.count(small) == n // 3 and not any(p.endswith("a.jpg") for p in seen)
    assert seen.count(os.path.join(root, rel[1])) == n // 3
    # every other dataset keeps the frame's paths
    other = [p for s in get_dataset("mscoco", 0, flip_type="random", data_root=root) for p in s.images]
    assert small not in other and other.count(os.path.join(root, rel[0])) == n // 3


def test_lemon_png_knob(monkeypatch):
    from lemon_amd import loader
    monkeypatch.delenv("LEMON_PNG", raising=False)
    assert loader.png_default() is False
    for v, want in (("pil", False), ("gpu", True), ("GPU", True)):
        monkeypatch.setenv("LEMON_PNG", v)
        assert loader.png_default() is want
    monkeypatch.setenv("LEMON_PNG", "bogus")
    with pytest.raises(ValueError, match="LEMON_PNG"):
        loader.png_default()


def test_layout_png_records_follow_an_unchanged_jpeg_layout():
    from lemon_amd import jpeg_host, png_host
    from tests import jpegfx
    rec, _ = jpeg_host.decode_record(jpegfx.accepted_cases()[3][1])
    png, _ = png_host.decode_record(pngfx.accepted_cases()[2][1])

    def build(with_png):
        lay, off = jpeg_host.BatchLayout(), 0
        lay.add_pixels(off, 5, 7)
        off = (off + 105 + 15) & ~15
        lay.add_record(off, rec)
        off = (off + rec.data.nbytes + 15) & ~15
        if with_png:
            lay.add_png_record(off, png)
            off = (off + png.data.nbytes + 15) & ~15
        return lay, lay.finish(off), off

    a, aux_a, _ = build(False)
    b, aux_b, off_b = build(True)
    assert a.n_png == 0 and b.n_png == 1 and a.n_jpeg == b.n_jpeg == 1
    assert np.array_equal(aux_b[:aux_a.size][[0, 2, 3, 4, 5, 6, 7]], aux_a[[0, 2, 3, 4, 5, 6, 7]])     # (all but the pixels' offset)
    assert b.png_aux_off % 16 == 0 and b.payload_bytes == b.png_aux_off + 64 and (b.payload_bytes - b.aux_off) == 8 * aux_b.size
    row = aux_b[-8:]
    assert list(row[:5]) == [b.png_records[0][1], png.h, png.w, png.colour_type, png.plte_count] and row[1] == png.h
    assert row[5] == b.desc[2][0] >= b.png_decoded_off >= b.payload_bytes and row[5] % 16 == 0 and row[6] == 0 and row[7] == 0
    assert b.total_bytes >= row[5] + png.h * png.w * 3 and b.png_work_bytes >= png_host.work_bytes_of(png.w)
    # a JPEG-only batch: nothing of it changes (same aux table, same sizes, no PNG fields in the payload)
    c, aux_c, _ = build(False)
    assert np.array_equal(aux_a, aux_c) and a.payload_bytes == a.aux_off + a.aux_bytes() and a.total_bytes == c.total_bytes


def test_pool_with_png_delivers_records_and_declined_files_come_as_pil_pixels(tmp_path):
    from lemon_amd import png_host
    from lemon_amd.loader import DecodeError, DecodePool
    good = pngfx.accepted_cases()[::6]
    bad = [c for c in pngfx.declined_cases() if c[0] not in PIL_RAISES]
    cases = []
    for i, c in enumerate(good):
        cases.append(c)
        if i < len(bad):
            cases.append(bad[i])
    paths = pngfx.write_all(str(tmp_path), cases)
    kinds = []
    with DecodePool(paths, workers=2, ring_bytes=4 << 20, png=True) as pool:
        assert pool.torch_in_worker == [False, False]
        for i, item in pool.images():
            assert pool.held <= pool.ring_bytes
            ref = pngfx.pil_rgb(cases[i][1])
            if isinstance(item, png_host.PngRecord):
                kinds.append("record")
                got, st = png_host.decode_host(item._replace(data=item.data.copy()))
                assert st == 0
            else:
                kinds.append("pixels")
                got = item
            assert np.array_equal(got, ref), cases[i][0]
    assert kinds == ["pixels" if len(c) == 3 else "record" for c in cases] and kinds.count("pixels") == len(bad) >= 10
    # a corrupt file: declined by the parser, and PIL's own exception reaches the caller with the path
    p = pngfx.write_all(str(tmp_path), [c for c in pngfx.declined_cases() if c[0] == "stream_short"])
    with DecodePool(p, workers=1, ring_bytes=1 << 20, png=True) as pool:
        with pytest.raises(DecodeError, match="stream_short"):
            list(pool.images())
    # png off (the default): no worker emits a record
    with DecodePool(paths[:6], workers=1, ring_bytes=1 << 20) as pool:
        assert all(isinstance(a, np.ndarray) for _, a in pool.images())
