"""GPU: the Huffman pass of progressive JPEGs on the device (lemon_jpeg_prog_entropy_device, csrc/jpeg_prog.hip) against the host
pass and PIL, bit for bit: the raw entry point over poisoned buffers, decode_jpegs(progressive=True) with both entropy modes,
corrupt scans against the same functions looped on the host, and file batches with LEMON_JPEG_PROGRESSIVE=1."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpegfx, jpegprogfx

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 4096


def _pil(raw):
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def _launch(packets):
    """lemon_jpeg_prog_entropy_device over `packets` (JpegProgPacket list) with every buffer poisoned and guarded.
    -> (statuses, [record of each packet], layout, the payload as read back, the payload as sent)."""
    from lemon_amd import _lib, jpeg_host
    from lemon_amd.ops import stream_ptr
    lay, off, items = jpeg_host.BatchLayout(), 0, []
    for pk in packets:
        lay.add_packet(off, pk)
        items.append((off, pk.data))
        off = (off + pk.data.nbytes + 15) & ~15
    aux = lay.finish(off)
    assert lay.n_prog == len(packets) and lay.n_packets == 0
    payload = np.zeros(lay.payload_bytes, np.uint8)
    for o, a in items:
        payload[o:o + a.nbytes] = a
    payload[lay.aux_off:] = aux.view(np.uint8)
    dev = torch.device("cuda")
    pk_dev = torch.from_numpy(payload).to(dev)
    rec_dev = torch.full((lay.rec_end + GUARD,), POISON, dtype=torch.uint8, device=dev)
    st_dev = torch.full((len(packets) * 4 + 2 * GUARD,), POISON, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    need = lib.lemon_jpeg_prog_entropy_workspace_bytes(len(packets), lay.prog_items, lay.prog_levels)
    assert need > 0
    ws = torch.full((need,), POISON, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    _lib.check(lib.lemon_jpeg_prog_entropy_device(vp(pk_dev.data_ptr()), lay.payload_bytes, len(packets), vp(pk_dev.data_ptr() + lay.pdesc_off),
                                                  lay.prog_items, lay.prog_levels, vp(rec_dev.data_ptr()), lay.rec_end,
                                                  vp(st_dev.data_ptr() + GUARD), vp(ws.data_ptr()), ws.numel(), stream_ptr(dev)),
               "lemon_jpeg_prog_entropy_device")
    torch.cuda.synchronize()
    rec, st = rec_dev.cpu().numpy(), st_dev.cpu().numpy()
    assert (st[:GUARD] == POISON).all() and (st[GUARD + 4 * len(packets):] == POISON).all()      # around the statuses
    records = []
    covered = np.zeros(rec.size, bool)
    for (i, roff, w, h, nc, hs, vs) in lay.records:
        n = jpeg_host.QUANT_BYTES + 128 * jpeg_host.blocks_of(w, h, nc, hs, vs)
        assert not covered[roff:roff + n].any()
        covered[roff:roff + n] = True
        records.append(rec[roff:roff + n])
    assert (rec[~covered] == POISON).all() and (~covered).sum() >= GUARD + lay.payload_bytes      # around and before the records
    return st[GUARD:GUARD + 4 * len(packets)].view(np.int32).copy(), records, lay, pk_dev.cpu().numpy(), payload


@pytest.fixture(scope="module")
def accepted():
    from lemon_amd import jpeg_host
    cases = jpegprogfx.accepted_cases()
    packets = [jpeg_host.prog_pack(raw)[0] for _, raw in cases]
    refs = [jpeg_host.decode_record(raw, progressive=True)[0].data for _, raw in cases]
    return cases, packets, refs


def test_device_records_equal_the_host_pass_in_one_mixed_batch_with_poisoned_buffers(hip, accepted):
    cases, packets, refs = accepted
    assert len(cases) == 59 and all(pk is not None for pk in packets)
    status, records, lay, after, before = _launch(packets)
    assert np.array_equal(after, before)                              # the packets are only read
    assert lay.prog_levels == 3 and lay.prog_items > sum(pk.scans for pk in packets)      # some scans take several waves
    for (name, _), st, rec, ref in zip(cases, status, records, refs):
        assert st == 0, (name, int(st))
        assert np.array_equal(rec, ref), (name, int((rec != ref).sum()))


def test_decode_jpegs_with_progressive_files_equals_pil(hip, tmp_path):
    from lemon_amd.data import RaggedImages, decode_jpegs
    prog = [c for c in jpegprogfx.accepted_cases() if c[0] in ("37x53_ss2_q90", "64x80_ss0_q30", "1x1_ss1_q90", "gray_41x67",
                                                               "restart_rows1", "noise_q95", "640x480")]
    base = jpegfx.accepted_cases()[60:64]
    cmyk = next(c[:2] for c in jpegfx.declined_cases() if c[0] == "cmyk")
    cases = [prog[0], base[0], prog[1], prog[2], cmyk, base[1], prog[3], prog[4], base[2], prog[5], base[3], prog[6]]
    raws = [c[1] for c in cases]
    paths = jpegfx.write_all(str(tmp_path), cases[:3])
    for entropy in ("host", "device"):
        r = decode_jpegs(paths + raws[3:], "cuda", fallback=True, entropy=entropy, progressive=True, poison=POISON)
        assert isinstance(r, RaggedImages) and len(r) == len(cases)
        assert r.layout.n_jpeg == len(cases) - 1 and r.layout.n_progressive == len(prog)      # all but the CMYK file
        if entropy == "device":
            assert r.layout.n_prog == len(prog) and r.layout.n_packets == len(base)
        for i, (name, raw) in enumerate(cases):
            assert np.array_equal(r.image(i).cpu().numpy(), _pil(raw)), (entropy, name)
        # without the switch the same call treats the progressive files as before: declined, or PIL's pixels with fallback
        with pytest.raises(ValueError, match="not decodable on the GPU"):
            decode_jpegs(raws[:2], "cuda", entropy=entropy)
        r = decode_jpegs(raws, "cuda", fallback=True, entropy=entropy)
        assert r.layout.n_jpeg == len(base) and r.layout.n_progressive == 0
        for i, (name, raw) in enumerate(cases):
            assert np.array_equal(r.image(i).cpu().numpy(), _pil(raw)), (entropy, name)


def test_corrupt_scans_get_the_host_codes_status_and_leave_their_neighbours_alone(hip, accepted):
    # (one launch; the same step functions have passed the sanitizer build in tests/test_jpeg_progressive.py)
    from lemon_amd import jpeg_host
    cases, packets, refs = accepted
    at = [name for name, _ in cases].index("64x80_ss2_q90")
    good, good_ref = packets[at], refs[at]
    bad = jpegprogfx.corrupt_packets(cases[at][1])
    assert [n for n, _ in bad] == ["refine_size_2", "eob_run_past_end", "bad_code", "early_end", "left_over"]
    batch = [good]
    for _, p in bad:
        batch += [good._replace(data=p), good]
    status, records, _, _, _ = _launch(batch)
    want = []
    for k, pk in enumerate(batch):
        ref = np.zeros(good_ref.size, np.uint8)
        want.append(jpeg_host.prog_entropy_par_host(pk.data, ref))
        assert status[k] == want[k], (k, int(status[k]), want[k])
        if k % 2 == 0:
            assert want[k] == 0 and np.array_equal(records[k], good_ref), k
    assert want[1::2] == [10, 11, 10, 11, 11], want                   # size-2 symbol: code; run past the end, early end, left over: stream


def test_packets_with_a_tampered_huffman_specification_get_the_looped_host_status(hip):
    # one launch: a specification of the pool overwritten (three codes of length 1, counts summing to 510, values that run past
    # the packet's end) or its pool offset pointing past the packet, between intact packets
    from lemon_amd import jpeg_host
    from tests import jpegverdictfx as fx
    _, _, bases = fx.load_golden()
    batch, good_ref = [], {}
    for name in fx.TAMPER_BASES[2:]:
        good = jpeg_host.prog_pack(bases[name])[0]
        good_ref[len(batch)] = jpeg_host.decode_record(bases[name], progressive=True)[0].data
        batch.append(good)
        for _, p in fx.tampered_packets(name, bases[name]):
            good_ref[len(batch) + 1] = good_ref[len(batch) - 1]
            batch += [good._replace(data=p), good]
    assert len(batch) == 26
    status, records, lay, after, before = _launch(batch)
    assert np.array_equal(after, before)                              # the packets are only read
    for k, pk in enumerate(batch):
        rec = np.full(records[k].size, POISON, np.uint8)
        want = jpeg_host.prog_entropy_par_host(pk.data, rec)
        assert status[k] == want == (0 if k in good_ref else 8), (k, int(status[k]), want)
        if k in good_ref:
            assert np.array_equal(records[k], good_ref[k]) and np.array_equal(rec, good_ref[k]), k


def _write_mixed(d, n=40):
    """n files of three sizes, every third progressive (with and without restart markers, one grayscale)."""
    rng = np.random.default_rng(7)
    sizes = [(96, 128), (75, 100), (64, 80)]
    paths, n_prog = [], 0
    for i in range(n):
        h, w = sizes[i % 3]
        gray = i == 9
        px = jpegfx.pixels(w, h, rng, channels=1 if gray else 3)
        kw = dict(quality=(90, 60, 30)[i % 3], subsampling=i % 3) if not gray else dict(quality=85)
        if i % 3 == 0:
            kw["progressive"] = True
            n_prog += 1
            if i % 2:
                kw["restart_marker_rows"] = 1
        p = os.path.join(d, f"{i:03d}.jpg")
        Image.fromarray(px).save(p, **kw)
        paths.append(p)
    return paths, n_prog


def test_file_batches_with_the_progressive_switch_equal_the_pil_mode_bit_for_bit(hip, tmp_path, monkeypatch):
    from lemon_amd import loader
    from lemon_amd.data import ImageLabelSet, RaggedImages
    paths, n_prog = _write_mixed(str(tmp_path))
    n = len(paths)
    assert n == 40 and n_prog == 14

    def run(mode, switch):
        monkeypatch.setenv("LEMON_JPEG", mode)
        if switch is None:
            monkeypatch.delenv("LEMON_JPEG_PROGRESSIVE", raising=False)
        else:
            monkeypatch.setenv("LEMON_JPEG_PROGRESSIVE", switch)
        stats, imgs = {}, []
        for s, e, px in loader.ragged_batches(paths, 16, 0, n, "cuda", workers=2, stats=stats):
            assert isinstance(px, RaggedImages) and len(px) == e - s
            imgs += [px.image(i).cpu() for i in range(len(px))]
        return imgs, stats

    ref, stats = run("pil", "1")
    assert stats.get("jpeg_progressive", 0) == 0                      # (ignored in pil mode)
    for i, p in enumerate(paths):
        assert np.array_equal(ref[i].numpy(), np.asarray(Image.open(p).convert("RGB"))), p
    for mode in ("gpu", "device"):
        got, stats = run(mode, "1")
        assert stats.get("jpeg_fallback", 0) == 0 and stats["jpeg_progressive"] == n_prog and stats["jpeg_images"] == n, (mode, stats)
        for i, p in enumerate(paths):
            assert torch.equal(got[i], ref[i]), (mode, p)
        got, stats = run(mode, None)                                  # without the variable: PIL decodes them in the workers
        assert stats["jpeg_progressive"] == 0 and stats["jpeg_images"] == n - n_prog, (mode, stats)
        for i, p in enumerate(paths):
            assert torch.equal(got[i], ref[i]), (mode, p)
    # the dataset's own batches read the same variables
    monkeypatch.setenv("LEMON_JPEG", "device")
    monkeypatch.setenv("LEMON_JPEG_PROGRESSIVE", "1")
    dset = ImageLabelSet(paths, list(range(n)), list(range(n)), image_size=32)
    seen = 0
    for px, clean, noisy in dset.batches(16, 0, n, device="cuda"):
        for i in range(len(px)):
            assert torch.equal(px.image(i).cpu(), ref[seen + i]), seen + i
        seen += len(px)
    assert seen == n
