"""GPU: the Huffman pass of baseline JPEGs on the device (lemon_jpeg_entropy_device, csrc/jpeg_entropy.hip) against the host pass
and PIL, bit for bit: the raw entry point over poisoned buffers, the public decode_jpegs(entropy="device"), corrupt scans against
the same functions looped on the host, and the file batches of ImageLabelSet with LEMON_JPEG=device."""
import ctypes
import io
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpegfx
from tests.test_gpu_jpeg import _extra_files
from tests.test_gpu_file_pipeline import _write_files
from tests.test_jpeg_entropy_par import mutants, slow_sync_jpeg

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 4096


def _pil(raw):
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def _launch(packets, subseq):
    """lemon_jpeg_entropy_device over `packets` (JpegPacket list) with every buffer poisoned and guarded.
    -> (statuses, [record of each packet], layout, the whole record buffer, the payload as read back, the payload as sent)."""
    from lemon_amd import _lib, jpeg_host
    from lemon_amd.ops import stream_ptr
    lay, off, items = jpeg_host.BatchLayout(subseq), 0, []
    for pk in packets:
        lay.add_packet(off, pk)
        items.append((off, pk.data))
        off = (off + pk.data.nbytes + 15) & ~15
    aux = lay.finish(off)
    payload = np.zeros(lay.payload_bytes, np.uint8)
    for o, a in items:
        payload[o:o + a.nbytes] = a
    payload[lay.aux_off:] = aux.view(np.uint8)
    dev = torch.device("cuda")
    pk_dev = torch.from_numpy(payload).to(dev)
    # records addressed as in the product layout: offsets count from the buffer's start, the region before them is a guard here
    rec_dev = torch.full((lay.rec_end + GUARD,), POISON, dtype=torch.uint8, device=dev)
    st_dev = torch.full((len(packets) * 4 + 2 * GUARD,), POISON, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    ws = torch.full((lib.lemon_jpeg_entropy_workspace_bytes(len(packets), lay.groups, lay.intervals),), POISON, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    _lib.check(lib.lemon_jpeg_entropy_device(vp(pk_dev.data_ptr()), lay.payload_bytes, len(packets), vp(pk_dev.data_ptr() + lay.edesc_off),
                                             lay.groups, lay.intervals, subseq, vp(rec_dev.data_ptr()), lay.rec_end,
                                             vp(st_dev.data_ptr() + GUARD), vp(ws.data_ptr()), ws.numel(), stream_ptr(dev)),
               "lemon_jpeg_entropy_device")
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
    cases = jpegfx.accepted_cases()
    packets = [jpeg_host.pack(raw)[0] for _, raw in cases]
    refs = [jpeg_host.decode_record(raw)[0].data for _, raw in cases]
    return cases, packets, refs


@pytest.mark.parametrize("subseq", [16, 0])
def test_device_records_equal_the_host_pass_in_one_mixed_batch_with_poisoned_buffers(hip, accepted, subseq):
    cases, packets, refs = accepted
    assert len(cases) >= 82
    status, records, lay, after, before = _launch(packets, subseq)
    assert np.array_equal(after, before)                              # the packets are only read
    assert lay.groups > len(cases)                                    # some scans span several workgroups
    for (name, _), st, rec, ref in zip(cases, status, records, refs):
        assert st == 0, (name, subseq, int(st))
        assert np.array_equal(rec, ref), (name, subseq, int((rec != ref).sum()))


def test_packets_with_a_tampered_huffman_specification_get_the_looped_host_status(hip):
    # one launch: three codes of length 1 / counts summing to 510 written over a DC or an AC specification, between intact packets
    from lemon_amd import jpeg_host
    from tests import jpegverdictfx as fx
    _, _, bases = fx.load_golden()
    batch, good_ref = [], {}
    for name in fx.TAMPER_BASES[:2]:
        good = jpeg_host.pack(bases[name])[0]
        good_ref[len(batch)] = jpeg_host.decode_record(bases[name])[0].data
        batch.append(good)
        for _, p in fx.tampered_packets(name, bases[name]):
            good_ref[len(batch) + 1] = good_ref[len(batch) - 1]
            batch += [good._replace(data=p), good]
    assert len(batch) == 18
    status, records, lay, after, before = _launch(batch, jpeg_host.SUBSEQ_MIN)
    assert np.array_equal(after, before)                              # the packets are only read
    assert lay.groups >= len(batch) and min(pk.scan_bytes for pk in batch) > jpeg_host.SUBSEQ_MIN      # every scan: several lanes
    for k, pk in enumerate(batch):
        rec = np.full(records[k].size, POISON, np.uint8)
        want = jpeg_host.entropy_par_host(pk.data, rec, jpeg_host.SUBSEQ_MIN)
        assert status[k] == want == (0 if k in good_ref else 13), (k, int(status[k]), want)
        if k in good_ref:
            assert np.array_equal(records[k], good_ref[k]) and np.array_equal(rec, good_ref[k]), k
        else:
            assert (records[k] == POISON).all() and (rec == POISON).all(), k      # a refused image's record is not touched


def test_decode_jpegs_with_device_entropy_equals_pil(hip, tmp_path):
    from lemon_amd.data import RaggedImages, decode_jpegs
    cases = jpegfx.accepted_cases()
    raws = [c[1] for c in cases]
    paths = jpegfx.write_all(str(tmp_path), cases[:5])
    r = decode_jpegs(paths + raws[5:], "cuda", entropy="device", poison=POISON)
    assert isinstance(r, RaggedImages) and len(r) == len(cases) and r.layout.n_packets == len(cases)
    torch.cuda.synchronize()
    data = r.data.cpu().numpy()
    covered = np.zeros(data.size, bool)
    covered[:r.layout.decoded_off] = True             # the copied payload and the records
    for i, (name, raw) in enumerate(cases):
        ref = _pil(raw)
        o, h, w, _ = (int(v) for v in r.desc[i])
        assert (h, w) == ref.shape[:2] and o >= r.layout.decoded_off, name
        got = data[o:o + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got, ref), (name, int(np.abs(got.astype(int) - ref).max()), int((got != ref).sum()))
        covered[o:o + h * w * 3] = True
    assert (data[~covered] == POISON).all() and (~covered).sum() > 0
    # declined files behave as in host mode
    good = raws[3]
    for name, raw, pil_ok in jpegfx.declined_cases():
        with pytest.raises(ValueError, match="not decodable on the GPU"):
            decode_jpegs([good, raw], "cuda", entropy="device")
        if pil_ok:
            r = decode_jpegs([good, raw, good], "cuda", fallback=True, entropy="device")
            assert r.layout.n_jpeg == 2
            for i, x in enumerate((good, raw, good)):
                assert np.array_equal(r.image(i).cpu().numpy(), _pil(x)), (name, i)
        else:
            with pytest.raises(Exception) as e:          # PIL's own exception for a corrupt file
                decode_jpegs([good, raw], "cuda", fallback=True, entropy="device")
            assert not isinstance(e.value, ValueError) or "not decodable on the GPU" not in str(e.value)
    with pytest.raises(ValueError, match="entropy"):
        decode_jpegs([good], "cuda", entropy="gpu")
    assert len(decode_jpegs([], "cuda", entropy="device")) == 0


def _corrupt_scan_pil_still_decodes():
    """The first mutant whose scan the device declines while its header is fine and PIL still returns pixels of the header's size."""
    from lemon_amd import jpeg_host
    for name, raw in mutants(64):
        pk, head = jpeg_host.pack(raw)
        if pk is None:
            continue
        rec = np.zeros(head.record_bytes, np.uint8)
        if jpeg_host.entropy_par_host(pk.data, rec, 0) == 0:
            continue
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                px = _pil(raw)
        except Exception:       # noqa: BLE001
            continue
        if px.shape == (head.height, head.width, 3):
            return name, raw
    return None


def test_corrupt_scans_get_the_status_of_the_same_code_on_the_host(hip):
    # (one launch; these mutants have passed the sanitizer build of the same functions in tests/test_jpeg_entropy_par.py)
    from lemon_amd import jpeg_host
    packed = [(name, jpeg_host.pack(raw)) for name, raw in mutants(64)]
    packed = [(name, pk, head) for name, (pk, head) in packed if pk is not None]
    assert len(packed) >= 16                           # (the packer declines the others: their marker structure is broken)
    status, records, _, _, _ = _launch([pk for _, pk, _ in packed], jpeg_host.SUBSEQ_MIN)
    seen = set()
    for (name, pk, head), st, rec in zip(packed, status, records):
        ref = np.zeros(head.record_bytes, np.uint8)
        want = jpeg_host.entropy_par_host(pk.data, ref, jpeg_host.SUBSEQ_MIN)
        assert st == want, (name, int(st), want)
        seen.add(want)
        if want == 0:
            assert np.array_equal(rec, ref), name
    assert 0 in seen and len(seen) >= 3, seen          # accepted mutants and at least two kinds of decline


def test_states_that_meet_again_after_different_block_counts_get_the_host_codes_status(hip):
    # (tests/test_jpeg_entropy_par.py says what the file is: at 16-byte lanes the fourth workgroup's first lane cannot have settled)
    from lemon_amd import jpeg_host
    raw = slow_sync_jpeg(3 * 256 * 16)
    ref = jpeg_host.decode_record(raw)[0]
    pk = jpeg_host.pack(raw)[0]
    assert ref is not None and pk is not None
    for subseq, want in ((16, 16), (0, 0)):
        status, records, _, _, _ = _launch([pk, pk], subseq)
        assert list(status) == [want, want], (subseq, status)
        if want == 0:
            assert np.array_equal(records[0], ref.data) and np.array_equal(records[1], ref.data)


def test_file_batches_with_device_entropy_equal_the_pil_mode_bit_for_bit(hip, tmp_path, monkeypatch):
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import ImageLabelSet, RaggedImages
    from lemon_amd.pipeline import Embedder
    paths = _write_files(str(tmp_path), n_jpg=40)
    extra = _extra_files(str(tmp_path))               # a progressive file and a gray file
    paths[5:5] = extra[:1]
    paths.append(extra[1])
    corrupt = _corrupt_scan_pil_still_decodes()
    assert corrupt is not None                        # (the seeds yield one: a scan the device declines and PIL still decodes)
    paths[11:11] = jpegfx.write_all(str(tmp_path), [corrupt])
    n = len(paths)
    cfg = ClipConfig.named("tiny")
    torch.manual_seed(0)
    emb = Embedder(LemonCLIP(cfg), torch.device("cuda"), batch_size=24)
    dset = ImageLabelSet(paths, list(range(n)), list(range(n)), image_size=cfg.image_size)
    res = {}
    for mode in ("pil", "device"):
        monkeypatch.setenv("LEMON_JPEG", mode)
        imgs, embs, seen = [], [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for px, clean, noisy in dset.batches(16, 0, n, device="cuda"):
                assert isinstance(px, RaggedImages) and len(px) == len(noisy)
                seen += list(noisy)
                imgs += [px.image(i).cpu() for i in range(len(px))]
                embs.append(emb.embed_images(px))
        emb.raise_if_nonfinite()
        assert seen == list(range(n))
        res[mode] = (imgs, torch.cat(embs))
    for i, p in enumerate(paths):
        assert torch.equal(res["device"][0][i], res["pil"][0][i]), p
    assert torch.equal(res["device"][1], res["pil"][1])
