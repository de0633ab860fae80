"""GPU: the JPEG kernels on files written coefficient by coefficient (tests/jpegcoeffx.py), each list aimed at one kernel edge:
lemon_jpeg_entropy_device (csrc/jpeg_entropy.hip) over poisoned and guarded buffers, one mixed batch per list and lane size,
against the writer's record and the status of the same functions looped on the host; and decode_jpegs (csrc/jpeg.hip) with the
Huffman pass on the device and on the host against PIL.  Every criterion is equality.  What the files are -- lane counts,
interval sizes, bit positions, plane borders -- is asserted by the PLACEMENTS of tests/test_jpeg_coef_host.py, which pins the
writer and the host side on a machine without a GPU."""
import numpy as np
import pytest
import torch

from tests import jpegcoeffx as fx
from tests.test_gpu_jpeg_entropy import POISON, _launch
from tests.test_jpeg_coef_host import LANE_SIZES, PLACEMENTS

pytestmark = pytest.mark.gpu

ENTROPY_LANES = {"big": (0, 4096, 16)}          # (every other list: LANE_SIZES, the five of the host module)


@pytest.fixture(scope="module")
def packed():
    """name -> (cases, placements, packets, host status of every case), built once."""
    from lemon_amd import jpeg_host
    cache = {}

    def get(name):
        if name not in cache:
            cases = fx.LISTS[name]()
            packets = [jpeg_host.pack(c.jpeg.raw)[0] for c in cases]
            assert all(pk is not None for pk in packets)
            cache[name] = (cases, PLACEMENTS[name](cases), packets, [jpeg_host.decode_record(c.jpeg.raw)[1].status for c in cases])
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(fx.LISTS))
def test_device_huffman_pass_gives_the_writers_record_and_the_host_loops_status(hip, packed, name):
    from lemon_amd import jpeg_host
    cases, _, packets, host_status = packed(name)
    for subseq in ENTROPY_LANES.get(name, LANE_SIZES):
        status, records, lay, after, before = _launch(packets, subseq)
        assert np.array_equal(after, before)                                         # the packets are only read
        assert lay.intervals == sum(len(c.jpeg.interval_bytes) for c in cases)
        for c, pk, st, rec, hst in zip(cases, packets, status, records, host_status):
            twin = np.full(rec.size, POISON, np.uint8)
            want = jpeg_host.entropy_par_host(pk.data, twin, subseq)
            assert st == want, (c.name, subseq, int(st), want)
            if not c.one_byte or subseq != 16:
                assert want == hst, (c.name, subseq, want, hst)                      # (settled: the sequential pass's verdict)
            if st == 0:
                assert np.array_equal(rec, c.jpeg.record), (c.name, subseq, int((rec != c.jpeg.record).sum()))


def _decode_and_compare(cases, entropy, refs):
    """One ragged batch through decode_jpegs over a poisoned buffer -> the batch; every image equal to refs[i]."""
    from lemon_amd.data import decode_jpegs
    r = decode_jpegs([c.jpeg.raw for c in cases], "cuda", poison=POISON, fallback=True, entropy=entropy)
    torch.cuda.synchronize()
    data = r.data.cpu().numpy()
    covered = np.zeros(data.size, bool)
    covered[:r.layout.decoded_off] = True
    for i, c in enumerate(cases):
        o, h, w, _ = (int(v) for v in r.desc[i])
        assert (h, w) == refs[i].shape[:2], c.name
        if o >= r.layout.decoded_off:                                                # (a declined file's PIL pixels lie in the payload)
            assert not covered[o:o + h * w * 3].any(), c.name
            covered[o:o + h * w * 3] = True
        got = data[o:o + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got, refs[i]), (c.name, entropy, int((got != refs[i]).sum()), int(np.abs(got.astype(int) - refs[i]).max()))
    assert (data[~covered] == POISON).all()                                          # nothing written between or after the images
    return r


@pytest.fixture(scope="module")
def pil_refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = [fx.pil_rgb(c.jpeg.raw) for c in fx.LISTS[name]()]
        return cache[name]
    return get


@pytest.mark.parametrize("entropy", ["device", "host"])
@pytest.mark.parametrize("name", [n for n in fx.LISTS if n not in ("envelope", "dc_range", "padding")])
def test_decode_jpegs_equals_pil(hip, packed, pil_refs, name, entropy):
    cases, _, _, host_status = packed(name)
    assert not any(host_status)
    if name == "big" and entropy == "device":
        cases = cases[:1]                       # (the pixels of one 6-megapixel file: the Huffman pass of all three is tested above)
    r = _decode_and_compare(cases, entropy, pil_refs(name))
    assert r.layout.n_jpeg == len(cases)


@pytest.mark.parametrize("entropy", ["device", "host"])
def test_padding_files_decode_to_pil_and_to_their_twins_at_every_store_alignment(hip, packed, pil_refs, entropy):
    cases, placed, _, host_status = packed("padding")
    assert not any(host_status) and placed["pairs"] >= 100
    refs = pil_refs("padding")
    r = _decode_and_compare(cases, entropy, refs)
    by = {c.name: i for i, c in enumerate(cases)}
    for n, i in by.items():
        if n + "_twin" in by:
            assert torch.equal(r.image(i), r.image(by[n + "_twin"])), n
    # both store paths of the colour kernel: lanes of four whole pixels at addresses of every residue mod 4, and short lanes
    full, short = set(), set()
    for o, h, w, _ in (tuple(int(v) for v in d) for d in r.desc):
        for y in range(h):
            for x0 in range(0, w, 4):
                (full if w - x0 >= 4 else short).add((o + (y * w + x0) * 3) % 4)
    assert full == {0, 1, 2, 3} and short == {0, 1, 2, 3}, (full, short)
    assert all(int(d[0]) % 16 == 0 for d in r.desc)                                  # (an image itself starts 16-byte aligned)


@pytest.mark.parametrize("entropy", ["device", "host"])
def test_envelope_files_equal_pil_when_accepted_and_fall_back_to_pil_when_declined(hip, packed, pil_refs, entropy):
    from lemon_amd.data import decode_jpegs
    for name in ("envelope", "dc_range"):
        cases, placed, _, host_status = packed(name)
        r = _decode_and_compare(cases, entropy, pil_refs(name))                      # declined ones come back as PIL's pixels
        if entropy == "host":
            assert r.layout.n_jpeg == sum(st == 0 for st in host_status)             # (on the device every packet is tried)
        first = next(i for i, st in enumerate(host_status) if st != 0)
        with pytest.raises(ValueError, match="not decodable on the GPU .outside the arithmetic envelope"):
            decode_jpegs([cases[0].jpeg.raw, cases[first].jpeg.raw], "cuda", entropy=entropy)
    cases, placed, _, host_status = packed("envelope")
    assert placed["random_accepted_exact"] >= 50 and placed["random_declined"] >= 50 and placed["single"] == 128
    assert host_status[0] in (0, 12) and set(host_status) == {0, 12}
