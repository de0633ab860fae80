"""GPU: the inflate of the PNG path on the device (lemon_png_inflate, csrc/png_inflate.hip) against its host twin and zlib, bit
for bit, on the streams of tests/inflatefx.py in batches of mixed sizes with poisoned buffers; the declines interleaved with
good streams; aux rows that leave their buffers; the chain into lemon_png_decode through decode_pngs(inflate="device") and the
loader under LEMON_PNG=device; and the kernel's resource figures as DESIGN.md states them."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import deflatefx as fx
from tests import inflatefx, pngfx
from tests.test_gpu_png import _mixed_directory

pytestmark = pytest.mark.gpu

POISON = 0xA5
STREAM, BUFFER = 12, 11


def device_inflate(cases, z_slack=0, aux_edit=None):
    """One launch over [(stream, want)]: streams packed at varying alignments, rows at varying alignments, everything else
    poisoned.  -> (statuses, [rows], z buffer before, z buffer after, rec buffer after, aux)."""
    from lemon_amd import _lib
    from lemon_amd.ops import stream_ptr
    n = len(cases)
    aux = np.zeros((n, 4), np.int64)
    zoff = roff = 7
    for i, (z, want) in enumerate(cases):
        zoff += (3 * i) % 5
        roff += (5 * i) % 7
        aux[i] = (zoff, len(z), roff, want)
        zoff += len(z)
        roff += want
    zbuf = np.full(zoff + 9 + z_slack, POISON, np.uint8)
    for i, (z, _) in enumerate(cases):
        zbuf[aux[i, 0]:aux[i, 0] + len(z)] = np.frombuffer(z, np.uint8)
    rec_bytes = roff + 11
    if aux_edit is not None:
        aux_edit(aux, zbuf.size, rec_bytes)
    dev = torch.device("cuda")
    z_dev = torch.from_numpy(zbuf).to(dev)
    rec = torch.full((rec_bytes,), POISON, dtype=torch.uint8, device=dev)
    aux_dev = torch.from_numpy(aux.copy()).to(dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    rc = _lib.load().lemon_png_inflate(vp(z_dev.data_ptr()), z_dev.numel(), n, vp(aux_dev.data_ptr()), vp(rec.data_ptr()), rec.numel(),
                                       vp(status.data_ptr()), stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    out = rec.cpu().numpy()
    return status.cpu().numpy(), [out[a[2]:a[2] + a[3]].tobytes() for a in aux], zbuf, z_dev.cpu().numpy(), out, aux


def host_inflate(z, want):
    from lemon_amd import png_host
    rows = np.empty(max(want, 1), np.uint8)
    st = ctypes.c_int32(-1)
    src = np.frombuffer(z, np.uint8) if len(z) else np.zeros(1, np.uint8)
    assert png_host.load().lemon_png_inflate_host(src.ctypes.data, len(z), rows.ctypes.data, want, ctypes.byref(st)) == 0
    return st.value, rows[:want].tobytes()


def check_untouched(out, aux, statuses):
    inside = np.zeros(out.size, bool)
    for a, st in zip(aux, statuses):
        if st != BUFFER:
            inside[a[2]:a[2] + a[3]] = True
    assert (out[~inside] == POISON).all()


def test_device_equals_the_host_twin_and_zlib_on_every_stream_in_batches_of_mixed_sizes(hip):
    cases = [(z, want) for _, z, want in inflatefx.edge_cases() + inflatefx.zlib_cases()]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(cases))                  # sizes mixed within every batch
    cases = [cases[i] for i in order]
    at, k = 0, 0
    sizes = [1, 2, 63, 64, 65]
    while at < len(cases):
        size = sizes[k] if k < len(sizes) else 1024
        batch = cases[at:at + size]
        status, rows, z_before, z_after, out, aux = device_inflate(batch)
        assert np.array_equal(z_before, z_after)         # the input is untouched
        check_untouched(out, aux, status)                # nothing outside each image's `want` bytes changed
        for j, (z, want) in enumerate(batch):
            ok, ref = fx.zlib_verdict(z, want)
            assert ok and status[j] == 0, (at + j, int(status[j]))
            assert rows[j] == ref, at + j
        for j in range(0, len(batch), 16 if k >= len(sizes) else 1):     # the host twin: every stream of the small batches, a sample of the rest (all of them on the CPU: test_png_inflate_host.py)
            hst, hrows = host_inflate(*batch[j])
            assert hst == status[j] and hrows == rows[j], at + j
        at += size
        k += 1
    assert k >= 7


def test_declines_interleaved_with_good_streams_get_their_status_and_leave_the_neighbours_exact(hip):
    good = [(z, want) for _, z, want in inflatefx.edge_cases()[:20]]
    bad = inflatefx.decline_cases()
    batch, kinds = [], []
    for k, (name, z, want, strict) in enumerate(bad):
        batch += [good[k % len(good)], (z, want)]
        kinds += [None, (name, strict)]
    batch.append(good[0])
    kinds.append(None)
    status, rows, z_before, z_after, out, aux = device_inflate(batch)
    assert np.array_equal(z_before, z_after)
    check_untouched(out, aux, status)
    for j, ((z, want), kind) in enumerate(zip(batch, kinds)):
        ok, ref = fx.zlib_verdict(z, want)
        hst, hrows = host_inflate(z, want)
        assert status[j] == hst, (j, kind)
        if kind is None or kind[1] is None:
            assert ok and status[j] == 0 and rows[j] == ref, (j, kind)
        elif kind[1]:
            assert not ok and status[j] == STREAM, kind
        else:
            assert status[j] == STREAM or rows[j] == ref, kind


def test_aux_rows_that_leave_their_buffers_get_the_buffer_status_and_touch_nothing(hip):
    good = [(z, want) for _, z, want in inflatefx.edge_cases()[:8]]

    def edit(aux, z_bytes, rec_bytes):
        aux[1, 0] = z_bytes - aux[1, 1] + 1               # the stream's end one past z_bytes
        aux[2, 2] = rec_bytes - aux[2, 3] + 1             # the rows' end one past rec_bytes
        aux[3, 0] = -1
        aux[4, 2] = -16
        aux[5, 1] = 1 << 62
        aux[6, 3] = 1 << 62

    status, rows, z_before, z_after, out, aux = device_inflate(good, aux_edit=edit)
    assert list(status) == [0, BUFFER, BUFFER, BUFFER, BUFFER, BUFFER, BUFFER, 0]
    assert np.array_equal(z_before, z_after)
    check_untouched(out, aux, status)
    for j in (0, 7):
        assert rows[j] == fx.zlib_verdict(*good[j])[1]
    from lemon_amd import _lib
    assert _lib.load().lemon_png_inflate(None, 0, 0, None, None, 0, None, None) == 0         # an empty batch
    assert _lib.load().lemon_png_inflate(None, 0, 1, None, None, 0, None, None) != 0


def test_decode_pngs_with_the_device_inflate_equals_pil(hip, tmp_path):
    from lemon_amd import png_host
    from lemon_amd.data import decode_pngs
    accepted = pngfx.accepted_cases()
    paths = pngfx.write_all(str(tmp_path), accepted[:5])
    files = paths + [c[1] for c in accepted[5:]]
    r = decode_pngs(files, "cuda", poison=POISON, inflate="device")
    assert len(r) == len(accepted) and r.layout.n_png == len(r.layout.png_streams) == len(accepted) and not r.status.any()
    host = decode_pngs(files, "cuda", inflate="host")
    data = r.data.cpu().numpy()
    covered = np.zeros(data.size, bool)
    covered[:r.layout.png_rec_end] = True             # the copied payload and the device-only records
    for i, (name, raw) in enumerate(accepted):
        ref = pngfx.pil_rgb(raw)
        o, h, w, _ = (int(v) for v in r.desc[i])
        assert np.array_equal(data[o:o + h * w * 3].reshape(h, w, 3), ref), name
        assert torch.equal(r.image(i), host.image(i)), name
        covered[o:o + h * w * 3] = True
        rec, _ = png_host.decode_record(raw)              # the record zlib fills: the device's, palette included for type 3
        _, roff, _, _, ct, _ = r.layout.png_records[i]
        lo = 0 if ct == 3 else 1024
        assert np.array_equal(data[roff + lo:roff + rec.data.size], rec.data[lo:]), name
    assert (data[~covered] == POISON).all()
    # the declined: a stream defect is now the device's verdict; fallback fills every declined file from PIL
    declined = pngfx.declined_cases()
    stream_bad = [c for c in declined if c[2] == STREAM]
    assert len(stream_bad) == 3
    for name, raw, _ in stream_bad:
        with pytest.raises(ValueError, match="zlib stream"):
            decode_pngs([accepted[0][1], raw], "cuda", inflate="device")
    readable = [c for c in declined if c[0] in ("depth16", "depth4", "stream_long", "stream_garbage", "actl")]
    assert [c[0] for c in readable] == ["depth16", "depth4", "actl", "stream_long", "stream_garbage"]
    files = [accepted[3][1]] + [c[1] for c in readable] + [accepted[40][1]]
    r = decode_pngs(files, "cuda", fallback=True, inflate="device")
    assert r.layout.n_png == 4 and list(r.status) == [0, STREAM, STREAM, 0]
    for i, raw in enumerate(files):
        assert np.array_equal(r.image(i).cpu().numpy(), pngfx.pil_rgb(raw)), i
    with pytest.raises(ValueError, match="inflate"):
        decode_pngs(files, "cuda", inflate="gpu")
    assert len(decode_pngs([], "cuda", inflate="device")) == 0


@pytest.mark.parametrize("jpeg_mode", ["pil", "device"])
def test_file_batches_with_lemon_png_device_equal_the_pil_mode(hip, tmp_path, monkeypatch, jpeg_mode):
    from lemon_amd.data import gpu_transform_ragged
    from lemon_amd.loader import png_default, png_inflate_default, ragged_batches
    paths, n_records, n_fallback = _mixed_directory(str(tmp_path))
    monkeypatch.setenv("LEMON_JPEG", jpeg_mode)
    res = {}
    for mode in ("pil", "device"):
        monkeypatch.setenv("LEMON_PNG", mode)
        assert png_default() is (mode == "device") and png_inflate_default() is (mode == "device")
        stats, imgs, feats = {}, [], []
        for s, e, px in ragged_batches(paths, 16, 0, len(paths), "cuda", workers=2, ring_bytes=8 << 20, stats=stats):
            imgs += [px.image(i).cpu() for i in range(len(px))]
            feats.append(gpu_transform_ragged(px, 32).cpu())
        res[mode] = (imgs, torch.cat(feats), stats)
    for i, p in enumerate(paths):
        ref = torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy())
        assert torch.equal(res["device"][0][i], ref) and torch.equal(res["pil"][0][i], ref), p
    assert torch.equal(res["device"][1], res["pil"][1])
    # the workers no longer inflate: the file with one scanline byte too many is a stream now, and the device declines it
    st = res["device"][2]
    assert st["png_streams"] == st["png_records"] == n_records + 1 and st["png_fallback"] == n_fallback + 1
    assert "png_streams" not in res["pil"][2] and "png_fallback" not in res["pil"][2]
    monkeypatch.setenv("LEMON_PNG", "gpu")
    assert png_default() is True and png_inflate_default() is False
    monkeypatch.setenv("LEMON_PNG", "inflate")
    with pytest.raises(ValueError, match="LEMON_PNG"):
        png_inflate_default()


def test_the_kernel_uses_no_scratch_and_the_lds_and_registers_design_md_states():
    from tests.test_build_guard import _kernel_asm
    import re
    asm = _kernel_asm("png_inflate.hip")
    blocks = [b for b in asm.split("  - .agpr_count:")[1:] if "k_png_inflate" in re.search(r"\.name:\s+(\S+)", b).group(1)]
    assert len(blocks) == 1
    meta = {k: int(re.search(rf"\.{k}:\s+(\d+)", blocks[0]).group(1))
            for k in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "vgpr_spill_count")}
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, meta
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    stated = re.search(r"k_png_inflate: (\d+) bytes of LDS, (\d+) VGPRs, no scratch", design)
    assert stated, "DESIGN.md states the kernel's resources"
    assert (meta["group_segment_fixed_size"], meta["vgpr_count"]) == (int(stated.group(1)), int(stated.group(2))), meta
    assert meta["group_segment_fixed_size"] <= 40 * 1024          # four resident streams per CU
