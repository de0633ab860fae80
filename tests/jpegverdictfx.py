"""The recorded verdicts of the JPEG host passes (tests/golden/jpeg_verdicts.npz, written by tools/make_golden_jpeg.py): how a
mutant is rebuilt from its base file, what is recorded of every entry point of lemon_amd/jpeg_host.py, and the packets with a
tampered Huffman specification that tests/test_jpeg_verdicts_host.py and the GPU tests send through the looped and the device
passes.  Uses the public functions of lemon_amd/jpeg_host.py only, so it runs against any commit's libraries."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_verdicts.npz")
XOR, SET, DEL, CUT, INS_MARKER, INS_BYTE = range(6)     # kinds of one (offset, kind, value) step; CUT value 1: EOI appended
MAX_OPS = 8
ENTRY_POINTS = ("info", "entropy", "pack", "entropy_par_host_16", "entropy_par_host_default", "prog_info", "prog_entropy",
                "prog_pack", "prog_entropy_par_host")
INFO_FIELDS = ("width", "height", "components", "hs", "vs", "record_bytes", "max_abs", "exact_blocks")
NOT_RUN = -1             # status of a looped-device pass whose packer declined the file
TAMPER_BASES = ("base_17x24_420", "base_37x53_444", "prog_17x24_420", "prog_37x53_444")


def apply(raw, ops):
    """The mutant of `raw`: the steps in order, each on the bytes the steps before it left."""
    m = bytearray(raw)
    for at, kind, value in ops:
        if kind < 0:
            break
        if kind == XOR:
            m[at] ^= value
        elif kind == SET:
            m[at] = value
        elif kind == DEL:
            del m[at]
        elif kind == CUT:
            del m[at:]
            if value:
                m += b"\xff\xd9"
        elif kind == INS_MARKER:
            m[at:at] = bytes([0xFF, value])
        elif kind == INS_BYTE:
            m[at:at] = bytes([value])
        else:
            raise ValueError(kind)
    return bytes(m)


def _fields(head):
    return [int(getattr(head, f)) for f in INFO_FIELDS]


def evaluate(raw):
    """(status [9], info [9][8], digest [9]: SHA-256 of the packet or record an entry point wrote with status 0, else None)."""
    from lemon_amd import jpeg_host
    status, info, digest = [], [], []

    def put(st, head=None, out=None):
        status.append(st)
        info.append(_fields(head) if head is not None else [0] * len(INFO_FIELDS))
        digest.append(hashlib.sha256(out.tobytes()).digest() if st == 0 and out is not None else None)

    def record_for(head):
        return np.full(head.record_bytes if head.status == 0 else 16, 0xA5, np.uint8)

    for prog in (False, True):
        head = jpeg_host.prog_info(raw) if prog else jpeg_host.info(raw)
        put(head.status, head)
        rec = record_for(head)
        full = jpeg_host.prog_entropy(raw, rec) if prog else jpeg_host.entropy(raw, rec)
        put(full.status, full, rec[:full.record_bytes])
        pk, phead = jpeg_host.prog_pack(raw) if prog else jpeg_host.pack(raw)
        put(phead.status, phead, pk.data if pk is not None else None)
        for subseq in ((None,) if prog else (jpeg_host.SUBSEQ_MIN, 0)):
            if pk is None:
                put(NOT_RUN)
                continue
            rec = record_for(phead)
            st = jpeg_host.prog_entropy_par_host(pk.data, rec) if prog else jpeg_host.entropy_par_host(pk.data, rec, subseq)
            put(st, None, rec)
    return status, info, digest


def _aligned_copy(pk):
    buf = np.empty(pk.size + 16, np.uint8)
    at = (-buf.ctypes.data) % 16
    out = buf[at:at + pk.size]
    out[:] = pk
    return out


def tampered_packets(name, raw):
    """[(name, packet)]: the packet of a base file with one Huffman specification overwritten.  A baseline packet keeps its
    eight specifications of 16 counts + 256 values from byte 512 on (csrc/jpeg_par.hpp); a progressive packet keeps a pool of
    offsets to specifications of 16 counts + sum(counts) values (csrc/jpeg_prog_par.hpp)."""
    from lemon_amd import jpeg_host
    prog = name.startswith("prog_")
    pk, head = jpeg_host.prog_pack(raw) if prog else jpeg_host.pack(raw)
    assert pk is not None, (name, head.status)
    base = pk.data.copy()
    three_of_length_1 = np.zeros(16, np.uint8)
    three_of_length_1[0] = 3
    sum_510 = np.zeros(16, np.uint8)
    sum_510[14:] = 255
    out = []
    if not prog:
        for label, counts in (("three_codes_of_length_1", three_of_length_1), ("counts_sum_510", sum_510)):
            for table, at in (("dc0", 512), ("ac0", 512 + 4 * 272)):
                p = base.copy()
                p[at:at + 16] = counts
                out.append((f"{name}/{label}/{table}", _aligned_copy(p)))
        return out
    hd = base[:128].view(np.int32)
    pool_off, entries = int(hd[10]), int(hd[7])
    pool = lambda p: p[pool_off:pool_off + 4 * entries].view(np.uint32)
    for label, counts in (("three_codes_of_length_1", three_of_length_1), ("counts_sum_510", sum_510)):
        for idx in (0, entries - 1):
            p = base.copy()
            at = int(pool(p)[idx])
            p[at:at + 16] = counts
            out.append((f"{name}/{label}/pool{idx}", _aligned_copy(p)))
    p = base.copy()                                      # a specification in the packet's last 16 bytes: its values lie past the end
    pool(p)[0] = p.size - 16
    p[p.size - 16:] = 0
    p[p.size - 15] = 2
    out.append((f"{name}/values_past_the_end", _aligned_copy(p)))
    p = base.copy()
    pool(p)[entries - 1] = p.size + 64
    out.append((f"{name}/pool_offset_past_the_packet", _aligned_copy(p)))
    return out


def tampered_status(name, packet, record_bytes):
    """Status of the looped-device pass on a packet of tampered_packets(), and the record it was given."""
    from lemon_amd import jpeg_host
    rec = np.full(record_bytes, 0xA5, np.uint8)
    if name.startswith("prog_"):
        return jpeg_host.prog_entropy_par_host(packet, rec), rec
    return jpeg_host.entropy_par_host(packet, rec, jpeg_host.SUBSEQ_MIN), rec


def load_golden():
    z = np.load(GOLDEN)
    names = [str(n) for n in z["base_names"]]
    off = z["base_off"]
    bases = {n: z["base_bytes"][off[i]:off[i + 1]].tobytes() for i, n in enumerate(names)}
    return z, names, bases
