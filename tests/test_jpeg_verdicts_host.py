"""CPU: the recorded verdicts of the JPEG host passes (tests/golden/jpeg_verdicts.npz, tools/make_golden_jpeg.py).  Every entry
point of lemon_amd/jpeg_host.py must give every base file and every mutant the status, the Info fields and the packet / record
bytes (by SHA-256) it gave when the table was recorded; and a packet whose Huffman specification was overwritten must get the
recorded status from the looped-device passes."""
import numpy as np
import pytest

from tests import jpegverdictfx as fx


@pytest.fixture(scope="module")
def golden():
    return fx.load_golden()


def test_the_table_is_not_trivial(golden):
    z, names, bases = golden
    assert len(names) >= 12 and [str(e) for e in z["entry_points"]] == list(fx.ENTRY_POINTS)
    assert [str(f) for f in z["info_fields"]] == list(fx.INFO_FIELDS)
    prog = np.array([names[b].startswith("prog_") for b in z["mut_base"]])
    native = np.where(prog, z["status"][:, fx.ENTRY_POINTS.index("prog_entropy")], z["status"][:, fx.ENTRY_POINTS.index("entropy")])
    count = np.bincount(native, minlength=18)
    assert all(count[s] >= 20 for s in (0, 8, 10, 11)) and all(count[s] >= 1 for s in (9, 15, 17)), count
    assert count.max() <= 0.7 * len(native), count
    assert min(np.bincount(z["mut_base"])) >= 150                       # a few hundred mutants per base


def test_every_entry_point_gives_every_case_its_recorded_verdict(golden):
    z, names, bases = golden
    status, info, digest_idx, digests = z["status"], z["info"], z["digest_idx"], z["digests"]
    for k, (b, ops) in enumerate(zip(z["mut_base"], z["mut_ops"])):
        st, fields, dg = fx.evaluate(fx.apply(bases[names[b]], ops.tolist()))
        for e, entry in enumerate(fx.ENTRY_POINTS):
            where = (k, names[b], ops[ops[:, 1] >= 0].tolist(), entry)
            assert st[e] == status[k, e], (where, st[e], int(status[k, e]))
            assert fields[e] == info[k, e].tolist(), (where, fields[e], info[k, e].tolist())
            want = digests[digest_idx[k, e]].tobytes() if digest_idx[k, e] >= 0 else None
            assert dg[e] == want, (where, "the bytes written differ")


def test_tampered_table_packets_get_their_recorded_status(golden):
    from lemon_amd import jpeg_host
    z, names, bases = golden
    want = dict(zip((str(n) for n in z["tamper_names"]), z["tamper_status"].tolist()))
    seen = 0
    for name in fx.TAMPER_BASES:
        record_bytes = jpeg_host.info(bases[name], progressive=True).record_bytes
        for tname, pk in fx.tampered_packets(name, bases[name]):
            before = pk.copy()
            st, _ = fx.tampered_status(tname, pk, record_bytes)
            assert st == want[tname], (tname, st, want[tname])
            # as recorded at the parent: the baseline pass refuses the packet, the progressive one names the table
            assert st == (8 if name.startswith("prog_") else 13), (tname, st)
            assert np.array_equal(pk, before), tname
            seen += 1
    assert seen == len(want) >= 16
