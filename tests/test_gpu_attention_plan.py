"""GPU: the attention entries launch the kernel the plan names.  For rows of tests/golden/attention_plan.txt (the decisions recorded
from the dispatchers of commit 974b7fe, see tests/test_attention_plan_host.py) the entry is called with the row's knobs on random
qkv, B = 2 sequences of H = 2 heads, and must return the row's code and leave the row's kernel in lemon_attention_last_kernel().
No value is compared here: the test_gpu_attention_{short,long,hd,varlen}.py suites own that -- but the staged, general and
streaming forms give the same bits by design, so only this test notices a call that went to the wrong one of them."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from .test_attention_plan_host import table_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H = 2, 2
FORMS = ("f32", "split3", "f16x3", "f16x3t")


def _case(entry, split, seq_len, head_dim=64, arithmetic=1, stream_min=288, head_dims=0, short_off=0, old_general=0, batch=B):
    return f"{entry} {split} {seq_len} {head_dim} {H} {arithmetic} {stream_min} {head_dims} {short_off} {old_general} {batch}"


def _cases():
    """the launched rows (the output form rotates through the list) -> [case]"""
    rows = [("plain", L, dict(arithmetic=a)) for a in (0, 1) for L in (32, 33, 64, 65, 160, 161, 256, 257, 288, 289, 577)]
    rows += [("plain", L, dict(arithmetic=a, stream_min=64)) for a in (0, 1) for L in (65, 288)]
    rows += [("plain", 100, dict(arithmetic=2))]
    rows += [("plain", L, dict(head_dim=hd, head_dims=1)) for hd in (72, 96, 104, 128) for L in (50, 289)]
    rows += [("plain", 50, dict(head_dims=2))]
    rows += [("varlen", L, dict(arithmetic=a)) for a in (0, 1, 2) for L in (32, 64, 65, 161, 288)]
    return [_case(entry, i % 4, L, **kw) for i, (entry, L, kw) in enumerate(rows)]


CASES = _cases()
# each of the eight entries: a launch, then a refused call and a batch == 0 call, which must leave the name alone
QUIET = [(_case(entry, split, 65), _case(entry, split, 65, head_dim=60), _case(entry, split, 65, batch=0))
         for entry in ("plain", "varlen") for split in range(4)]
# the two knobs of the environment, in a child process
ENV_CASES = [_case(entry, 0, L, short_off=1, old_general=1) for entry in ("plain", "varlen") for L in (33, 100)]


@pytest.fixture(scope="module")
def table():
    return dict(table_rows())


def _call(lib, case):
    """the case's knobs, one call through the C ABI, the knobs restored -> (return code, last kernel)"""
    f = case.split()
    entry, (split, L, hd, heads, arith, smin, hdm, _, _, batch) = f[0], map(int, f[1:])
    W = heads * hd
    rows = max(batch, 1) * L
    torch.manual_seed(L + hd)
    qkv = torch.randn(max(batch, 1), L, 3 * W, device="cuda")
    out = torch.zeros((rows + 127) // 128 * 128 * W * 12, dtype=torch.uint8, device="cuda")     # room for every output form
    lengths = torch.full((max(batch, 1),), max(L - 3, 1), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    prev = lib.lemon_attention_set_f16(arith), lib.lemon_attention_set_stream_min(smin), lib.lemon_attention_set_head_dims(hdm)
    try:
        if entry == "varlen":
            rc = getattr(lib, f"lemon_attention_{FORMS[split]}_varlen")(p(qkv), batch, L, heads, hd, p(lengths), p(out), stream)
        else:
            rc = getattr(lib, f"lemon_attention_{FORMS[split]}")(p(qkv), batch, L, heads, hd, 0, p(out), stream)
        torch.cuda.synchronize()
    finally:
        lib.lemon_attention_set_f16(prev[0])
        lib.lemon_attention_set_stream_min(prev[1])
        lib.lemon_attention_set_head_dims(prev[2])
    return rc, lib.lemon_attention_last_kernel().decode("ascii")


def _expect(table, case):
    """the table's row -> (return code, kernel or None, message or None)"""
    row = table[case]
    if row.startswith("refused "):
        return int(row.split()[1]), None, row.split(" ", 2)[2]
    return 0, None if row == "nothing" else row.rsplit(" ", 5)[0], None


@pytest.mark.parametrize("case", CASES)
def test_the_entry_launches_the_kernel_the_table_names(hip, table, case):
    from lemon_amd import _lib
    rc, kernel, _ = _expect(table, case)
    assert rc == 0 and kernel
    assert _call(_lib.load(), case) == (0, kernel)


@pytest.mark.parametrize("launched,refused,empty", QUIET)
def test_a_refused_call_and_an_empty_batch_leave_the_name_alone(hip, table, launched, refused, empty):
    from lemon_amd import _lib
    lib = _lib.load()
    kernel = _expect(table, launched)[1]
    assert kernel and _call(lib, launched) == (0, kernel)
    rc, none, message = _expect(table, refused)
    assert rc == -1 and none is None
    assert _call(lib, refused) == (rc, kernel) and lib.lemon_last_error().decode() == message
    assert _expect(table, empty) == (0, None, None) and _call(lib, empty) == (0, kernel)


_CHILD = r"""
import json, sys
from tests.test_gpu_attention_plan import _call
from lemon_amd import _lib
lib = _lib.load()
assert lib.lemon_attention_last_kernel() == b""
print(json.dumps([_call(lib, case) for case in json.loads(sys.argv[1])]))
"""


def test_the_environment_knobs_reach_the_plain_entries_only(hip, table):
    # LEMON_ATTN_SHORT=0 and LEMON_ATTN_GENERAL=old are read once per process: a fresh child.  The plain entry runs the general
    # fp16 form at both lengths, the varlen entry its short and staged forms as if the knobs were unset.
    env = dict(os.environ, LEMON_ATTN_SHORT="0", LEMON_ATTN_GENERAL="old")
    run = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(ENV_CASES)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(g) for g in json.loads(run.stdout.splitlines()[-1])]
    assert got == [(0, _expect(table, case)[1]) for case in ENV_CASES]
    assert [k for _, k in got] == ["k_attention_hd64<0, true>", "k_attention_hd64<0, true>", "k_attnvl_short<2, 0, true>", "k_attnvl_f16<0>"]
