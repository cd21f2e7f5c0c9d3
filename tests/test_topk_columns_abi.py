"""CPU: the transposed call of ocf_topk (per-column top-K).  The fields appended to OcfTopkArgs are declared and
mirrored, laid out as gcc lays them out, behind the earlier fields whose offsets have not moved; every new refusal
has its own message and comes before any launch; a zeroed new part is judged exactly as the struct was before; the
Model / Engine surface exists.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from omnidirectional_collaborative_filtering_amd import _lib
from test_abi import HDR
from test_topk_abi import _good, _set

# every field of OcfTopkArgs before the transposed call, with its offset then (x86-64 / LP64)
OLD_OFFSETS = [
    ("compute_dtype", 0), ("h", 8), ("ldh", 16), ("W", 24), ("w_dtype", 32), ("ldw", 40), ("w_blocked", 48),
    ("bias", 56), ("M", 64), ("N", 68), ("K", 72), ("m_real", 76), ("n_real", 80), ("k", 84), ("groups", 88),
    ("ex_rows", 96), ("ex_rp", 104), ("ex_tptr", 112), ("ex_col", 120), ("ex_ntiles", 128), ("ex_mask", 136),
    ("ld_ex", 144), ("ex_mrows", 152), ("out_idx", 160), ("out_val", 168), ("ld_out", 176), ("work", 184),
    ("work_bytes", 192), ("rel_rows", 200), ("rel_rp", 208), ("rel_col", 216), ("rel_val", 224), ("rel_min", 232),
    ("row_rank", 240),
]
NEW_FIELDS = ["bias_by_row", "h_dtype1", "h_blocked"]


def _c_layout(fields):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void) {",
             'printf("size %zu\\n", sizeof(OcfTopkArgs));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(OcfTopkArgs, %s));' % (f, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}


def test_new_fields_are_appended_and_old_offsets_unchanged():
    fields = [f for f, _ in _lib.OcfTopkArgs._fields_]
    assert fields == [f for f, _ in OLD_OFFSETS] + NEW_FIELDS
    got = _c_layout(fields)                                  # compiles only if the header declares every field
    assert ctypes.sizeof(_lib.OcfTopkArgs) == got["size"]
    for f in fields:
        assert getattr(_lib.OcfTopkArgs, f).offset == got[f], f
    for f, off in OLD_OFFSETS:
        assert got[f] == off, f
    assert min(got[f] for f in NEW_FIELDS) >= 248            # behind row_rank (240 + 8)


def _good_t():
    """the transposed call's arguments in a form that passes every check up to the workspace"""
    a = _good(B=20096, N=512, K=512)
    a.n_real, a.m_real = 500, 20000
    a.bias_by_row, a.h_dtype1, a.h_blocked = 1, _lib.DT_F16 + 1, 1
    return a


@pytest.mark.parametrize("change, message", [
    (dict(bias=None), "bias_by_row needs a bias of M values"),
    (dict(h_dtype1=_lib.DT_F32 + 1), "blocked h needs a 16-bit operand"),
    (dict(compute_dtype=_lib.DT_F32, w_dtype=_lib.DT_F32, h_dtype1=0), "blocked h needs a 16-bit operand"),
    (dict(ldh=544), "blocked h needs ldh % 64 == 0"),
    (dict(h_dtype1=_lib.DT_BF16 + 1), "h must be fp32 or the compute dtype"),
    (dict(h_dtype1=7), "h must be fp32 or the compute dtype"),
    (dict(h_dtype1=-1), "h must be fp32 or the compute dtype"),
])
def test_new_refusals_have_their_own_message(change, message):
    a = _set(_good_t(), **change)
    with pytest.raises(_lib.OcfError, match=message):
        _lib.call("ocf_topk", a, None)


def test_new_messages_are_distinct():
    src = open(os.path.join(os.path.dirname(HDR), "..", "omnidirectional_collaborative_filtering_amd", "csrc",
                            "ocf_topk.hip")).read()
    for m in ("bias_by_row needs a bias of M values", "a blocked h needs a 16-bit operand",
              "blocked h needs ldh % 64 == 0", "h must be fp32 or the compute dtype"):
        assert src.count(m) == 1, m


@pytest.mark.parametrize("new", [dict(), dict(bias_by_row=1), dict(h_dtype1=_lib.DT_F16 + 1), dict(h_dtype1=1),
                                 dict(h_blocked=1), dict(bias_by_row=1, h_dtype1=1)])
def test_good_arguments_reach_the_workspace_check(new):
    """a zeroed new part is accepted exactly as before, and so is every valid setting of it: the first refusal is
    the workspace's, the last check before the launches"""
    lib = _lib.load()
    a = _set(_good(), **new)
    need = lib.ocf_topk_workspace(ctypes.byref(a))
    assert need == lib.ocf_topk_workspace(ctypes.byref(_good())) > 0      # the new fields do not enter the formula
    a.work_bytes = need - 1
    with pytest.raises(_lib.OcfError, match="work_bytes too small"):
        _lib.call("ocf_topk", a, None)


def test_zeroed_new_part_is_refused_exactly_as_before():
    for change, message in [(dict(bias=None), "null h, W, bias, out_idx or out_val"), (dict(ldh=500), "multiples of 8"),
                            (dict(w_dtype=_lib.DT_F32, w_blocked=1), "blocked flag needs a 16-bit weight")]:
        with pytest.raises(_lib.OcfError, match=message):
            _lib.call("ocf_topk", _set(_good(), **change), None)


def test_workspace_of_a_large_m_is_64_bit():
    """M = 480,256 rows (Netflix's columns), k = 128, one group: 491 MB, past 2^31 / 8 entries x 8 bytes"""
    lib = _lib.load()
    a = _good(B=480256, N=17792, K=512, k=128, groups=0)
    assert lib.ocf_topk_workspace(ctypes.byref(a)) == 256 + 480256 * 1 * 128 * 8
    a = _good(B=480256, N=17792, K=512, k=128, groups=139)
    assert lib.ocf_topk_workspace(ctypes.byref(a)) == 256 + 480256 * 139 * 128 * 8     # 68 GB: > 2^32


def test_surface():
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.dataset import FixedSplit, RatingsCSR
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from omnidirectional_collaborative_filtering_amd.model import Model
    for name in ("encode_rows", "recommend_columns", "evaluate_ranking_columns"):
        assert callable(getattr(Model, name))
        assert "ZeRO-1" in getattr(Model, name).__doc__
    assert callable(Engine.encode_rows) and callable(Engine.topk_columns)
    assert callable(RatingsCSR.transposed) and callable(FixedSplit.catalogue) and callable(data_reader.catalogue)
