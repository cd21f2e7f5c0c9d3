"""CPU: ocf_predict_entries in the C ABI (declared, mirrored, laid out as gcc lays it out), its argument checks
(every refusal has its own message and happens before any launch), and the Python surface above it.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from omnidirectional_collaborative_filtering_amd import _lib
from test_abi import HDR, declared_functions


def test_header_declares_predict_entries():
    assert "ocf_predict_entries" in declared_functions() and "ocf_predict_entries" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["ocf_predict_entries"]
    assert res is ctypes.c_int and args[0] is ctypes.POINTER(_lib.OcfPredictArgs)
    assert hasattr(_lib.load(), "ocf_predict_entries")


def test_predict_args_layout_matches_c():
    fields = [f for f, _ in _lib.OcfPredictArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void) {",
             'printf("size %zu\\n", sizeof(OcfPredictArgs));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(OcfPredictArgs, %s));' % (f, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        with open(c, "w") as fh:
            fh.write("\n".join(lines))
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert ctypes.sizeof(_lib.OcfPredictArgs) == got["size"]
    for f in fields:
        assert getattr(_lib.OcfPredictArgs, f).offset == got[f], f


def _good():
    a = _lib.OcfPredictArgs()
    for f in ("rows", "rp", "col", "val", "lboff", "flag", "ch_row", "ch_j0", "ch_j1", "h", "W", "bias", "y",
              "chunk_stats", "row_stats", "total"):
        setattr(a, f, 1)                  # never dereferenced: every call below is refused
    a.n_chunks, a.B, a.Bp = 10, 100, 128
    a.h_dtype = a.w_dtype = _lib.DT_F16
    a.H = a.ldh = a.ldw = 512
    a.aux = 1.0
    return a


@pytest.mark.parametrize("change, message", [
    (dict(h=None), "null h"),
    (dict(W=None), "null W"),
    (dict(bias=None), "null bias"),
    (dict(y=None), "null y"),
    (dict(lboff=None), "null lboff"),
    (dict(H=0), r"multiple of 128 in \[128, 2048\]"),
    (dict(H=500), r"multiple of 128 in \[128, 2048\]"),
    (dict(H=2176, ldh=2176, ldw=2176), r"multiple of 128 in \[128, 2048\]"),
    (dict(w_dtype=_lib.DT_F32, w_blocked=1), "blocked flag needs a 16-bit weight"),
    (dict(clip=1, clip_lo=5.0, clip_hi=0.5), "clip needs clip_lo <= clip_hi"),
    (dict(val=None), "row_stats given without val, chunk_stats or total"),
    (dict(chunk_stats=None), "row_stats given without val, chunk_stats or total"),
    (dict(total=None), "row_stats given without val, chunk_stats or total"),
    (dict(w_dtype=7), "h_dtype and w_dtype"),
    (dict(ldw=256), "must be >= H"),
    (dict(B=200), "0 <= B <= Bp"),
    (dict(col=None), "chunks given without"),
])
def test_refusals_have_their_own_message(change, message):
    a = _good()
    for key, v in change.items():
        setattr(a, key, v)
    with pytest.raises(_lib.OcfError, match=message):
        _lib.call("ocf_predict_entries", a, None)


def test_refusal_messages_are_distinct():
    """the five cases the interface names each answer with a message of their own"""
    msgs = []
    for change in (dict(h=None), dict(W=None), dict(bias=None), dict(y=None), dict(lboff=None), dict(H=500),
                   dict(w_dtype=_lib.DT_F32, w_blocked=1), dict(clip=1, clip_lo=1.0, clip_hi=0.0), dict(val=None)):
        a = _good()
        for key, v in change.items():
            setattr(a, key, v)
        with pytest.raises(_lib.OcfError) as e:
            _lib.call("ocf_predict_entries", a, None)
        msgs.append(str(e.value))
    assert len(set(msgs)) == len(msgs), msgs
    with pytest.raises(_lib.OcfError, match="null arguments"):
        _lib.call("ocf_predict_entries", None, None)


def test_python_surface():
    from omnidirectional_collaborative_filtering_amd import train
    from omnidirectional_collaborative_filtering_amd.engine import Engine
    from omnidirectional_collaborative_filtering_amd.model import Model
    assert callable(Model.predict_entries) and callable(Engine.predict_entries)
    for key in ("save_test_predictions", "clip_predictions"):
        assert key in train.DEFAULTS and train.DEFAULTS[key] is None
