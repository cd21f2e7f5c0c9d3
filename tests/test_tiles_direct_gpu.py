"""The encoder over column tiles, called directly through the library's C entry point (ocf_encoder_tiles, both the
packed form and the per-row chain) on the hand-built calls of tests/tiles_ref.py, against its NumPy fp64
reference under epilogue_ref.product_tol: one tile per split up to twelve, 1 to 10 splits (a second round of XCD
groups, an empty split), H = 128 / 256 / 384 / 512 with ldw > H and NaN beyond H, Bp = 384 (half a row group),
rows[b] = -1 and zero-length rows inside the batch, B = 0, a row over 1,024 entries, a tile whose bucket holds over
1,024 words with twelve rows over 8 entries (both slow paths at a known place, the tile after it clean),
duplicates with several nonzero values, inexact values (round to nearest even).

Every element of part[:Bp, :S, :H] is compared per split; rows >= B, -1 rows, zero-length rows and empty splits
must be exactly 0.  `part` is the front of a NaN-filled buffer with a tail of 256 S H floats and the workspace is
exactly ocf_encoder_tiles_workspace bytes at the front of a 0xFF-filled buffer: both tails must come back bit for
bit.  The two forms must agree bit for bit on the half-integer cases (the same X image, the same MFMAs in the same
order), a reused workspace must not change a result, ocf_rows_reduce (RAW, row_cptr[b] = b splits) must equal the
in-order float32 sum of the device partials, and every host-side argument check must raise before any launch.
tests/test_tiles_ref.py shows on the CPU that the bound rejects ten plausible bugs.

Worst observed |err| / bound per (dtype, form) over all cases (MI355X, this file's own run; recorded, not used to
set the bound):

    dtype             packed   per-row    worst case
    f16                0.165     0.165    rounding   (half-integer cases: 0.116, empty_split)
    bf16               0.119     0.119    rounding   (half-integer cases: 0.066, xcd_round2)
    (the two forms give the same figure in every case: they agree bit for bit; the longest splits sit lowest,
    long_split 0.023 / 0.017: the bound grows with the (row, split)'s nonzero products, the error much slower)
    Bit-for-bit comparisons (the two forms, the reused workspace, the row reduction, both tails): no mismatch.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tiles_ref as T
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

CD = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
NAN_BITS = 0x7FC00000                    # torch.full(.., nan) in float32
WORK_TAIL = 4096                         # bytes of 0xFF kept after the workspace


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def tune(key, value):
    prev = _lib.I32(0)
    _lib.call("ocf_set_tuning", key, int(value), ctypes.byref(prev))
    return prev.value


@functools.lru_cache(maxsize=None)
def device_case(name, wt):
    """one case's inputs on the device (shared by the tests, never written); validated first"""
    c = T.make_case(name)
    T.validate(c)
    bits, _ = T.weights_for(name, wt)
    assert bits.shape == (c.n_tiles * T.BK, c.ldw)
    rows = c.rows if c.B else np.full(1, -1, np.int32)                 # (a non-null pointer for B = 0: never read)
    t = SimpleNamespace(rows=dev(rows), rp=dev(c.rp), tptr=dev(c.tptr), tcol=dev(c.tcol), tlidx=dev(c.tlidx),
                        lboff=dev(c.lboff), xval=dev(c.xval), W=dev(bits))
    return SimpleNamespace(c=c, wt=wt, t=t)


def tile_args(d, part, work=None, work_bytes=0, kw=None):
    c, t = d.c, d.t
    a = _lib.OcfEncTileArgs()
    a.rows, a.rp, a.tptr, a.tcol, a.tlidx = (x.data_ptr() for x in (t.rows, t.rp, t.tptr, t.tcol, t.tlidx))
    a.lboff, a.xval, a.W = t.lboff.data_ptr(), t.xval.data_ptr(), t.W.data_ptr()
    a.ldw, a.w_dtype, a.B, a.Bp, a.n_tiles, a.H, a.splits = c.ldw, CD[d.wt], c.B, c.Bp, c.n_tiles, c.H, c.splits
    a.part, a.nnz, a.n_entries, a.max_row_len = part.data_ptr(), c.nnz, c.n_entries, c.max_row_len
    a.work, a.work_bytes = (work.data_ptr() if work is not None else None), work_bytes
    for k, v in (kw or {}).items():                        # (the argument-check tests: one field replaced)
        setattr(a, k, v)
    return a


def part_floats(c):
    return c.Bp * c.splits * c.H, T.BM * c.splits * c.H          # the partials, the tail a missing row guard would hit


def workspace_bytes(d):
    need = int(_lib.load().ocf_encoder_tiles_workspace(ctypes.byref(tile_args(d, torch.empty(1, device="cuda")))))
    assert need > 0
    return need


def new_buffers(n_part, n_tail, n_work):
    return (torch.full((n_part + n_tail,), float("nan"), device="cuda"),
            torch.full((n_work + WORK_TAIL,), 255, dtype=torch.uint8, device="cuda"))


def launch(d, pack, buf, work, need):
    """one call of the form `pack` into the front of buf / work; (host part [Bp][S][H], both tails untouched)"""
    c = d.c
    n, _ = part_floats(c)
    prev = tune(b"enc_tiles_pack", pack)
    try:
        _lib.call("ocf_encoder_tiles", tile_args(d, buf, work, need), cur_stream())
        torch.cuda.synchronize()
        _lib.call("ocf_check_async")
    finally:
        tune(b"enc_tiles_pack", prev)
    part = buf[:n].cpu().numpy().reshape(c.Bp, c.splits, c.H)
    tail_ok = bool((buf[n:].view(torch.int32) == NAN_BITS).all()) and bool((work[need:] == 255).all())
    return part, tail_ok


@functools.lru_cache(maxsize=None)
def result(name, wt, pack):
    """the case's partials from a fresh pair of buffers (cached: the comparison of the forms reuses them)"""
    d = device_case(name, wt)
    need = workspace_bytes(d)
    buf, work = new_buffers(*part_floats(d.c), need)
    part, tail_ok = launch(d, pack, buf, work, need)
    part.setflags(write=False)
    return part, tail_ok


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [1, 0], ids=["packed", "per-row"])
@pytest.mark.parametrize("wt", T.DTYPES)
@pytest.mark.parametrize("name", T.NAMES)
def test_partials_against_fp64(gpu, name, wt, pack):
    c = T.make_case(name)
    part, tail_ok = result(name, wt, pack)
    r, i = T.check(c, wt, part)
    print("TILES_RATIO %s | %d | %s | %.4g at %s" % (wt, pack, name, r, i))
    assert np.isfinite(part).all(), (name, np.argwhere(~np.isfinite(part))[:4].tolist())
    assert r <= 1.0, "%s %s pack=%d: worst |err| / bound %.4g at [b, s, h] = %s" % (name, wt, pack, r, i)
    # exact zeros: rows >= B, -1 rows, zero-length rows, empty splits
    assert not part[T.zero_rows(c)].any()
    for s in range(c.splits):
        t0, t1 = T.split_range(c, s)
        if t0 == t1:
            assert not part[:, s].any()
    assert tail_ok, "the NaN tail after part or the bytes after the workspace were written"


@pytest.mark.gpu
@pytest.mark.parametrize("wt", T.DTYPES)
@pytest.mark.parametrize("name", T.EXACT_NAMES)
def test_the_two_forms_agree_bit_for_bit(gpu, name, wt):
    packed, _ = result(name, wt, 1)
    per_row, _ = result(name, wt, 0)
    same = packed.view(np.int32) == per_row.view(np.int32)
    assert same.all(), (name, wt, int((~same).sum()), np.argwhere(~same)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [1, 0], ids=["packed", "per-row"])
def test_reused_workspace(gpu, pack):
    """deep7, short_last, deep7 on the same workspace and part buffers: the third result is the first's"""
    wt = "f16"
    ds = [device_case(n, wt) for n in ("deep7", "short_last")]
    needs = [workspace_bytes(d) for d in ds]
    sizes = [part_floats(d.c) for d in ds]
    buf, work = new_buffers(max(n + t for n, t in sizes), 0, max(needs))
    out = []
    for k in (0, 1, 0):
        buf.fill_(float("nan"))
        work[needs[k]:].fill_(255)                         # (what lies inside the workspace stays: the other call's)
        part, tail_ok = launch(ds[k], pack, buf, work, needs[k])
        assert tail_ok
        r, i = T.check(ds[k].c, wt, part)
        assert r <= 1.0, (ds[k].c.name, r, i)
        out.append(part)
    assert np.array_equal(out[0].view(np.int32), out[2].view(np.int32))
    assert np.array_equal(out[0].view(np.int32), result("deep7", wt, pack)[0].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["short_last", "long_split"])
def test_rows_reduce_pairing(gpu, name):
    """ocf.h's pairing: ocf_rows_reduce RAW with row_cptr[b] = b * splits = the in-order float32 sum of the partials"""
    wt = "bf16"
    c = T.make_case(name)
    part, _ = result(name, wt, 1)
    dpart = dev(part)
    cptr = torch.arange(0, (c.Bp + 1) * c.splits, c.splits, device="cuda", dtype=torch.int32)
    out = torch.full((c.Bp, c.H), float("nan"), device="cuda")
    r = _lib.OcfRowsReduceArgs()
    r.part, r.row_cptr, r.B, r.Bp, r.H, r.mode, r.out = (dpart.data_ptr(), cptr.data_ptr(), c.B, c.Bp, c.H,
                                                         _lib.REDUCE_RAW, out.data_ptr())
    _lib.call("ocf_rows_reduce", r, cur_stream())
    torch.cuda.synchronize()
    _lib.call("ocf_check_async")
    want = np.zeros((c.Bp, c.H), np.float32)
    for s in range(c.splits):
        want[:c.B] = want[:c.B] + part[:c.B, s]
    got = out.cpu().numpy()
    same = got.view(np.int32) == want.view(np.int32)
    assert same.all(), (name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


BAD_ARGS = {
    "w_dtype f32": (None, dict(w_dtype=_lib.DT_F32)),
    "H = 192": (None, dict(H=192)),
    "ldw < H": (None, dict(ldw=120)),
    "ldw % 8 != 0": (None, dict(ldw=132)),
    "Bp = 200": (None, dict(Bp=200)),
    "B > Bp": (None, dict(B=257)),
    "splits = 0": (None, dict(splits=0)),
    "n_tiles = 0": (None, dict(n_tiles=0)),
    "nnz = 0": (None, dict(nnz=0)),
    "n_entries = 0": (None, dict(n_entries=0)),
    "1,025 tiles in one split": (None, dict(n_tiles=1025, splits=1)),
    "packed: work = NULL": (1, dict(work=None)),
    "packed: work_bytes one short": (1, "short"),
    "packed: max_row_len = 0": (1, dict(max_row_len=0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_argument_checks_raise_before_any_launch(gpu, what):
    """host-side only: _lib.OcfError and the NaN-filled part untouched (no_rows: B = 0, so even a kernel that did
    run would read no entry)"""
    pack, kw = BAD_ARGS[what]
    d = device_case("no_rows", "f16")
    need = workspace_bytes(d)
    buf, work = new_buffers(*part_floats(d.c), need)
    if kw == "short":
        kw = dict(work_bytes=need - 1)
    for p in ((1, 0) if pack is None else (pack,)):
        prev = tune(b"enc_tiles_pack", p)
        try:
            with pytest.raises(_lib.OcfError):
                _lib.call("ocf_encoder_tiles", tile_args(d, buf, work, need, kw), cur_stream())
        finally:
            tune(b"enc_tiles_pack", prev)
        torch.cuda.synchronize()
        _lib.call("ocf_check_async")
        assert bool((buf.view(torch.int32) == NAN_BITS).all()) and bool((work == 255).all())
    # (the same arguments, unchanged, are accepted)
    launch(d, 1, buf, work, need)


@pytest.mark.gpu
def test_workspace_size_checks(gpu):
    d = device_case("no_rows", "f16")
    one = torch.empty(1, device="cuda")
    size = lambda **kw: int(_lib.load().ocf_encoder_tiles_workspace(ctypes.byref(tile_args(d, one, kw=kw))))
    assert size() > 0 and size() % 256 == 0
    assert size(n_tiles=0) == -1 and size(n_entries=-1) == -1
    assert int(_lib.load().ocf_encoder_tiles_workspace(None)) == -1
