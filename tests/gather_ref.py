"""NumPy fp64 restatements of the sparse row gathers (include/ocf.h OcfGatherArgs / OcfRowsReduceArgs,
csrc/ocf_sparse.hip): the encoder's chunk sums, the row reduction in its three modes, the decoder's per-entry
forward / loss / delta, its hidden-delta sums and its stats; the small hand-built batch the GPU tests launch
them on (tests/test_gathers_gpu.py), the error bounds of every stage, a float32 restatement that sums in the
kernels' order (`twin`) and a list of deliberately wrong variants of it.  tests/test_gather_ref.py shows on the
CPU that the bounds accept the float32 restatement and reject every wrong variant.

Bounds (u = 2^-24, nothing tuned):
  * a sum of n fp32 products accumulated in fp32 in any order, then c partial sums (or a bias) added:
    |got - ref| <= 1.01 (n + c + 2) u sum|terms|  (recursive summation, gamma_k <= 1.01 k u for k u < 0.01; an
    FMA only removes roundings; added zeros are exact; the "+ 2" covers a following product or difference whose
    result is no larger than sum|terms|, such as the decoder's m * (.) and its - t when |t| <= sum|terms|, and
    is otherwise slack);
  * an activation: its Lipschitz constant (1/4 sigmoid, else 1) times the input's bound, plus 4 fp32 ulp of the
    output (epilogue_ref.product_tol's term for __expf / tanhf); grad-activation: the input's bound times
    |mask / keep * act'(a)| plus 4 u |ref| (the bar of test_epilogues_gpu.py's grad_refs);
  * a store in the compute dtype: epilogue_ref.round_tol.
Two places need one more term, each argued where it is added: tanh' = 1 - a a near saturation (check_delta_rows)
and the count of t + y != 0 at entries whose |t + y| lies within y's own bound (dec_stats).
Every stage's reference takes the previous stage's DEVICE output (the partials for the reduction, a / mask / h
for the decoder, delta_e for the hidden-delta sums), so no stage inherits another's rounding.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import epilogue_ref as R
import loss_ref as L

U = 2.0 ** -24
ULP4 = 4.0 * 2.0 ** -23                  # "4 fp32 ulp of the output" (epilogue_ref.product_tol)
HUBER_DELTA = 1.0
LOSS_CODE = {"mse": 0, "mae": 1, "huber": 2, "logcosh": 3}          # ocf.h OCF_LOSS_*
N_COLS, N_PAD = 1000, 1024               # real columns; weight rows (a multiple of 64: the blocked layout)
B_REAL, B_PADROWS = 20, 3
KEEP = 0.8
KEEP32 = float(np.float32(KEEP))
GSCALE = float(np.float32(R.GSCALE))
CHUNK_OF = {128: 64, 256: 96, 384: 64, 512: 256}
ESIZE = {"f32": 4, "f16": 8, "bf16": 8}  # elements of a 16-byte piece
LIP = {"sigmoid": 0.25, "tanh": 1.0, "relu": 1.0, "linear": 1.0}

# batch rows with a fixed role (make_batch)
ROW_LONG, ROW_NONE, ROW_EMPTY, ROW_1, ROW_7, ROW_255, ROW_256, ROW_257, ROW_NOIN, ROW_NOTGT, ROW_DUP = range(11)
FIXED_LENS = {ROW_LONG: 700, ROW_NONE: 0, ROW_EMPTY: 0, ROW_1: 1, ROW_7: 7, ROW_255: 255, ROW_256: 256, ROW_257: 257,
              ROW_NOIN: 40, ROW_NOTGT: 30, ROW_DUP: 50}

# the instance grid: every compiled (weight type, G, PPL) of gather_shape
GRID = ([(wt, H, bl) for wt in ("f16", "bf16") for H in (128, 256, 384, 512) for bl in (0, 1)] +
        [("f32", H, 0) for H in (128, 256, 384, 512)])
GRID_IDS = ["%s-H%d-%s" % (wt, H, "blocked" if bl else "rowmajor") for wt, H, bl in GRID]
# the losses other than MSE: one 16-bit blocked and one fp32 grid point each (each loss at a point where
# ocf_gather_encdec runs row-resident: f16 512, f32 256, f16 256 / f32 512)
LOSS_CASES = [("mae", "f16", 512, 1), ("mae", "f32", 128, 0), ("huber", "bf16", 384, 1), ("huber", "f32", 256, 0),
              ("logcosh", "f16", 256, 1), ("logcosh", "f32", 512, 0)]
ALL_ACTS_AT = ("f16", 512, 1)            # the grid point that runs all four activations (sigmoid elsewhere)


def gather_shape(wt, H):
    """(G, PPL) of ocf_sparse.hip gather_shape: the widest group of <= 32 lanes the row's pieces fill"""
    pieces = H // ESIZE[wt]
    for g in (32, 16):
        if pieces % g == 0 and pieces // g <= 4:
            return g, pieces // g
    raise ValueError((wt, H))


def rowres_runs(wt, H):
    """ocf_sparse.hip rowres_shape_ok: the row-resident form takes these, the others run chunked"""
    return H % 256 == 0 if wt == "f32" else H != 384


# ---- the batch ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_batch(H, seed=5, n_cols=N_COLS, B=B_REAL, pad=B_PADROWS):
    """One small CSR and one batch of B real rows + `pad` padding rows on the kernels' edges (asserted below).
    Host arrays only; read-only for the tests (cached per H)."""
    rng = np.random.RandomState(seed + H)
    Bp = B + pad
    lens = np.array([FIXED_LENS.get(b, 0) for b in range(B)], np.int64)
    lens[len(FIXED_LENS):] = rng.randint(5, 400, size=B - len(FIXED_LENS))
    # the dataset CSR: the batch's rows in a shuffled order among a few rows the batch does not use
    n_ds = B + 6
    ds_of = rng.permutation(n_ds)[:B]
    ds_len = rng.randint(1, 50, size=n_ds)
    ds_len[ds_of] = lens
    rp = np.zeros(n_ds + 1, np.int64)
    np.cumsum(ds_len, out=rp[1:])
    col = np.zeros(rp[-1], np.int32)
    for r in range(n_ds):
        col[rp[r]:rp[r + 1]] = rng.permutation(n_cols)[:ds_len[r]]
    val = (rng.randint(1, 11, size=rp[-1]) / 2.0).astype(np.float32)           # half-stars in [0.5, 5]
    rows = np.full(Bp, -1, np.int32)
    rows[:B] = ds_of
    rows[ROW_NONE] = -1
    lens[ROW_NONE] = 0
    # the long row uses column 0, the last real column and both sides of multiples of 64
    forced = np.array([0, n_cols - 1, 63, 64, 65, 127, 128], np.int32)
    s = rp[rows[ROW_LONG]]
    rest = np.setdiff1d(col[s:s + 700], forced)[:700 - len(forced)]
    col[s:s + 700] = rng.permutation(np.concatenate([forced, rest]))
    # duplicate columns inside one row (list positions 0..2 and 47..49)
    s = rp[rows[ROW_DUP]]
    col[s + 47:s + 50] = col[s:s + 3]
    lboff = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=lboff[1:])
    E = int(lboff[-1])
    eb = np.repeat(np.arange(B), lens)                                          # batch row of each batch-local entry
    ej = np.arange(E) - lboff[eb]
    src = rp[np.maximum(rows[eb], 0)] + ej                                       # its CSR position
    ecol = col[src].astype(np.int64)
    # the engineered target: t = 0 at a live target of the row without inputs (its output bias is 0 below)
    eng = int(lboff[ROW_NOIN])
    val[src[eng]] = 0.0
    et = val[src].astype(np.float64)
    xval = np.where(rng.rand(E) < 0.7, val[src], 0.0).astype(np.float32)
    flag = (rng.rand(E) < 0.7).astype(np.uint8)
    at = lambda b: slice(int(lboff[b]), int(lboff[b + 1]))
    xval[at(ROW_NOIN)], flag[at(ROW_NOIN)] = 0.0, 1
    flag[at(ROW_NOTGT)] = 0
    xval[at(ROW_1)], flag[at(ROW_1)] = val[src[at(ROW_1)]], 1
    d0 = int(lboff[ROW_DUP])
    edge = [d0 + j for j in (0, 1, 2, 47, 48, 49)]
    edge += [i for i in range(*at(ROW_LONG).indices(E)) if ecol[i] in forced]     # both an input and a target
    for i in edge:
        xval[i], flag[i] = val[src[i]], 1
    # weights: hidden pre-activations and predictions O(1), residuals of both signs over about [-9, 4]
    W1 = (0.02 * rng.randn(N_PAD, H)).astype(np.float32)
    Wout = (0.4 / np.sqrt(H) * rng.randn(N_PAD, H)).astype(np.float32)
    bias_h = (0.1 * rng.randn(H)).astype(np.float32)
    bias_out = (1.5 * rng.randn(N_PAD)).astype(np.float32)
    bias_out[ecol[eng]] = 0.0
    h_given = rng.rand(Bp, H).astype(np.float32)                                 # the plain decoder's hidden rows
    h_given[ROW_NOIN] = 0.0
    stats_in = rng.rand(4096, 4).astype(np.float32)                              # chunk stats for the reduce tests
    fx = SimpleNamespace(H=H, B=B, Bp=Bp, n_real=H - 3, n_cols=n_cols, rows=rows, rp=rp, col=col, val=val, lboff=lboff,
                         lens=lens, E=E, eb=eb, ej=ej, ecol=ecol, et=et, xval=xval, flag=flag, W1=W1, Wout=Wout,
                         bias_h=bias_h, bias_out=bias_out, h_given=h_given, eng=eng, stats_in=stats_in)
    check_batch(fx)
    for a in vars(fx).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return fx


def check_batch(fx):
    """the edges the batch must hold, by construction"""
    at = lambda b: slice(int(fx.lboff[b]), int(fx.lboff[b + 1]))
    assert fx.rows[ROW_NONE] == -1 and (fx.rows[fx.B:] == -1).all()
    r = fx.rows[ROW_EMPTY]
    assert r >= 0 and fx.rp[r + 1] == fx.rp[r]
    assert all(fx.lens[b] == n for b, n in FIXED_LENS.items())
    assert {1, 7, 255, 256, 257, 700} <= set(fx.lens.tolist())
    assert not fx.xval[at(ROW_NOIN)].any() and fx.flag[at(ROW_NOIN)].all()
    assert not fx.flag[at(ROW_NOTGT)].any() and fx.xval[at(ROW_NOTGT)].any()
    free = np.ones(fx.E, bool)
    for b in (ROW_NOIN, ROW_NOTGT, ROW_1, ROW_DUP):
        free[at(b)] = False
    assert 0.2 < (fx.xval[free] == 0).mean() < 0.4 and 0.2 < (fx.flag[free] == 0).mean() < 0.4
    both = (fx.xval != 0) & (fx.flag != 0)
    assert 0.3 < both[free].mean() < 0.7                        # inputs and targets overlap
    c = fx.ecol[at(ROW_DUP)]
    assert len(np.unique(c)) == len(c) - 3 and both[at(ROW_DUP)][[0, 1, 2, 47, 48, 49]].all()
    for b in range(fx.B):
        if b != ROW_DUP:
            assert len(np.unique(fx.ecol[at(b)])) == fx.lens[b]
    used = set(fx.ecol[both].tolist())
    assert {0, fx.n_cols - 1, 63, 64, 65, 127, 128} <= used and fx.ecol.max() == fx.n_cols - 1
    assert fx.et[fx.eng] == 0 and fx.flag[fx.eng] and fx.bias_out[fx.ecol[fx.eng]] == 0 and not fx.h_given[ROW_NOIN].any()
    live_t = fx.et[(fx.flag != 0) & (np.arange(fx.E) != fx.eng)]
    assert live_t.min() >= 0.5 and live_t.max() <= 5.0 and (live_t * 2 == np.round(live_t * 2)).all()
    assert 3000 <= fx.E <= 6000


def chunk_tables(lens, chunk):
    """data_reader._chunk_tables for one batch: every row cut into ceil(len / chunk) chunks of equal length"""
    Ln = np.asarray(lens, np.int64)
    nc = (Ln + chunk - 1) // chunk
    row_cptr = np.zeros(len(Ln) + 1, np.int32)
    np.cumsum(nc, out=row_cptr[1:])
    rep = np.repeat(np.arange(len(Ln), dtype=np.int64), nc)
    k = np.arange(int(nc.sum()), dtype=np.int64) - np.repeat(np.cumsum(nc) - nc, nc)
    j0, j1 = k * Ln[rep] // nc[rep], (k + 1) * Ln[rep] // nc[rep]
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    return SimpleNamespace(ch_row=i32(rep), ch_j0=i32(j0), ch_j1=i32(j1), row_cptr=row_cptr, n_chunks=len(rep),
                           chunk=chunk)


@functools.lru_cache(maxsize=None)
def chunks_for(H, chunk=None):
    fx = make_batch(H)
    ct = chunk_tables(fx.lens, chunk or CHUNK_OF[H])
    # chunk of each batch-local entry
    ct.ech = np.repeat(np.arange(ct.n_chunks), ct.ch_j1 - ct.ch_j0)
    assert len(ct.ech) == fx.E and (ct.ch_j1 - ct.ch_j0).max() <= max(ct.chunk, 1)
    return ct


def pack_weights(W, dtype, blocked):
    """W [rows][H] fp32 rounded to `dtype` (torch, RNE) and laid out row-major or in ocf.h's 64x64 blocks (blocks of
    64 rows x 64 columns, each 8 KB contiguous and row-major inside, blocks row-major).  Returns the packed array
    (float32, or the 16-bit patterns as int16; [rows][H] elements) and the rounded values as float64 [rows][H]."""
    import torch
    td = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    t = torch.from_numpy(np.array(W, np.float32)).to(td)
    Wr = t.float().numpy().astype(np.float64)
    if blocked:
        assert dtype != "f32"
        n, H = W.shape
        t = t.view(n // 64, 64, H // 64, 64).permute(0, 2, 1, 3).contiguous().view(n, H)
    packed = t.numpy() if dtype == "f32" else t.view(torch.int16).numpy()
    return packed, Wr


def unpack_rows(packed, dtype, blocked, n):
    """rows n of a packed weight array as float32 [len(n)][H]: what load_piece_raw reads"""
    import torch
    rows, H = packed.shape
    n = np.asarray(n, np.int64)
    flat = packed.reshape(-1)
    if blocked:
        x = np.arange(H, dtype=np.int64)
        idx = (((n[:, None] >> 6) * (H >> 6) + (x[None, :] >> 6)) << 12) + (n[:, None] & 63) * 64 + (x[None, :] & 63)
    else:
        idx = n[:, None] * H + np.arange(H, dtype=np.int64)[None, :]
    got = flat[idx]
    if dtype == "f32":
        return got.astype(np.float32)
    td = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    return torch.from_numpy(np.ascontiguousarray(got)).view(td).float().numpy()


@functools.lru_cache(maxsize=None)
def weights_for(wt, H, blocked):
    """(packed W1, rounded W1, packed W_out, rounded W_out) of the H fixture"""
    fx = make_batch(H)
    p1, r1 = pack_weights(fx.W1, wt, blocked)
    po, ro = pack_weights(fx.Wout, wt, blocked)
    for a in (p1, r1, po, ro):
        a.setflags(write=False)
    return p1, r1, po, ro


# ---- bounds and comparisons -------------------------------------------------------------------------------
def sum_bound(n, c, mag):
    return 1.01 * (np.asarray(n, np.float64) + c + 2.0) * U * mag


def worst(got, ref, tol, mask=None):
    """(worst |got - ref| / tol, its index); a NaN (an element never written) is an infinite error, an exact
    match under a zero bound is 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.where(np.isnan(got), np.inf, np.abs(got - ref))
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    ratio = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))
    if mask is not None:
        ratio = np.where(mask, ratio, 0.0)
    if ratio.size == 0:
        return 0.0, ()
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), tuple(int(k) for k in i)


class Report(list):
    """(check, worst error / bound, index) of every comparison of a case"""

    def add(self, what, got, ref, tol, mask=None):
        r, i = worst(got, ref, tol, mask)
        self.append((what, r, i))

    def exact(self, what, got, ref, mask=None):
        """got == ref elementwise (NaN never equal)"""
        bad = ~(np.asarray(got) == np.asarray(ref))
        if mask is not None:
            bad &= mask
        i = tuple(int(k) for k in np.argwhere(bad)[0]) if bad.any() else ()
        self.append((what, np.inf if bad.any() else 0.0, i))

    def worst(self):
        return max(self, key=lambda t: t[1]) if self else ("", 0.0, ())

    def failures(self):
        return [t for t in self if not t[1] <= 1.0]


def seg_sums(seg, n_seg, terms):
    """sum of terms [E][H] and of |terms| over the entries of each segment (seg non-decreasing), and the
    segments' entry counts"""
    cnt = np.bincount(seg, minlength=n_seg).astype(np.int64)
    ref = np.zeros((n_seg,) + terms.shape[1:])
    mag = np.zeros_like(ref)
    if len(seg):
        assert (np.diff(seg) >= 0).all()
        starts = np.concatenate([[0], np.nonzero(np.diff(seg))[0] + 1])
        ref[seg[starts]] = np.add.reduceat(terms, starts, axis=0)
        mag[seg[starts]] = np.add.reduceat(np.abs(terms), starts, axis=0)
    return ref, mag, cnt


# ---- fp64 references -----------------------------------------------------------------------------------------
def enc_partials(fx, ct, Wr):
    """per chunk: sum xval_j W1[col_j][x]; (ref, sum |terms|, entries per chunk)"""
    return seg_sums(ct.ech, ct.n_chunks, fx.xval.astype(np.float64)[:, None] * Wr[fx.ecol])


def dec_partials(fx, ct, Wr, delta_e):
    """per chunk: sum delta_j W_out[col_j][x]"""
    return seg_sums(ct.ech, ct.n_chunks, np.asarray(delta_e, np.float64)[:fx.E, None] * Wr[fx.ecol])


def row_gather(fx, coef, Wr):
    """per batch row [Bp]: sum coef_j W[col_j][x] over the row's entries (the row-resident forms)"""
    return seg_sums(fx.eb, fx.Bp, np.asarray(coef, np.float64)[:fx.E, None] * Wr[fx.ecol])


def row_sum(part, row_cptr, Bp):
    """chunk partials [n_chunks][K] summed per row: (ref [Bp][K], sum |part|, chunks per row)"""
    part = np.asarray(part, np.float64)
    nB = len(row_cptr) - 1
    seg = np.repeat(np.arange(nB), np.diff(row_cptr))
    return seg_sums(seg, Bp, part[:len(seg)])


def bias_act(v, bias, act, m_real, n_real, mask=None, keep=1.0):
    """a = act(v + bias) for b < m_real, x < n_real, else 0; h = (a / keep) * mask"""
    v = np.asarray(v, np.float64)
    a = np.zeros_like(v)
    a[:m_real, :n_real] = R.act(act, v + np.asarray(bias, np.float64))[:m_real, :n_real]
    h = a if mask is None or keep >= 1.0 else R.dropout_fwd(a, mask, keep)
    return a, h


def loss_grad(loss, e):
    """rho'(e) as the decoder applies it: MSE's delta is e * m (the factor 2 lives in the gradient scale)"""
    return np.asarray(e, np.float64) if loss == "mse" else L.drho(loss, e, HUBER_DELTA)


def dec_entry(fx, h, Wr, bias, m, loss):
    """per batch-local entry: y = m (h . W_out[n] + bias[n]), e = y - t, delta = rho'(e) m at the live targets
    (0 elsewhere), with the bound of each and the entries whose reference residual lies within its own bound of
    a kink of rho' (MAE: e = 0; Huber: |e| = delta)"""
    m = float(np.float32(m))
    hb, w = np.asarray(h, np.float64)[fx.eb], Wr[fx.ecol]
    bn = np.asarray(bias, np.float64)[fx.ecol]
    live = fx.flag != 0
    y = m * ((hb * w).sum(1) + bn)
    by = abs(m) * sum_bound(fx.H, 1, (np.abs(hb) * np.abs(w)).sum(1) + np.abs(bn))
    e = y - fx.et
    be = by + U * np.abs(e)
    g = loss_grad(loss, e)
    d = np.where(live, g * m, 0.0)
    lip = 0.0 if loss == "mae" else 1.0
    bd = np.where(live, abs(m) * (lip * be + (ULP4 * np.abs(g) if loss == "logcosh" else 0.0)) + U * np.abs(d), 0.0)
    kink = np.zeros(fx.E, bool)
    if loss == "mae":
        kink = live & (np.abs(e) <= be)
    elif loss == "huber":
        kink = live & (np.abs(np.abs(e) - HUBER_DELTA) <= be)
    return SimpleNamespace(y=y, tpy=fx.et + y, by=by, e=e, be=be, d=d, bd=bd, live=live, kink=kink, loss=loss,
                           ambiguous=live & (by > 0) & (np.abs(fx.et + y) <= by))


def dec_stats(ent, seg, n_seg, n_sums=0):
    """{sum e^2, sum |e|, count(t + y != 0), sum rho(e)} over the live targets of each segment (slot 3 is 0 under
    MSE), and the bounds: each entry's propagated residual bound (2 |e| be + be^2; be; rho's Lipschitz constant 1
    times be, plus the evaluation of rho in fp32: 2 u rho for Huber's two roundings, 4 ulp of |e| + ln 2 for
    log-cosh) plus the summation bound over the segment's live entries and n_sums partial sums.  The count is
    exact but for the entries whose reference |t + y| lies within y's own bound (ent.ambiguous: each may fall
    either way; kink_share counts them with the kinks, so they stay under 1 %)"""
    lv = ent.live.astype(np.float64)
    e, be = np.abs(ent.e), ent.be
    rho = np.zeros_like(e) if ent.loss == "mse" else L.rho(ent.loss, ent.e, HUBER_DELTA)
    ev = {"mse": 0.0, "mae": 0.0, "huber": 2.0 * U * rho, "logcosh": ULP4 * (e + np.log(2.0))}[ent.loss]
    terms = np.stack([e * e, e, lv * 0.0, rho], 1) * lv[:, None]
    errs = np.stack([2.0 * e * be + be * be, be, lv * 0.0, (be + ev) * (ent.loss != "mse")], 1) * lv[:, None]
    ref, mag, _ = seg_sums(seg, n_seg, terms)
    perr, _, _ = seg_sums(seg, n_seg, errs)
    n_live = np.bincount(seg, weights=lv, minlength=n_seg)
    ref[:, 2] = np.bincount(seg, weights=lv * (ent.tpy != 0), minlength=n_seg)
    bound = perr + sum_bound(n_live[:, None], n_sums, mag)
    bound[:, 2] = np.bincount(seg, weights=ent.ambiguous, minlength=n_seg)      # exact but for those entries
    return ref, bound


# ---- the checks (shared by the GPU tests and the CPU test of the bounds) -----------------------------------------
def check_encoder(rep, fx, ct, W1r, part):
    ref, mag, n = enc_partials(fx, ct, W1r)
    rep.add("encoder: part", part, ref, sum_bound(n[:, None], 0, mag))


def check_reduce_raw(rep, fx, ct, part, out):
    ref, mag, c = row_sum(part, ct.row_cptr, fx.Bp)
    rep.add("reduce: RAW", out, ref, sum_bound(0, c[:, None], mag))


def hidden_bound(v_bound, a_ref, act):
    return LIP[act] * v_bound + ULP4 * np.abs(a_ref)


def check_hidden(rep, stage, fx, cd, act, keep, bias_h, v_ref, v_bound, a_out, mask_out, h, rows=None):
    """a_out against act(v_ref + bias) (v_bound: the bound of v + bias), mask_out 0 / 1, h against the DEVICE a_out
    and mask: one rounding to the compute dtype, with dropout after the correctly rounded fp32 division.
    rows: the batch rows the launch promises (None: all Bp)"""
    sel = np.ones(fx.Bp, bool) if rows is None else rows
    a_ref, _ = bias_act(v_ref, bias_h, act, fx.B, fx.n_real)
    rep.add(stage + ": a_out", a_out[sel], a_ref[sel], hidden_bound(v_bound, a_ref, act)[sel])
    a_dev = np.asarray(a_out, np.float64)
    if keep < 1.0:
        rep.exact(stage + ": mask is 0 / 1", np.isin(mask_out[sel], (0, 1)), True)
        want = R.dropout_fwd(a_dev, mask_out, KEEP32)
        tol = R.round_tol(cd, np.abs(want) * (1.0 + U)) + U * np.abs(want)
    else:
        want = a_dev
        tol = R.round_tol(cd, want)
    rep.add(stage + ": h", h[sel], want[sel], tol[sel])


def check_bias_act(rep, fx, ct, cd, act, keep, bias_h, part, a_out, mask_out, h, rows=None, stage="reduce"):
    """OCF_REDUCE_BIAS_ACT (and the decoder's hidden epilogue) on the device partials `part`"""
    v, mag, c = row_sum(part, ct.row_cptr, fx.Bp)
    vb = sum_bound(0, c[:, None] + 1, mag + np.abs(np.asarray(bias_h, np.float64)))
    check_hidden(rep, stage, fx, cd, act, keep, bias_h, v, vb, a_out, mask_out, h, rows)


def check_delta_rows(rep, stage, fx, cd, act, keep, v, v_bound, a_in, mask_in, h_out, db_part, raw=False):
    """the hidden delta of every row from the row sums v (bound v_bound): grad_act on the DEVICE a / mask, rounded
    to the compute dtype, zero for b >= B and x >= n_real; db_part = delta * gscale.  raw: h_out holds v itself"""
    if raw:
        rep.add(stage + ": row sums", h_out, v, v_bound)
        return
    live = np.zeros((fx.Bp, fx.H), bool)
    live[:fx.B, :fx.n_real] = True
    mk = mask_in if keep < 1.0 else None
    fac = np.where(live, np.abs(R.grad_act(act, np.ones_like(v), a_in, mk, KEEP32 if keep < 1.0 else 1.0)), 0.0)
    ref = np.where(live, R.grad_act(act, v, a_in, mk, KEEP32 if keep < 1.0 else 1.0), 0.0)
    tol32 = v_bound * fac + 4.0 * U * np.abs(ref)
    if act == "tanh":
        # act' = 1 - a * a cancels near saturation: the rounding of a * a (u a^2) is an ABSOLUTE error of act',
        # not one of the relative roundings the 4 u |ref| term counts (test_epilogues_gpu.py draws a uniformly,
        # so it never meets |a| ~ 0.999; a 500-entry row's pre-activation here does)
        a2 = np.asarray(a_in, np.float64) ** 2
        tol32 = tol32 + U * a2 * np.abs(np.where(live, R.grad_act("linear", v, a_in, mk, KEEP32 if keep < 1.0 else 1.0), 0.0))
    rep.add(stage + ": hidden delta", h_out, ref, tol32 + R.round_tol(cd, ref) * live)
    if db_part is not None:
        rep.add(stage + ": db_part", db_part, ref * GSCALE, (tol32 + U * np.abs(ref)) * GSCALE)


def check_grad_act(rep, fx, ct, cd, act, keep, part, chunk_stats, a_in, mask_in, h_out, db_part, stats_part, row_sse,
                   stats4):
    """OCF_REDUCE_GRAD_ACT on device partials and device chunk stats"""
    v, mag, c = row_sum(part, ct.row_cptr, fx.Bp)
    check_delta_rows(rep, "reduce", fx, cd, act, keep, v, sum_bound(0, c[:, None], mag), a_in, mask_in, h_out, db_part)
    s, smag, c = row_sum(chunk_stats, ct.row_cptr, fx.Bp)
    sb = sum_bound(0, c[:, None], smag)
    if not stats4:
        s[:, 3], sb[:, 3] = 0.0, 0.0
    rep.add("reduce: stats_part", stats_part, s, sb)
    rep.exact("reduce: row_sse", row_sse, np.asarray(stats_part)[:, 0])


def check_entries(rep, stage, fx, ent, delta_e, d_out, cd):
    """delta_e at every entry (exactly 0 at the entries that are no live target; the entries at a kink of rho' are
    left out), the dense delta = the DEVICE delta_e rounded to the compute dtype at the live targets (either one
    of a duplicated column's), untouched (NaN) elsewhere"""
    de = np.asarray(delta_e, np.float64)[:fx.E]
    rep.add(stage + ": delta_e", de, ent.d, ent.bd, mask=~ent.kink)
    rep.exact(stage + ": delta_e off the targets", de[~ent.live], 0.0)
    if d_out is None:
        return
    d_out = np.asarray(d_out, np.float64)
    lv = np.nonzero(ent.live)[0]
    got = d_out[fx.eb[lv], fx.ecol[lv]]
    err = np.abs(got - de[lv]) / np.maximum(R.round_tol(cd, de[lv]), 1e-300)
    err = np.where(np.isnan(got), np.inf, np.where(got == de[lv], 0.0, err))
    key = fx.eb[lv] * N_PAD + fx.ecol[lv]
    best = np.full(fx.Bp * N_PAD, np.inf)
    np.minimum.at(best, key, err)                       # duplicates: the store of either entry
    r = best[key]
    i = int(np.argmax(r)) if len(r) else 0
    rep.append((stage + ": d_out", float(r[i]) if len(r) else 0.0, (int(lv[i]),) if len(r) else ()))
    hit = np.zeros(d_out.shape, bool)
    hit[fx.eb[lv], fx.ecol[lv]] = True
    rep.exact(stage + ": d_out untouched elsewhere", np.isnan(d_out), ~hit)


def check_decoder(rep, fx, ct, cd, Woutr, h_dev, m, loss, delta_e, d_out, part, chunk_stats):
    """the plain decoder: entries, chunk partials from the DEVICE delta_e, chunk stats"""
    ent = dec_entry(fx, h_dev, Woutr, fx.bias_out, m, loss)
    check_entries(rep, "decoder", fx, ent, delta_e, d_out, cd)
    ref, mag, n = dec_partials(fx, ct, Woutr, delta_e)
    rep.add("decoder: part", part, ref, sum_bound(n[:, None], 0, mag))
    s, sb = dec_stats(ent, ct.ech, ct.n_chunks)
    rep.add("decoder: chunk_stats", np.asarray(chunk_stats)[:, :3 if loss == "mse" else 4], s[:, :3 if loss == "mse" else 4],
            sb[:, :3 if loss == "mse" else 4])
    return ent


def check_fused(rep, stage, fx, ct, cd, Woutr, act, keep, m, loss, o, raw=False):
    """the decoder with its folded / row-resident reduction, from the DEVICE a / mask / h and delta_e: entries, the
    hidden delta of every row (raw: the raw row sums), db_part, the row stats; rows without entries and padding
    rows are zero.  o: a_out, mask_out, h, delta_e, d_out, hd, db_part, stats_part, row_sse"""
    ent = dec_entry(fx, o.h, Woutr, fx.bias_out, m, loss)
    check_entries(rep, stage, fx, ent, o.delta_e, o.d_out, cd)
    v, mag, n = row_gather(fx, o.delta_e, Woutr)
    c = np.zeros(fx.Bp)
    c[:fx.B] = np.diff(ct.row_cptr)
    empty = np.ones(fx.Bp, bool)
    empty[:fx.B] = fx.lens == 0
    # (a / mask of the rows without entries are not promised; their delta is zero whatever they hold)
    a_in, mk = np.where(empty[:, None], 0.0, o.a_out), np.where(empty[:, None], 0, o.mask_out)
    check_delta_rows(rep, stage, fx, cd, act, keep, v, sum_bound(n[:, None], c[:, None], mag), a_in, mk, o.hd,
                     o.db_part, raw)
    s, sb = dec_stats(ent, fx.eb, fx.Bp, c[:, None])
    if loss == "mse":
        s[:, 3], sb[:, 3] = 0.0, 0.0
    rep.add(stage + ": stats_part", o.stats_part, s, sb)
    if o.row_sse is not None:
        rep.exact(stage + ": row_sse", o.row_sse, np.asarray(o.stats_part)[:, 0])
    rep.exact(stage + ": rows without entries are zero",
              (np.asarray(o.hd, np.float64)[empty] == 0).all() and (np.asarray(o.stats_part)[empty] == 0).all(), True)
    return ent


def check_hidden_scratch(rep, stage, fx, ct, cd, W1r, act, keep, bias_h, o, rows):
    """a_out / mask_out / h of a launch that runs the encoder itself (ocf_gather_encdec): from the entries"""
    v, mag, n = row_gather(fx, fx.xval, W1r)
    c = np.zeros(fx.Bp)
    c[:fx.B] = np.diff(ct.row_cptr)
    vb = sum_bound(n[:, None], c[:, None] + 1, mag + np.abs(np.asarray(bias_h, np.float64)))
    check_hidden(rep, stage, fx, cd, act, keep, bias_h, v, vb, o.a_out, o.mask_out, o.h, rows)


def kink_share(fx, ent):
    """share of the live targets left out of the delta comparison (a kink of rho') or of the exact count"""
    return float((ent.kink | ent.ambiguous).sum()) / max(int(ent.live.sum()), 1)


# ---- float32 restatement in the kernels' order, and its wrong variants -----------------------------------------------
WRONG = {
    1: "drops the last entry of each chunk",
    2: "drops entries past the last full (256 / G) * 4 stride of a chunk",
    3: "pieces of a PPL > 1 row in the wrong order",
    4: "blocked weights addressed as row-major",
    5: "flag ignored",
    6: "xval == 0 entries accumulated with the raw rating",
    7: "delta = e instead of e * m",
    8: "count of live entries instead of count_nonzero(t + y)",
    9: "only the first chunk of a row reduced",
    10: "dropout mask applied without / keep",
    11: "padding rows left unwritten",
    12: "fourth stats slot left 0 under a loss other than MSE",
}


def wrong_applies(k, wt, H, blocked, loss):
    if k == 3:
        return gather_shape(wt, H)[1] > 1
    if k == 4:
        return bool(blocked)
    if k == 12:
        return loss != "mse"
    return True


def _f32_loss(loss, e):
    f = np.float32
    a = np.abs(e)
    if loss == "mse":
        return e * e, e
    if loss == "mae":
        return a, np.sign(e).astype(f)
    if loss == "huber":
        d = f(HUBER_DELTA)
        return np.where(a <= d, f(0.5) * (e * e), d * (a - f(0.5) * d)).astype(f), np.clip(e, -d, d)
    return (a + np.log1p(np.exp(f(-2.0) * a)) - f(np.log(2.0))).astype(f), np.tanh(e).astype(f)


def twin(fx, ct, wt, blocked, act="sigmoid", keep=KEEP, m=-1.0, loss="mse", h_given=False, stats4=1, wrong=None,
         seed=9):
    """Every stage of the GPU tests in float32, summed as the kernels sum (each group's entries strided by the
    group count, then the groups pairwise; a row's chunks in order), with `wrong` (a key of WRONG) one
    deliberate bug.  Returns the stage outputs as a namespace of host arrays laid out like the device buffers."""
    f = np.float32
    G, PPL = gather_shape(wt, fx.H)
    NG = 256 // G
    H, B, Bp, E = fx.H, fx.B, fx.Bp, fx.E
    p1, _, po, _ = weights_for(wt, H, blocked)
    as_blocked = blocked and wrong != 4

    def rows_of(packed):
        w = unpack_rows(packed, wt, as_blocked, fx.ecol)
        if wrong == 3:
            pieces = H // ESIZE[wt]
            perm = np.empty(pieces, np.int64)
            for l in range(G):
                for i in range(PPL):
                    perm[l + G * i] = l * PPL + i
            w = w.reshape(E, pieces, -1)[:, perm].reshape(E, H)
        return w

    def chunk_sums(coef, w):
        terms = coef.astype(f)[:, None] * w
        part = np.zeros((ct.n_chunks, H), f)
        for c in range(ct.n_chunks):
            lo = int(fx.lboff[ct.ch_row[c]])
            j0, j1 = lo + int(ct.ch_j0[c]), lo + int(ct.ch_j1[c])
            if wrong == 1:
                j1 -= 1
            if wrong == 2:
                j1 = j0 + (j1 - j0) // (NG * 4) * (NG * 4)
            t = terms[j0:max(j1, j0)]
            n = -(-len(t) // NG) * NG
            t = np.concatenate([t, np.zeros((n - len(t), H), f)]).reshape(-1, NG, H)
            g = np.add.reduce(t, axis=0, dtype=f) if len(t) else np.zeros((NG, H), f)
            part[c] = np.add.reduce(g[0::2], axis=0, dtype=f) + np.add.reduce(g[1::2], axis=0, dtype=f)
        return part

    def reduce_rows(part, fill=0.0):
        out = np.full((Bp, part.shape[1]), np.nan if wrong == 11 else fill, f)
        for b in range(B):
            c0, c1 = int(ct.row_cptr[b]), int(ct.row_cptr[b + 1])
            if wrong == 9:
                c1 = min(c1, c0 + 1)
            v = np.zeros(part.shape[1], f)
            for c in range(c0, c1):
                v = v + part[c]
            out[b] = v
        return out

    o = SimpleNamespace()
    rng = np.random.RandomState(seed)
    # encoder, RAW reduction, hidden epilogue
    xin = fx.xval if wrong != 6 else np.where(fx.xval != 0, fx.xval, fx.et.astype(f))
    o.enc_part = chunk_sums(xin, rows_of(p1))
    o.enc_rows = reduce_rows(o.enc_part)
    live = np.zeros((Bp, H), bool)
    live[:B, :fx.n_real] = True
    v = np.nan_to_num(o.enc_rows) + fx.bias_h[None, :]
    a = {"sigmoid": lambda z: f(1.0) / (f(1.0) + np.exp(-z)), "tanh": np.tanh, "relu": lambda z: np.maximum(z, f(0.0)),
         "linear": lambda z: z}[act](v.astype(f)).astype(f)
    o.a_out = np.where(live, a, f(0.0)).astype(f)
    o.mask_out = (rng.rand(Bp, H) < keep).astype(np.uint8)
    hv = o.a_out
    if keep < 1.0:
        hv = (o.a_out if wrong == 10 else o.a_out / f(KEEP32)) * o.mask_out.astype(f)
    o.h = R.round_to(hv, wt)
    if wrong == 11:
        o.a_out[B:], o.h[B:] = np.nan, np.nan
    # decoder
    h = R.round_to(np.array(fx.h_given), wt) if h_given else np.nan_to_num(o.h)
    o.h_dec = h
    wo = rows_of(po)
    mm = f(m)
    y = mm * ((h[fx.eb] * wo).sum(1, dtype=f) + fx.bias_out[fx.ecol])
    e = (y - fx.et.astype(f)).astype(f)
    lv = np.ones(E, bool) if wrong == 5 else fx.flag != 0
    rho, g = _f32_loss(loss, e)
    d = np.where(lv, g if wrong == 7 else g * mm, f(0.0)).astype(f)
    o.delta_e = d
    o.d_out = np.full((Bp, N_PAD), np.nan, f)
    o.d_out[fx.eb[lv], fx.ecol[lv]] = R.round_to(d[lv], wt)
    o.dec_part = chunk_sums(d, wo)
    cnt = lv if wrong == 8 else lv & ((fx.et.astype(f) + y) != 0)
    st = np.stack([e * e, np.abs(e), cnt.astype(f), np.zeros(E, f) if (loss == "mse" or wrong == 12) else rho], 1)
    st = (st * lv[:, None]).astype(f)
    o.chunk_stats = np.zeros((ct.n_chunks, 4), f)
    for c in range(ct.n_chunks):
        s = ct.ech == c
        o.chunk_stats[c] = np.add.reduce(st[s][::-1], axis=0, dtype=f) if s.any() else 0.0
    # GRAD_ACT reduction of the decoder's partials
    dv = np.nan_to_num(reduce_rows(o.dec_part))
    if keep < 1.0:
        dv = dv * (o.mask_out.astype(f) / f(KEEP32))
    a0 = np.nan_to_num(o.a_out)
    ga = {"sigmoid": a0 * (f(1.0) - a0), "tanh": f(1.0) - a0 * a0, "relu": (a0 > 0).astype(f), "linear": np.ones_like(a0)}[act]
    hd = np.where(live, dv * ga, f(0.0)).astype(f)
    o.hd = R.round_to(hd, wt)
    o.db_part = hd * f(GSCALE)
    o.stats_part = reduce_rows(o.chunk_stats)
    if not stats4:
        o.stats_part[:, 3] = 0.0
    if wrong == 11:
        o.hd[B:], o.db_part[B:] = np.nan, np.nan
    o.row_sse = o.stats_part[:, 0].copy()
    return o


def check_twin(fx, ct, wt, blocked, o, act="sigmoid", keep=KEEP, m=-1.0, loss="mse", stats4=1):
    """every check of the GPU tests on a twin's outputs; returns (Report, kink share)"""
    _, W1r, _, Woutr = weights_for(wt, fx.H, blocked)
    rep = Report()
    check_encoder(rep, fx, ct, W1r, o.enc_part)
    check_reduce_raw(rep, fx, ct, o.enc_part, o.enc_rows)
    check_bias_act(rep, fx, ct, wt, act, keep, fx.bias_h, o.enc_part, o.a_out, o.mask_out, o.h)
    ent = check_decoder(rep, fx, ct, wt, Woutr, o.h_dec, m, loss, o.delta_e, o.d_out, o.dec_part, o.chunk_stats)
    check_grad_act(rep, fx, ct, wt, act, keep, o.dec_part, o.chunk_stats, o.a_out, o.mask_out, o.hd, o.db_part,
                   o.stats_part, o.row_sse, stats4)
    fo = SimpleNamespace(a_out=o.a_out, mask_out=o.mask_out, h=o.h_dec, delta_e=o.delta_e, d_out=None, hd=o.hd,
                         db_part=o.db_part, stats_part=o.stats_part, row_sse=o.row_sse)
    check_fused(rep, "fused", fx, ct, wt, Woutr, act, keep, m, loss, fo)
    return rep, kink_share(fx, ent)
