"""Every fused ocf_gemm epilogue through the generic tile kernel, and the two split-K reductions that share
their arithmetic, against the NumPy fp64 restatements of tests/epilogue_ref.py: EPI_BIAS_ACT / ocf_splitk_bias_act,
EPI_GRAD_ACT / ocf_splitk_grad_act, EPI_PREDICT, EPI_MASKED_MSE in its three target modes (+ ocf_dense_targets and
ocf_stats_finalize on its outputs) and EPI_OPTIM (generic kernel, and the role-split kernel for the optimizers it
takes).  These are the forms the "bit-identical to another launch form" tests compare against.

Shapes: M = N = 256, K = 192 (two row tiles, two column tiles, three K-steps), m_real = 200, n_real = 130.
Tolerances (epilogue_ref.py): products within 4 K 2^-24 sum|a||b| of the fp64 product of the operands as rounded
to the compute dtype (fp32 accumulation; derived, the same for f32 / f16 / bf16), optimizer state within
rtol 1e-5 / atol 2e-6, counts exact, roundings to 16 bits bitwise.  tests/test_epilogue_ref.py shows on the CPU that
those bars reject a subtly wrong update formula."""
import numpy as np
import pytest
import torch

import epilogue_ref as R
from epilogue_ref import K, M, M_REAL, N, N_REAL
from omnidirectional_collaborative_filtering_amd import _lib
from omnidirectional_collaborative_filtering_amd.dataset import RatingsCSR
from omnidirectional_collaborative_filtering_amd.engine import cur_stream

CD = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CDS = ("f32", "f16", "bf16")
U = R.U16
KEEP = 0.8
KEEP32 = float(np.float32(KEEP))
SENT = -768.0          # exactly representable in f16 and bf16


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.float().cpu().numpy().astype(np.float64) if t.is_floating_point() else t.cpu().numpy()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tune(key, value):
    prev = _lib.I32(0)
    _lib.call("ocf_set_tuning", key, int(value), prev)
    return prev.value


def gemm(cd, A, a_col, B, b_dt, b_col, epi, **kw):
    a = _lib.OcfGemmArgs()
    a.compute_dtype = CD[cd]
    a.A, a.a_dtype, a.a_col, a.lda = A.data_ptr(), CD[cd], a_col, A.stride(0)
    a.B, a.b_dtype, a.b_col, a.ldb = B.data_ptr(), CD[b_dt], b_col, B.stride(0)
    a.M, a.N, a.K, a.splits, a.epi = M, N, K, 1, epi
    a.opt.gscale = 1.0
    a.keep = 1.0
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    _lib.call("ocf_gemm", a, cur_stream())
    torch.cuda.synchronize()


def operands(cd, w_dt, b_col, seed, a_scale=1.0, w_scale=0.05, a_uniform=False):
    """A [M][K] in the compute dtype (padding rows hold values too: m_real must mask them) and a weight W,
    stored [K][N] (b_col) or [N][K], as the fp32 master or the compute-dtype shadow.  Returns the device
    operands and the fp64 [M][K] / [K][N] values the kernel multiplies: both rounded to the compute dtype (an
    fp32 master is rounded while it is staged)."""
    rng = np.random.RandomState(seed)
    A = R.round_to(a_scale * (rng.rand(M, K) if a_uniform else rng.randn(M, K)), cd)
    W = (w_scale * rng.randn(K, N)).astype(np.float32)
    if w_dt != "f32":
        W = R.round_to(W, cd)
    Wd = dev(W if b_col else W.T).to(TD[w_dt])
    return dev(A).to(TD[cd]), Wd, A.astype(np.float64), R.round_to(W, cd).astype(np.float64)


def assert_within(got, ref, tol, what):
    ratio = float((np.abs(got - ref) / tol).max())
    print("%s: worst |err| / bound = %.3g (max |err| %.3g)" % (what, ratio, float(np.abs(got - ref).max())))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def live(x):
    return x[:M_REAL, :N_REAL]


def assert_padding_zero(x, what):
    """x: host [M][>= N]; rows >= m_real and columns n_real .. N are exactly 0"""
    assert not x[M_REAL:, :N].any() and not x[:, N_REAL:N].any(), what


# =========================================================================================================
# EPI_BIAS_ACT
# =========================================================================================================
SAT = np.array([30.0, -30.0, 100.0, -100.0, 1e4, -1e4], np.float32)
SAT_ROW = 7


def forward_case(cd, seed, w_dt="f32"):
    """operands of a hidden-layer forward: row SAT_ROW of A is zero and the first six biases are +-30, +-100,
    +-1e4, so that row's pre-activations are exactly those"""
    Ad, Wd, A, W = operands(cd, w_dt, 1, seed)
    Ad[SAT_ROW] = 0
    A[SAT_ROW] = 0
    rng = np.random.RandomState(seed + 1)
    bias = (0.1 * rng.randn(N)).astype(np.float32)
    bias[:len(SAT)] = SAT
    z = A @ W + bias.astype(np.float64)
    mag = np.abs(A) @ np.abs(W) + np.abs(bias)
    return Ad, Wd, dev(bias), z, mag


def bias_act_call(cd, Ad, Wd, bias, act, ld, keep, seed=0, stream=0, mask_in=None, want_mask=False):
    a_out = torch.full((M, ld), SENT, device="cuda")
    h_out = torch.full((M, ld), SENT, device="cuda").to(TD[cd])
    mask = torch.full((M, ld), 7, device="cuda", dtype=torch.uint8) if want_mask else None
    gemm(cd, Ad, 0, Wd, "f32", 1, _lib.EPI_BIAS_ACT, bias=bias, act=_lib.ACT[act], keep=keep, seed=seed,
         stream=stream, mask_in=mask_in, mask_out=mask, a_out=a_out, h_out=h_out, h_dtype=CD[cd], ld_out=ld,
         m_real=M_REAL, n_real=N_REAL)
    return a_out, h_out, mask


def check_dropout(cd, a_out, h_out, mask, what):
    mk = host(mask)[:, :N]
    assert np.isin(mk, (0, 1)).all(), what
    mean = float(live(mk).mean())
    print("%s: mask mean %.4f" % (what, mean))
    assert abs(mean - KEEP) <= 0.0125, (what, mean)           # 5 sigma of 26,000 Bernoulli(0.8) draws
    ref = (host(a_out)[:, :N] / KEEP32) * mk
    # the correctly rounded fp32 division (one fp32 unit roundoff; the product with the 0 / 1 mask is exact),
    # then one rounding to h_dtype
    lim = (R.round_tol(cd, ref) + 2.0 ** -24 * np.abs(ref)) * (1.0 + 2.0 ** -20)
    assert (np.abs(host(h_out)[:, :N] - ref) <= lim).all(), what


BIAS_ACT_CASES = [(cd, act, N) for cd in CDS for act in R.ACTS] + [("f16", "tanh", N + 64), ("f32", "sigmoid", N + 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("cd,act,ld", BIAS_ACT_CASES)
def test_bias_act(gpu, cd, act, ld):
    Ad, Wd, bias, z, mag = forward_case(cd, 31)
    ref = R.act(act, z)
    a_out, h_out, _ = bias_act_call(cd, Ad, Wd, bias, act, ld, 1.0)
    a = host(a_out)
    assert_within(live(a), live(ref), live(R.product_tol(K, mag, ref)), "a_out %s %s" % (cd, act))
    assert_padding_zero(a, "a_out padding")
    assert (a[:, N:] == SENT).all() and (host(h_out)[:, N:] == SENT).all()
    # keep = 1: h is a rounded once to h_dtype
    assert torch.equal(bits(h_out[:, :N].contiguous()), bits(a_out[:, :N].to(TD[cd]).contiguous()))
    # saturated pre-activations: finite, at the limits
    sat = a[SAT_ROW, :len(SAT)]
    assert np.isfinite(a[:, :N]).all()
    if act in ("sigmoid", "tanh"):
        assert np.abs(sat - R.act(act, SAT.astype(np.float64))).max() <= 1e-6, sat
    # dropout from the device RNG
    a2, h2, mk = bias_act_call(cd, Ad, Wd, bias, act, ld, KEEP, seed=1234, stream=5, want_mask=True)
    assert torch.equal(a2[:, :N], a_out[:, :N])
    check_dropout(cd, a2, h2, mk, "dropout %s %s" % (cd, act))
    assert (host(mk)[:, N:] == 7).all()
    # the recorded mask fed back reproduces h
    _, h3, _ = bias_act_call(cd, Ad, Wd, bias, act, ld, KEEP, seed=99, stream=99, mask_in=mk)
    assert torch.equal(bits(h3), bits(h2))
    # another stream, another mask
    _, _, mk2 = bias_act_call(cd, Ad, Wd, bias, act, ld, KEEP, seed=1234, stream=6, want_mask=True)
    assert not torch.equal(mk2[:, :N], mk[:, :N])
    assert abs(float(live(host(mk2)).mean()) - KEEP) <= 0.0125


def slab_call(cd, Ad, Bd, b_dt, b_col, splits, ld):
    slabs = torch.full((splits, M, ld), SENT, device="cuda")
    gemm(cd, Ad, 0, Bd, b_dt, b_col, _lib.EPI_SLAB, splits=splits, out=slabs, ld_out=ld, split_stride=M * ld)
    return slabs


def splitk_bias_act_call(cd, slabs, bias, act, ld, keep, seed, stream):
    a_out = torch.full((M, ld), SENT, device="cuda")
    h_out = torch.full((M, ld), SENT, device="cuda").to(TD[cd])
    mask = torch.full((M, ld), 7, device="cuda", dtype=torch.uint8)
    _lib.call("ocf_splitk_bias_act", slabs.data_ptr(), slabs.shape[0], M * ld, M, N, ld, bias.data_ptr(), _lib.ACT[act],
              keep, seed, stream, None, mask.data_ptr(), a_out.data_ptr(), h_out.data_ptr(), CD[cd], M_REAL, N_REAL,
              cur_stream())
    torch.cuda.synchronize()
    return a_out, h_out, mask


@pytest.mark.gpu
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("splits,ld", [(1, N), (1, N + 64), (3, N), (7, N)])
def test_splitk_bias_act(gpu, cd, splits, ld):
    # EPI_SLAB takes the fp32 master weights or their compute-dtype shadow (EPI_BIAS_ACT: the master only)
    w_dt = cd if splits == 3 else "f32"
    Ad, Wd, bias, z, mag = forward_case(cd, 32, w_dt)
    slabs = slab_call(cd, Ad, Wd, w_dt, 1, splits, ld)
    for act in R.ACTS:
        a_out, h_out, mk = splitk_bias_act_call(cd, slabs, bias, act, ld, KEEP, 1234, 5)
        ref = R.act(act, z)
        a = host(a_out)
        assert_within(live(a), live(ref), live(R.product_tol(K, mag, ref)), "splitk a_out %s %s x%d" % (cd, act, splits))
        assert_padding_zero(a, "a_out padding")
        assert (a[:, N:] == SENT).all()
        check_dropout(cd, a_out, h_out, mk, "splitk dropout %s %s" % (cd, act))
        if splits == 1:     # the same accumulators, the same (seed, stream, index): the epilogue's outputs exactly
            a2, h2, mk2 = bias_act_call(cd, Ad, Wd, bias, act, ld, KEEP, seed=1234, stream=5, want_mask=True)
            assert torch.equal(bits(a_out), bits(a2)) and torch.equal(bits(h_out), bits(h2)) and torch.equal(mk, mk2)


# =========================================================================================================
# EPI_GRAD_ACT
# =========================================================================================================
def backward_case(cd, act, ld, seed):
    """delta [M][K] x W [N][K] (the fp32 master), the layer's forward activation a_in (exact 0.0 and 1.0 among
    them) and a 0 / 1 dropout mask, both [M][ld]"""
    Ad, Wd, A, W = operands(cd, "f32", 0, seed)
    rng = np.random.RandomState(seed + 1)
    a_in = np.full((M, ld), 0.5, np.float32)
    a_in[:, :N] = R.a_in_for(act, (M, N), rng)
    assert (live(a_in) == 0.0).any() and (live(a_in) == 1.0).any()
    mask = np.ones((M, ld), np.uint8)
    mask[:, :N] = rng.rand(M, N) < KEEP
    return Ad, Wd, A @ W, np.abs(A) @ np.abs(W), a_in, mask


def grad_refs(act, d_raw, mag, a_in, mask, dd):
    """reference delta (zero outside the live range), its bound before / after the rounding to d_dtype"""
    a, mk = a_in[:, :N], mask[:, :N]
    ref = np.zeros((M, N))
    ref[:M_REAL, :N_REAL] = live(R.grad_act(act, d_raw, a, mk, KEEP32))
    fac = np.abs(R.grad_act(act, np.ones_like(d_raw), a, mk, KEEP32))
    tol32 = R.product_tol(K, mag) * fac + 4.0 * 2.0 ** -24 * np.abs(ref) + 1e-30       # + the three fp32 products
    return ref, tol32, tol32 + R.round_tol(dd, ref)


def check_db(db, ref, tol32, rows_per_part, gscale, what):
    parts = M // rows_per_part
    want = ref.reshape(parts, rows_per_part, N).sum(1) * gscale
    tol = (tol32.reshape(parts, rows_per_part, N).sum(1) +
           rows_per_part * 2.0 ** -24 * np.abs(ref).reshape(parts, rows_per_part, N).sum(1)) * gscale + 1e-30
    assert_within(host(db)[:, :N], want, tol, what)


@pytest.mark.gpu
@pytest.mark.parametrize("cd,dd,ld", [(cd, dd, N) for cd in CDS for dd in CDS] + [("bf16", "bf16", N + 64)])
def test_grad_act(gpu, cd, dd, ld):
    gscale = float(np.float32(R.GSCALE))
    for act in R.ACTS:
        Ad, Wd, d_raw, mag, a_in, mask = backward_case(cd, act, ld, 41)
        ref, tol32, tol = grad_refs(act, d_raw, mag, a_in, mask, dd)
        a_dev, m_dev = dev(a_in), dev(mask)
        d_out = torch.full((M, ld), SENT, device="cuda").to(TD[dd])
        db = torch.full((M // 128, ld), SENT, device="cuda")
        gemm(cd, Ad, 0, Wd, "f32", 0, _lib.EPI_GRAD_ACT, a_in=a_dev, mask_in=m_dev, keep=KEEP, act=_lib.ACT[act],
             h_out=d_out, h_dtype=CD[dd], ld_out=ld, db_part=db, m_real=M_REAL, n_real=N_REAL,
             opt=_lib.OcfOptParams(0, 0, 0, 0, 0, 0, gscale))
        d = host(d_out)
        what = "grad_act %s->%s %s" % (cd, dd, act)
        assert_within(live(d), live(ref), live(tol), what)
        assert_padding_zero(d, what)
        assert (d[:, N:] == SENT).all()
        check_db(db, ref, tol32, 128, gscale, what + " db_part")
        # relu'(0) = 0, sigmoid'(1) = tanh'(1) = 0, exactly
        if act != "linear":
            dead = live((a_in[:, :N] == (0.0 if act == "relu" else 1.0)))
            assert dead.any() and not live(d)[dead].any(), what
        # the split-K reduction on the same product
        for splits in (1, 3):
            slabs = slab_call(cd, Ad, Wd, "f32", 0, splits, ld)
            d2 = torch.full((M, ld), SENT, device="cuda").to(TD[dd])
            db2 = torch.full((M // 4, ld), SENT, device="cuda")
            _lib.call("ocf_splitk_grad_act", slabs.data_ptr(), splits, M * ld, M, N, ld, a_dev.data_ptr(),
                      m_dev.data_ptr(), KEEP, _lib.ACT[act], d2.data_ptr(), CD[dd], db2.data_ptr(), gscale, M_REAL,
                      N_REAL, cur_stream())
            torch.cuda.synchronize()
            dh = host(d2)
            assert_within(live(dh), live(ref), live(tol), what + " splitk x%d" % splits)
            assert_padding_zero(dh, what)
            check_db(db2, ref, tol32, 4, gscale, what + " splitk db x%d" % splits)
            if splits == 1:
                assert torch.equal(bits(d2), bits(d_out)), what


# =========================================================================================================
# EPI_PREDICT
# =========================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("cd,b_col,masked,ld", [(cd, bc, mk, N) for cd in CDS for bc in (1, 0) for mk in (False, True)]
                         + [("f16", 1, True, N + 64)])
def test_predict(gpu, cd, b_col, masked, ld):
    Ad, Wd, A, W = operands(cd, "f32", b_col, 51)
    rng = np.random.RandomState(52)
    bias = (0.1 * rng.randn(N)).astype(np.float32)
    pm = rng.choice(np.array([0.0, -1.0, 1.0, 0.5], np.float32), size=(M, ld + 8))
    y = A @ W + bias.astype(np.float64)
    tol = R.product_tol(K, np.abs(A) @ np.abs(W) + np.abs(bias), y)
    if masked:
        y, tol = pm[:, :N] * y, np.abs(pm[:, :N]) * tol + 1e-30
    out = torch.full((M, ld), SENT, device="cuda")
    gemm(cd, Ad, 0, Wd, "f32", b_col, _lib.EPI_PREDICT, bias=dev(bias), out=out, ld_out=ld, m_real=M_REAL,
         n_real=N_REAL, **(dict(pmask=dev(pm), ld_pmask=ld + 8) if masked else {}))
    o = host(out)
    assert_within(live(o), live(y), live(tol), "predict %s b_col=%d masked=%d" % (cd, b_col, masked))
    o[:M_REAL, :N_REAL] = SENT
    assert (o == SENT).all(), "EPI_PREDICT wrote outside [m_real, n_real)"


# =========================================================================================================
# EPI_MASKED_MSE: one target set in the three target modes
# =========================================================================================================
N_TILES = N // 128


def target_set(seed, aux):
    """A rating CSR (lists in random order, empty rows, one duplicated (row, column) pair) and a batch of its
    rows (some batch rows without a row, some with an empty one); live-target flags that kill ~20 % of the
    entries and one of the two duplicates.  Returns the row-segment descriptor and the dense [m_real][n_real]
    targets / masks of the live entries."""
    rng = np.random.RandomState(seed)
    rows_ds = 230
    lens = rng.randint(0, 24, size=rows_ds)
    lens[rng.rand(rows_ds) < 0.1] = 0
    cols, vals = [], []
    for r in range(rows_ds):
        c = rng.choice(N_REAL, size=lens[r], replace=False)
        if lens[r] >= 2 and r % 3 == 0:
            c[0], c[1] = N_REAL - 1, 128          # the last real column, the first column of the second tile
            c = np.concatenate([c[:2], np.setdiff1d(c[2:], c[:2])])
            lens[r] = len(c)
        cols.append(c)
        vals.append(rng.randint(1, 11, size=lens[r]) / 2.0)
    t_rows = rng.choice(rows_ds, size=M_REAL, replace=False).astype(np.int32)
    t_rows[rng.rand(M_REAL) < 0.05] = -1
    dup_b = int(np.nonzero((t_rows >= 0) & (lens[np.maximum(t_rows, 0)] >= 3))[0][0])
    dup_r = int(t_rows[dup_b])
    cols[dup_r] = np.concatenate([cols[dup_r], cols[dup_r][2:3]])          # the pair: list positions 2 and last
    vals[dup_r] = np.concatenate([vals[dup_r], [5.0 if vals[dup_r][2] != 5.0 else 0.5]])
    lens[dup_r] += 1
    rp = np.zeros(rows_ds + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = np.concatenate(cols).astype(np.int32)
    val = np.concatenate(vals).astype(np.float32)
    val[rng.choice(len(val), 8, replace=False)] = 0.0                       # rated exactly 0
    csr = RatingsCSR(rp, col, val)
    col_s, val_s, lidx_s, tptr = csr.tile_index(N)
    blens = np.where(t_rows >= 0, lens[np.maximum(t_rows, 0)], 0)
    lboff = np.zeros(M_REAL + 1, np.int64)
    np.cumsum(blens, out=lboff[1:])
    flag = (rng.rand(int(lboff[-1])) < 0.8).astype(np.uint8)
    flag[lboff[dup_b] + 2], flag[lboff[dup_b] + lens[dup_r] - 1] = 0, 1   # last write wins
    T = np.zeros((M_REAL, N_REAL), np.float32)
    Mk = np.zeros((M_REAL, N_REAL), np.float32)
    seen = np.zeros((M_REAL, N_REAL), np.int32)
    for b, r in enumerate(t_rows):
        for j in range(blens[b]):
            if flag[lboff[b] + j]:
                c = col[rp[r] + j]
                T[b, c], Mk[b, c] = val[rp[r] + j], aux
                seen[b, c] += 1
    assert seen.max() == 1, "at most one live target per (row, column)"
    assert (Mk[:, N_REAL - 1] != 0).any() and (Mk[:, 128] != 0).any() and ((Mk != 0) & (T == 0)).any()
    assert (Mk != 0).any(1).sum() < M_REAL - 5, "rows with no targets"
    seg = dict(t_rows=dev(t_rows), t_rp=dev(rp), t_tptr=dev(tptr), t_col=dev(col_s), t_val=dev(val_s),
               t_lidx=dev(lidx_s), t_flag=dev(flag), t_lboff=dev(lboff), t_ntiles=tptr.shape[1] - 1, t_aux=aux)
    return seg, T, Mk


def dense_targets_call(Td, Md, ld, B, n_cols, n_tiles, rows, cap):
    cnt = torch.zeros(n_tiles, dtype=torch.int32, device="cuda")
    ptr = torch.full((n_tiles + 1,), -5, dtype=torch.int32, device="cuda")
    cur = torch.full((n_tiles,), -5, dtype=torch.int32, device="cuda")
    rc = torch.full((cap,), -5, dtype=torch.int32, device="cuda")
    bt = torch.full((cap,), SENT, device="cuda")
    bm = torch.full((cap,), SENT, device="cuda")
    _lib.call("ocf_dense_targets", Td.data_ptr(), Md.data_ptr(), ld, B, n_cols, n_tiles, cnt.data_ptr(), ptr.data_ptr(),
              cur.data_ptr(), rc.data_ptr(), bt.data_ptr(), bm.data_ptr(), rows.data_ptr() if rows is not None else None,
              cur_stream())
    torch.cuda.synchronize()
    return cnt, ptr, cur, rc, bt, bm


def assert_buckets(got, want):
    cnt, ptr, cur, rc, bt, bm = got
    wptr, wrc, wt, wm = want
    n = int(wptr[-1])
    assert ptr.cpu().numpy().tolist() == wptr.tolist()
    assert cur.cpu().numpy().tolist() == wptr[:-1].tolist() and not cnt.any()       # counts left zeroed
    assert np.array_equal(rc.cpu().numpy()[:n], wrc)
    assert np.array_equal(bt.cpu().numpy()[:n], wt) and np.array_equal(bm.cpu().numpy()[:n], wm)
    assert (rc[n:] == -5).all() and (bt[n:] == SENT).all()


def mse_call(cd, hd, Wd, w_dt, b_col, bias, ld, gscale, tg, train=True):
    gm = M // 128
    d_out = torch.full((M, ld), SENT, device="cuda").to(TD[cd]) if train else None
    db = torch.full((gm, ld), SENT, device="cuda") if train else None
    sp = torch.full((N_TILES * gm, 4), SENT, device="cuda")
    rs = torch.full((N_TILES, M), SENT, device="cuda")
    gemm(cd, hd, 0, Wd, w_dt, b_col, _lib.EPI_MASKED_MSE, bias=bias, h_out=d_out, h_dtype=CD[cd], ld_out=ld,
         db_part=db, ld_db=ld, stats_part=sp, row_sse_part=rs, m_real=M_REAL, n_real=N_REAL,
         opt=_lib.OcfOptParams(0, 0, 0, 0, 0, 0, gscale), **tg)
    out = torch.full((4 + M,), SENT, device="cuda")
    _lib.call("ocf_stats_finalize", sp.data_ptr(), N_TILES * gm, rs.data_ptr(), N_TILES, M, out.data_ptr(), cur_stream())
    torch.cuda.synchronize()
    return d_out, db, sp, rs, out


def check_mse(cd, res, y, ytol, T, Mk, gscale, what, train=True):
    d_out, db, _, _, out = res
    ref = R.masked_mse(y, T, Mk)
    am = np.abs(Mk.astype(np.float64))
    o = host(out)
    # count_nonzero(t + yhat) is exact: the reference's own entries are nowhere near the decision
    assert o[2] == ref["count"], (what, o[2], ref["count"])
    assert o[3] == 0.0
    sse_tol = 1e-5 * ref["row_sse"] + (2.0 * np.abs(ref["err"]) * am * ytol).sum(1) + 1e-30
    assert_within(o[4:4 + M_REAL], ref["row_sse"], sse_tol, what + " row SSE")
    assert not o[4 + M_REAL:].any(), what
    assert_within(o[0:1], np.array([ref["sse"]]), np.array([1e-5 * ref["sse"] + (2.0 * np.abs(ref["err"]) * am * ytol).sum()]),
                  what + " SSE")
    assert_within(o[1:2], np.array([ref["sae"]]), np.array([1e-5 * ref["sae"] + (am * ytol)[ref["on"]].sum()]), what + " SAE")
    if not train:
        return
    dref = np.zeros((M, N))
    dref[:M_REAL, :N_REAL] = ref["d"]
    tol32 = np.zeros((M, N))
    tol32[:M_REAL, :N_REAL] = am * am * ytol + 4.0 * 2.0 ** -24 * np.abs(ref["d"])
    dtol = tol32 + U[cd] * (cd != "f32") * np.abs(dref) + 1e-30       # (|d| > 1e-4 at every target, asserted by the caller: no f16 underflow)
    d = host(d_out)
    assert_within(d[:, :N], dref, dtol, what + " d_out")
    assert not d[:, :N][dref == 0].any(), what + ": delta outside the targets"
    assert (d[:, N:] == SENT).all()
    check_db(db, dref, tol32, 128, gscale, what + " db_part")


MSE_CASES = [("f32", "f32", 1, -1.0, N), ("f32", "f32", 0, 1.0, N), ("f16", "f32", 1, -1.0, N), ("f16", "f16", 0, 1.0, N),
             ("f16", "f16", 1, -1.0, N + 64), ("bf16", "f32", 0, 1.0, N), ("bf16", "bf16", 1, -1.0, N),
             ("bf16", "bf16", 0, 1.0, N)]


@pytest.mark.gpu
@pytest.mark.parametrize("cd,w_dt,b_col,aux,ld", MSE_CASES)
def test_masked_mse_three_target_modes(gpu, cd, w_dt, b_col, aux, ld):
    gscale = float(np.float32(R.GSCALE))
    rng = np.random.RandomState(61)
    # hidden activations in [0, 1); weight and bias scaled so that max |y| = 0.4
    hd, _, h, W0 = operands(cd, "f32", 1, 62, a_uniform=True, w_scale=1.0)
    b0 = 0.5 * rng.randn(N)
    s = 0.4 / np.abs(h @ W0 + b0).max()
    W = (s * W0).astype(np.float32)
    if w_dt != "f32":
        W = R.round_to(W, cd)
    Wd = dev(W if b_col else W.T).to(TD[w_dt])
    W = R.round_to(W, cd).astype(np.float64)
    bias = (s * b0).astype(np.float32)
    y = live(h @ W + bias.astype(np.float64))
    ytol = live(R.product_tol(K, np.abs(h) @ np.abs(W) + np.abs(bias), h @ W + bias))
    seg, T, Mk = target_set(63, aux)
    # the reference's own decisions are well-posed (asserted, not filtered)
    yhat = Mk * y
    assert np.abs(y).max() < 0.45
    assert (np.abs(T + yhat)[(T != 0) & (Mk != 0)] > 1e-3).all()
    assert (np.abs(yhat)[(T == 0) & (Mk != 0)] > 1e-4).all()
    # dense mode: the batch rows live at permuted rows of a larger array
    perm = rng.permutation(M_REAL + 17)[:M_REAL].astype(np.int64)
    ld_dn = N_REAL + 6
    Tds = np.full((M_REAL + 17, ld_dn), 3.0, np.float32)
    Mds = np.full((M_REAL + 17, ld_dn), 1.0, np.float32)
    Tds[perm, :N_REAL], Mds[perm, :N_REAL] = T, Mk
    Tdd, Mdd, rows_d = dev(Tds), dev(Mds), dev(perm)
    dense = dict(dn_t=Tdd, dn_m=Mdd, ld_dn=ld_dn, dn_rows=rows_d)
    # bucket mode: ocf_dense_targets on the same arrays, checked against the documented layout
    n_ent = int(((T != 0) | (Mk != 0)).sum())
    bk = dense_targets_call(Tdd, Mdd, ld_dn, M_REAL, N_REAL, N_TILES, rows_d, n_ent + 8)
    assert_buckets(bk, R.bucket_layout(T, Mk, N_TILES))
    bucket = dict(bk_ptr=bk[1], bk_rc=bk[3], bk_t=bk[4], bk_m=bk[5])
    bd = dev(bias)
    res = {}
    for mode, tg in (("segment", seg), ("bucket", bucket), ("dense", dense)):
        what = "masked_mse %s/%s b_col=%d aux=%g %s" % (cd, w_dt, b_col, aux, mode)
        res[mode] = mse_call(cd, hd, Wd, w_dt, b_col, bd, ld, gscale, tg)
        check_mse(cd, res[mode], y, ytol, T, Mk, gscale, what)
        ev = mse_call(cd, hd, Wd, w_dt, b_col, bd, ld, gscale, tg, train=False)      # d_out = NULL: eval
        check_mse(cd, ev, y, ytol, T, Mk, gscale, what + " eval", train=False)
        assert torch.equal(ev[2], res[mode][2])
        # (the bucket mode adds a row's squared errors with LDS atomics: its row SSE is not ordered)
        assert mode == "bucket" or torch.equal(ev[3], res[mode][3])
    for mode in ("bucket", "dense"):
        assert torch.equal(bits(res[mode][0]), bits(res["segment"][0])), mode
        assert torch.equal(bits(res[mode][1][:, :N].contiguous()), bits(res["segment"][1][:, :N].contiguous())), mode
    # entries only the bucket / dense modes can express: m = 0 with t != 0 (counted: t + 0 != 0, zero delta)
    # and, in a bucket, m = 0 with t = 0 (never counted)
    free = np.argwhere((T == 0) & (Mk == 0))
    pick = free[rng.choice(len(free), 40, replace=False)]
    T2, Mk2 = T.copy(), Mk.copy()
    T2[pick[:30, 0], pick[:30, 1]] = rng.randint(1, 11, 30) / 2.0
    ptr, rc, bt, bm = R.bucket_layout(T2, Mk2, N_TILES)
    zb, zn = pick[30:, 0], pick[30:, 1]
    parts = []
    for t in range(N_TILES):                       # the all-zero entries go to the end of their tile's bucket
        z = (zn >> 7) == t
        parts.append((np.concatenate([rc[ptr[t]:ptr[t + 1]], ((zb[z] << 7) | (zn[z] & 127)).astype(np.int32)]),
                      np.concatenate([bt[ptr[t]:ptr[t + 1]], np.zeros(z.sum(), np.float32)]),
                      np.concatenate([bm[ptr[t]:ptr[t + 1]], np.zeros(z.sum(), np.float32)])))
    ptr2 = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int32)
    bucket2 = dict(bk_ptr=dev(ptr2), bk_rc=dev(np.concatenate([p[0] for p in parts])),
                   bk_t=dev(np.concatenate([p[1] for p in parts])), bk_m=dev(np.concatenate([p[2] for p in parts])))
    what = "masked_mse %s/%s bucket, m = 0 entries" % (cd, w_dt)
    r2 = mse_call(cd, hd, Wd, w_dt, b_col, bd, ld, gscale, bucket2)
    check_mse(cd, r2, y, ytol, T2, Mk2, gscale, what)
    assert R.masked_mse(y, T2, Mk2)["count"] == R.masked_mse(y, T, Mk)["count"] + 30
    Tds[perm, :N_REAL] = T2
    r3 = mse_call(cd, hd, Wd, w_dt, b_col, bd, ld, gscale, dict(dense, dn_t=dev(Tds)))
    check_mse(cd, r3, y, ytol, T2, Mk2, gscale, what.replace("bucket", "dense"))


# =========================================================================================================
# EPI_OPTIM
# =========================================================================================================
def optim_call(cd, kind, l2, ld, blocked=0):
    A, B = R.optim_operands(cd)
    p0, s10, s20 = R.opt_inputs((M, N), 22)
    full = lambda x: np.concatenate([x, np.full((M, ld - N), SENT, np.float32)], 1)
    P, S1, S2 = dev(full(p0)), dev(full(s10)), dev(full(s20))
    Sh = torch.full((M, ld), SENT, device="cuda").to(TD[cd]) if cd != "f32" else None
    h = R.hyper(kind, l2)
    opt = _lib.OcfOptParams(R.OPT_KIND[kind], h["lr"], h["eps"], h["rho"], h["beta2"], h["l2"], h["gscale"])
    gemm(cd, dev(A).to(TD[cd]), 1, dev(B).to(TD[cd]), cd, 1, _lib.EPI_OPTIM, p=P, ld_out=ld, opt=opt,
         s1=S1 if kind != "sgd" else None, s2=S2 if kind == "adam" else None, p_shadow=Sh, shadow_blocked=blocked)
    g = A.astype(np.float64).T @ B.astype(np.float64)
    ref = R.opt_update(kind, p0, g, s10 if kind != "sgd" else None, s20 if kind == "adam" else None, **h)
    return (P, S1, S2, Sh), ref, (p0, s10, s20)


def check_optim(cd, kind, res, ref, init, what, blocked=0):
    P, S1, S2, Sh = res
    got = [host(t)[:, :N] for t in (P, S1, S2)]
    worst = R.opt_worst(got, ref)
    print("%s: worst |err| / (atol + rtol |ref|) = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)
    # slots the optimizer does not have, and everything past column N, are untouched
    for x, x0, r in zip(got[1:], init[1:], ref[1:]):
        assert r is not None or np.array_equal(x, x0), what
    for t in (P, S1, S2):
        assert (t[:, N:] == SENT).all(), what
    assert not np.array_equal(got[0], init[0])
    if Sh is not None:          # the shadow is the updated fp32 parameter rounded once
        want = P[:, :N].to(TD[cd]).contiguous()
        if blocked:
            want = want.view(M // 64, 64, N // 64, 64).permute(0, 2, 1, 3).contiguous().view(M, N)
            assert torch.equal(bits(Sh.view(-1)[:M * N].view(M, N)), bits(want)), what
        else:
            assert torch.equal(bits(Sh[:, :N].contiguous()), bits(want)), what
            assert (Sh[:, N:] == SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("kind", R.OPTS)
def test_optim_generic_kernel(gpu, cd, kind, l2):
    prev = _tune(b"optim_ws", 0)
    try:
        res, ref, init = optim_call(cd, kind, l2, N)
    finally:
        _tune(b"optim_ws", prev)
    check_optim(cd, kind, res, ref, init, "optim generic %s %s l2=%d" % (cd, kind, l2))


@pytest.mark.gpu
@pytest.mark.parametrize("cd,kind,ld,blocked", [("f32", "adam", N + 64, 0), ("f16", "sgd", N + 64, 0),
                                                ("bf16", "rmsprop", N + 64, 0), ("f16", "adagrad", N, 1)])
def test_optim_generic_kernel_ld_and_blocked_shadow(gpu, cd, kind, ld, blocked):
    prev = _tune(b"optim_ws", 0)
    try:
        res, ref, init = optim_call(cd, kind, True, ld, blocked)
    finally:
        _tune(b"optim_ws", prev)
    check_optim(cd, kind, res, ref, init, "optim generic %s %s ld=%d blocked=%d" % (cd, kind, ld, blocked), blocked)


@pytest.mark.gpu
@pytest.mark.parametrize("cd", ["f16", "bf16"])
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("kind", ["adagrad", "rmsprop", "adam"])
def test_optim_role_split_kernel(gpu, cd, kind, l2):
    """the other side of test_optim_ws_gpu.py::test_ws_dense_bit_identical, against the same reference"""
    prev = _tune(b"optim_ws", 1)
    try:
        res, ref, init = optim_call(cd, kind, l2, N)
    finally:
        _tune(b"optim_ws", prev)
    check_optim(cd, kind, res, ref, init, "optim role-split %s %s l2=%d" % (cd, kind, l2))
