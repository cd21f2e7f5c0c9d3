"""NumPy fp64 restatement of ocf_predict_entries (include/ocf.h OcfPredictArgs, csrc/ocf_predict.hip) on the
hand-built batch of tests/gather_ref.py: the prediction y at every batch-local entry, its clipped value, the row
statistics and their total, with the bound of each; a float32 restatement that sums in the kernel's order (`twin`)
and a list of deliberately wrong variants of it.  tests/test_predict_ref.py shows on the CPU that the bounds accept
the restatement and reject every variant; tests/test_predict_direct_gpu.py applies the same checks to the kernel.

Bounds (gather_ref's, nothing tuned):
  * y = aux (h . W[n] + bias[n]): gather_ref.dec_entry's `by` (a sum of H fp32 products and one bias);
  * the clipped y: clipping is 1-Lipschitz, so the same `by`;
  * the statistics, taken on the stored (clipped) y: gather_ref.dec_stats on the residual e = y - t with
    be = by + u |e|, summed over a row's flagged entries and its chunk count; the count of t + y != 0 is exact but
    for the entries whose |t + y| lies within y's bound (dec_stats' `ambiguous`);
  * total: the DEVICE rows added in fp64, bound of a sum of Bp terms.

TEST INFRASTRUCTURE ONLY: nothing here is on the product path.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import epilogue_ref as R
import gather_ref as G

CLIP = (0.5, 5.0)
CHUNK, CHUNK_ALT = 256, 64
GUARD = 64                               # elements past E the kernel must leave alone
SLAB = 512
# the kernel's instances: gather_ref.GRID (every (weight type, G, PPL) of the register form) and the slab form
# (H > 512) at a short last slab (640) and at whole slabs (1024), fp32 and 16-bit, row-major and blocked
GRID = list(G.GRID) + [("f32", 640, 0), ("f32", 1024, 0), ("f16", 640, 0), ("f16", 1024, 0), ("f16", 640, 1),
                       ("f16", 1024, 1)]
GRID_IDS = ["%s-H%d-%s" % (wt, H, "blocked" if bl else "rowmajor") for wt, H, bl in GRID]
ALL_H = (128, 256, 384, 512, 640, 768, 1024, 2048)


def shape(wt, H):
    """(G, PPL, slab form) of ocf_predict.hip launch_by_shape"""
    if H > SLAB:
        return 32, SLAB // 32 // G.ESIZE[wt], True
    g, ppl = G.gather_shape(wt, H)
    return g, ppl, False


def hidden(fx, wt):
    """the fixture's hidden rows rounded to the operand type: (float32 array as stored, float64 values)"""
    h = R.round_to(np.array(fx.h_given), wt)
    return h, h.astype(np.float64)


def reference(fx, ct, hr, Wr, aux, clip, use_flag):
    """fp64: y per entry (clipped when clip), bound by; row statistics [Bp][4] and their bound"""
    ent = G.dec_entry(fx, hr, Wr, fx.bias_out, aux, "mse")
    y = np.clip(ent.y, *clip) if clip else ent.y
    live = (fx.flag != 0) if use_flag else np.ones(fx.E, bool)
    e = y - fx.et
    se = SimpleNamespace(live=live, e=e, be=ent.by + G.U * np.abs(e), tpy=fx.et + y, loss="mse",
                         ambiguous=live & (ent.by > 0) & (np.abs(fx.et + y) <= ent.by))
    c = np.zeros(fx.Bp)
    c[:fx.B] = np.diff(ct.row_cptr)
    rows, rb = G.dec_stats(se, fx.eb, fx.Bp, c[:, None])
    rows[:, 3], rb[:, 3] = 0.0, 0.0
    empty = np.ones(fx.Bp, bool)
    empty[:fx.B] = fx.lens == 0
    return SimpleNamespace(y=y, by=ent.by, y_raw=ent.y, rows=rows, rows_bound=rb, empty=empty, ent=se)


def check(rep, fx, ref, y, row_stats, total, stage="predict"):
    """y [E + GUARD] (prefilled with NaN), row_stats [Bp][4], total [4] (None: no statistics asked for)"""
    y = np.asarray(y, np.float64)
    rep.add(stage + ": y", y[:fx.E], ref.y, ref.by)
    rep.exact(stage + ": guard past E untouched", np.isnan(y[fx.E:]), True)
    if row_stats is None:
        return
    rs = np.asarray(row_stats, np.float64)
    rep.add(stage + ": row_stats", rs, ref.rows, ref.rows_bound)
    rep.exact(stage + ": rows without entries and padding rows are zero", rs[ref.empty], 0.0)
    rep.add(stage + ": total", total, rs.sum(0), G.sum_bound(0, fx.Bp, np.abs(rs).sum(0)))


# ---- float32 restatement in the kernel's order, and its wrong variants ----------------------------------------------
WRONG = {
    1: "flag ignored in the statistics",
    2: "clip applied after the residual",
    3: "aux dropped",
    4: "bias of the wrong column",
    5: "blocked weights addressed as row-major",
    6: "last entry of a chunk dropped",
    7: "slabs beyond 512 dropped",
}


def wrong_applies(k, wt, H, blocked, aux, clip, use_flag):
    return {1: use_flag, 2: clip is not None, 3: aux != 1.0, 5: bool(blocked), 7: H > SLAB}.get(k, True)


def twin(fx, ct, wt, blocked, aux, clip, use_flag, wrong=None):
    """ocf_predict_entries in float32, summed as the kernel sums: a lane's pieces slab by slab, piece by piece,
    element by element; the G lanes by the xor butterfly; a group's entries in order, the groups in order, a row's
    chunks in order, the rows strided over 256 threads and folded by halves.  wrong: a key of WRONG."""
    f = np.float32
    H, E, Bp = fx.H, fx.E, fx.Bp
    Gl, PPL, slab = shape(wt, H)
    Ee = G.ESIZE[wt]
    NG = 256 // Gl
    _, _, po, _ = G.weights_for(wt, H, blocked)
    w = G.unpack_rows(po, wt, blocked and wrong != 5, fx.ecol)
    h, _ = hidden(fx, wt)
    prod = (h[fx.eb] * w).astype(f)
    span = Gl * PPL * Ee
    ns = -(-H // span)
    if wrong == 7:
        prod[:, span:] = 0
    prod = np.concatenate([prod, np.zeros((E, ns * span - H), f)], 1)
    lanes = prod.reshape(E, ns, PPL, Gl, Ee).transpose(0, 3, 1, 2, 4).reshape(E, Gl, ns * PPL * Ee)
    dot = np.zeros((E, Gl), f)
    for q in range(lanes.shape[2]):
        dot = dot + lanes[:, :, q]
    off = Gl // 2
    while off:
        dot = dot + dot[:, np.arange(Gl) ^ off]
        off //= 2
    dot = dot[:, 0]
    bcol = (fx.ecol + 1) % G.N_PAD if wrong == 4 else fx.ecol
    y = dot + fx.bias_out[bcol]
    if wrong != 3:
        y = f(aux) * y
    y = y.astype(f)
    ys = np.clip(y, f(clip[0]), f(clip[1])) if clip else y                # the stored value
    yr = y if wrong == 2 else ys                                          # the value the residual is taken on
    t = fx.et.astype(f)
    e = (yr - t).astype(f)
    lv = (fx.flag != 0) if (use_flag and wrong != 1) else np.ones(E, bool)
    st = (np.stack([e * e, np.abs(e), ((t + yr) != 0).astype(f), np.zeros(E, f)], 1) * lv[:, None]).astype(f)
    out_y = np.full(E + GUARD, np.nan, f)
    chunk_stats = np.zeros((ct.n_chunks, 4), f)
    for c in range(ct.n_chunks):
        lo = int(fx.lboff[ct.ch_row[c]])
        j0, j1 = lo + int(ct.ch_j0[c]), lo + int(ct.ch_j1[c])
        if wrong == 6:
            j1 -= 1
        out_y[j0:j1] = ys[j0:j1]
        v = np.zeros(4, f)
        for g in range(NG):
            s = np.zeros(4, f)
            for row in st[j0 + g:j1:NG]:
                s = s + row
            v = v + s
        chunk_stats[c] = v
    rows = np.zeros((Bp, 4), f)
    for b in range(fx.B):
        for c in range(int(ct.row_cptr[b]), int(ct.row_cptr[b + 1])):
            rows[b] = rows[b] + chunk_stats[c]
    red = np.zeros((256, 4), f)
    for b in range(Bp):
        red[b % 256] = red[b % 256] + rows[b]
    n = 128
    while n:
        red[:n] = red[:n] + red[n:2 * n]
        n //= 2
    return SimpleNamespace(y=out_y, row_stats=rows, total=red[0].copy())
