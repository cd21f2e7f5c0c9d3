#!/usr/bin/env python
"""Times top-k recommendation two ways from the same hidden activations, in one process:

  new       Engine.topk (ocf_topk): the decoder GEMM with the top-k epilogue + the merge launch; seen items
            excluded through the row-segment form; no [B, N] array
  baseline  what the same answer took before ocf_topk: Engine.predict_dense into a [B, N] fp32 array, masked_fill
            of the same exclusions (the boolean mask is built once, outside the timing), torch.topk

at a BASELINE.json configuration (synthetic_fixed_split, B = 256, H = 500, f16, seen items excluded), for k = 10
and k = 100.  Device events; both warmed up; the two alternate for --repeats rounds of --inner calls each.  Prints
one JSON line and writes it to profiles/recommend_<config>.json.  The bar: the new path's mean below the baseline's
by more than the two spreads (standard deviations over the rounds) combined; the line says whether it is met.
The achieved bytes/s (algorithmic bytes of each path over its time, against the 8 TB/s HBM peak) is information,
not a bar.

Only the batch's rows matter for the timing (N, H, B and the entries per row), so the synthetic matrix is built
with --rows rows at the configuration's density instead of all of them.

    python tools/recommend_bench.py --config ml20m
    python tools/recommend_bench.py --config netflix
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ml20m", choices=["ml100k", "ml1m", "ml1m_u", "ml20m", "netflix"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=500)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--rows", type=int, default=4096, help="rows of the synthetic matrix (0: the configuration's)")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats >= 5")

    import torch
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.dataset import SYNTH_SHAPES, synthetic_fixed_split
    from omnidirectional_collaborative_filtering_amd.model import omni_model

    shape = SYNTH_SHAPES[args.config]
    rows = min(args.rows, shape["rows"]) if args.rows else shape["rows"]
    data = synthetic_fixed_split(args.config, seed=0, scale_rows=rows if rows != shape["rows"] else None)
    N, B, H = data.num_cols, args.batch, args.hidden
    np.random.seed(0)
    rd = data_reader(N, data.train.n_rows, dataset=data, eval_mode="fixed_split")
    om = omni_model(1, H, N, B, dense_activation="sigmoid", use_causal_info=False, compute_dtype=args.dtype, seed=3)
    m, e = om.model, om.engine
    m.compile(O.Adagrad(lr=0.005, epsilon=1e-8), "mean_squared_error")
    gen = rd.data_gen(B, [1.0, 1.0], "valid", False, None, -1)
    m._check_gen(gen)
    bi = gen.next_batch_index()
    m._load(None, gen, bi)
    e.forward(training=False)
    e._finish_deferred_encoder()            # h[0] written; both paths start from it
    t = gen.src1.tiles(N)
    seg = dict(ex_rows=gen.rows_dev.data_ptr() + 4 * bi * B, ex_rp=gen.src1.rp, ex_tptr=t["t_tptr"],
               ex_col=t["t_col"], ex_ntiles=t["t_ntiles"])
    rows_b = gen.rows_host[bi]
    csr = data.valid_in
    seen = torch.zeros(B, N, dtype=torch.bool)
    for b, r in enumerate(rows_b):
        seen[b, torch.as_tensor(csr.col[csr.row_ptr[r]:csr.row_ptr[r + 1]].astype(np.int64))] = True
    n_seen = int(seen.sum())
    seen = seen.to(e.dev)
    scores = torch.empty(B, N, device=e.dev, dtype=torch.float32)
    torch.cuda.synchronize()

    def new(k):
        return e.topk(k, exclude=seg, groups=args.groups or None)

    def base(k, out=scores):
        e.predict_dense(None, out)
        out.masked_fill_(seen, float("-inf"))
        return torch.topk(out, k, dim=1)

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn(k)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    def peak_extra(fn, k):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(k)
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    es = 4 if args.dtype == "float32" else 2
    Wt, _ = e._wop(1)
    line = dict(tool="recommend_bench", config=args.config, N=N, B=B, H=H, dtype=args.dtype, matrix_rows=rows,
                seen_entries=n_seen, repeats=args.repeats, inner=args.inner, groups=args.groups,
                device=torch.cuda.get_device_name(0), operand="shadow" if Wt is not e.W[1] else "master")
    for k in [int(x) for x in args.ks.split(",")]:
        iv, vv = new(k)
        bv, bidx = base(k)
        torch.cuda.synchronize()
        same_vals = bool(torch.equal(vv.view(torch.int32), bv.contiguous().view(torch.int32)))
        for _ in range(args.warmup):
            new(k)
            base(k)
        torch.cuda.synchronize()
        tn, tb = [], []
        for _ in range(args.repeats):
            tn.append(timed(new, k))
            tb.append(timed(base, k))
        tn, tb = np.array(tn), np.array(tb)
        mem_new = peak_extra(new, k)
        mem_base = peak_extra(lambda kk: base(kk, torch.empty(B, N, device=e.dev, dtype=torch.float32)), k) \
            + seen.numel() * seen.element_size()
        bytes_new = e.Np * e.Hp[0] * es + e.Bp * e.Hp[0] * es + n_seen * 4
        bytes_base = e.Np * e.Hp[0] * 4 + e.Bp * e.Hp[0] * es + 4 * B * N * 4 + B * N
        met = bool(tn.mean() < tb.mean() - (tn.std() + tb.std()))
        line["k%d" % k] = dict(
            new_ms=dict(mean=float(tn.mean()), std=float(tn.std()), min=float(tn.min()), max=float(tn.max())),
            baseline_ms=dict(mean=float(tb.mean()), std=float(tb.std()), min=float(tb.min()), max=float(tb.max())),
            ratio_baseline_over_new=float(tb.mean() / tn.mean()), bar_met=met,
            values_equal_bitwise=same_vals,
            peak_extra_bytes=dict(new=mem_new, baseline=mem_base),
            algorithmic_bytes=dict(new=int(bytes_new), baseline=int(bytes_base)),
            achieved_TBps=dict(new=float(bytes_new / (tn.mean() * 1e-3) / 1e12),
                               baseline=float(bytes_base / (tb.mean() * 1e-3) / 1e12), hbm_peak=8.0))
        if not met:
            line["k%d" % k]["note"] = ("bar NOT met: the new path's mean is not below the baseline's by more than "
                                       "the two spreads combined")
    s = json.dumps(line)
    print(s)
    out = args.out or os.path.join(ROOT, "profiles", "recommend_%s.json" % args.config)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(s + "\n")


if __name__ == "__main__":
    main()
