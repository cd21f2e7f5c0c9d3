#!/usr/bin/env python
"""Times per-column top-K (k rows for every column: k items for every user of an item-row model) two ways from the
same weights and the same catalogue, in one process:

  new       Engine.encode_rows (every candidate row's hidden code, one table [R_p, Hp]) + Engine.topk_columns (the
            transposed ocf_topk: decoder weight rows on the M side, the codes on the N side, seen rows excluded
            through the transposed input CSR); no [R, N] array.  The two parts are also timed on their own.
  baseline  what the same answer took before: the same forward per batch, Engine.predict_dense of every batch into
            one [R_p, N] fp32 tensor, masked_fill of the same exclusions (the boolean mask is built once, outside the
            timing), torch.topk over dim 0

at a BASELINE.json configuration's width AND row count (synthetic_fixed_split; H = 500, B = 256, f16), for k = 10
and k = 100.  Device events; both warmed up; the two alternate for --repeats rounds of --inner calls each.  Prints
one JSON line and writes it to profiles/recommend_columns_<config>.json.  The bar: the new path's mean below the
baseline's by more than the two spreads (standard deviations over the rounds) combined; the line says whether it is
met.  Peak extra device memory of both paths is recorded (the baseline's includes its mask).

    python tools/recommend_columns_bench.py --config ml20m
    python tools/recommend_columns_bench.py --config netflix
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--split", default="valid", choices=["train", "valid", "test"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats >= 5")

    import torch
    from omnidirectional_collaborative_filtering_amd import optimizers as O
    from omnidirectional_collaborative_filtering_amd.data_reader import data_reader
    from omnidirectional_collaborative_filtering_amd.dataset import synthetic_fixed_split
    from omnidirectional_collaborative_filtering_amd.model import omni_model

    t0 = time.time()
    data = synthetic_fixed_split(args.config, seed=0)
    N, B, H = data.num_cols, args.batch, args.hidden
    np.random.seed(0)
    rd = data_reader(N, data.train.n_rows, dataset=data, eval_mode="fixed_split")
    om = omni_model(1, H, N, B, dense_activation="sigmoid", use_causal_info=False, compute_dtype=args.dtype, seed=3)
    m, e = om.model, om.engine
    m.compile(O.Adagrad(lr=0.005, epsilon=1e-8), "mean_squared_error")
    cat = rd.catalogue(args.split)
    R = cat["n"]
    Rp = -(-R // 128) * 128
    t = cat["seen"].tiles(Rp)
    seg = dict(ex_rp=cat["seen"].rp, ex_tptr=t["t_tptr"], ex_col=t["t_col"], ex_ntiles=t["t_ntiles"])
    nb = -(-R // B)
    # the baseline's exclusion mask [R, N], built once
    inputs = cat["inputs"].host
    rows_i = torch.as_tensor(np.repeat(np.arange(R, dtype=np.int64), inputs.row_lengths()[:R]), device=e.dev)
    seen = torch.zeros(R, N, dtype=torch.bool, device=e.dev)
    seen[rows_i, torch.as_tensor(inputs.col.astype(np.int64), device=e.dev)] = True
    n_seen = int(inputs.nnz)
    del rows_i
    scores = torch.empty(max(nb * B, Rp), N, device=e.dev, dtype=torch.float32)
    torch.cuda.synchronize()
    setup_s = time.time() - t0

    def encode():
        return e.encode_rows(rd.catalogue_gen(B, args.split))

    state = {}

    def select(k):
        return e.topk_columns(state["codes"], R, k, exclude=seg, groups=args.groups or None)

    def new(k):
        state["codes"] = encode()
        return select(k)

    def base(k, out=None):
        out = scores if out is None else out
        gen = rd.catalogue_gen(B, args.split)
        while True:
            bi = gen.next_batch_index()
            if bi is None:
                break
            m._load(None, gen, bi)
            e.forward(training=False)
            e._finish_deferred_encoder()
            e.predict_dense(None, out[bi * B:(bi + 1) * B])
        s = out[:R]
        s.masked_fill_(seen, float("-inf"))
        return torch.topk(s, k, dim=0)

    def timed(fn, *a):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        for _ in range(args.inner):
            fn(*a)
        y.record()
        y.synchronize()
        return x.elapsed_time(y) / args.inner

    def peak_extra(fn, *a):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(*a)
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    def stats(x):
        x = np.array(x)
        return dict(mean=float(x.mean()), std=float(x.std()), min=float(x.min()), max=float(x.max()))

    Wt, _ = e._wop(1)
    line = dict(tool="recommend_columns_bench", config=args.config, split=args.split, N=N, R=R, B=B, H=H,
                dtype=args.dtype, seen_entries=n_seen, repeats=args.repeats, inner=args.inner, groups=args.groups,
                device=torch.cuda.get_device_name(0), setup_s=round(setup_s, 1),
                m_operand=("blocked " if e._wblk(1) else "row-major ") + ("shadow" if Wt is not e.W[1] else "master"),
                code_table_bytes=int(Rp * e.Hp[0] * (4 if args.dtype == "float32" else 2)))
    for k in [int(x) for x in args.ks.split(",")]:
        iv, vv = new(k)
        bv, _ = base(k)
        torch.cuda.synchronize()
        same_vals = bool(torch.equal(vv.view(torch.int32), bv.t().contiguous().view(torch.int32)))
        for _ in range(args.warmup):
            new(k)
            base(k)
        torch.cuda.synchronize()
        tn, tb, te, ts = [], [], [], []
        for _ in range(args.repeats):
            tn.append(timed(new, k))
            tb.append(timed(base, k))
            te.append(timed(encode))
            ts.append(timed(select, k))
        tn, tb = np.array(tn), np.array(tb)
        e._topk_work = None                      # count the candidate workspace too: it is the path's own
        mem_new = peak_extra(new, k)
        mem_base = peak_extra(lambda kk: base(kk, torch.empty(scores.shape, device=e.dev, dtype=torch.float32)), k) \
            + seen.numel() * seen.element_size()
        met = bool(tn.mean() < tb.mean() - (tn.std() + tb.std()))
        line["k%d" % k] = dict(new_ms=stats(tn), baseline_ms=stats(tb), encode_ms=stats(te), select_merge_ms=stats(ts),
                               ratio_baseline_over_new=float(tb.mean() / tn.mean()), bar_met=met,
                               values_equal_bitwise=same_vals,
                               peak_extra_bytes=dict(new=mem_new, baseline=mem_base))
        if not met:
            line["k%d" % k]["note"] = ("bar NOT met: the new path's mean is not below the baseline's by more than "
                                       "the two spreads combined")
    s = json.dumps(line)
    print(s)
    out = args.out or os.path.join(ROOT, "profiles", "recommend_columns_%s.json" % args.config)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(s + "\n")


if __name__ == "__main__":
    main()
