#!/usr/bin/env python
"""Times per-entry predictions of test batches three ways, in one process on one device:

  new   what Model.predict_entries runs per batch: the generator batch's scatter, the eval-mode forward and
        Engine.predict_entries (ocf_predict_entries: one decoder weight row per held-out entry, no [B, N] array)
  (a)   the route there was before it: Model.predict on the same batch as dense [B, N] inputs and output mask (held
        on the device, built outside the timing), then indexing the target positions out of the dense [B, N] output
  (b)   Model.evaluate_sse's step on the same batch (scatter, forward, the loss launch): it reads the same decoder
        rows for the squared sum only, so new - (b) is what writing the predictions costs, and what moving the
        evaluation onto the forward-only kernel could save

at a BASELINE.json configuration (synthetic_fixed_split, the fixed split's test batches, B = 256, H = 500, f16,
synthetic weights).  The decoder halves are also timed alone from the same hidden activations: Engine.predict_entries
against Engine.predict_dense + the indexing.  Device events; every route warmed up; the routes alternate for
--repeats rounds of --inner passes over --batches batches.  Prints one JSON line and writes it to
profiles/predict_entries_<config>.json.  The condition: new is not slower than (a) (its mean not above (a)'s by more
than the two spreads combined); the line says whether it is met.  Achieved bytes/s (algorithmic bytes over time) is
information, not a bar.

Only the batch's rows matter for the timing (N, H, B and the entries per row), so the synthetic matrix is built with
--rows rows at the configuration's density instead of all of them.

    python tools/predict_entries_bench.py --config ml20m
    python tools/predict_entries_bench.py --config netflix
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
    ap.add_argument("--rows", type=int, default=4096, help="rows of the synthetic matrix (0: the configuration's)")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
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
    test = lambda: rd.data_gen(B, None, "test", False, None, -1)
    gen = test()
    m._check_gen(gen)
    gen._start()
    nb = min(args.batches, gen.num_batches)
    if nb < 1:
        ap.error("the test split has no full batch at --rows %d" % rows)
    # route (a)'s inputs: the dense batches and the positions to index, on the device, outside the timing
    gd = test()
    dense, where, queries = [], [], []
    tgt = data.test_tgt
    for bi in range(nb):
        inputs, _ = next(gd)[:2]
        dense.append([t.contiguous() for t in inputs])
        r = gen.rows_host[bi]
        lens = tgt.row_lengths()[r]
        b_of = np.repeat(np.arange(B), lens)
        cols = np.concatenate([tgt.col[tgt.row_ptr[x]:tgt.row_ptr[x + 1]] for x in r]).astype(np.int64)
        where.append((torch.as_tensor(b_of, device=e.dev), torch.as_tensor(cols, device=e.dev)))
        queries.append(dict(gen.gather_tables(bi)["dec"], aux=gen.aux, E=int(gen.tlocal[bi])))
    entries = int(sum(q["E"] for q in queries))
    torch.cuda.synchronize()

    def load(bi):
        m._load(None, gen, bi)
        e.forward(training=False)

    def new(bi):
        load(bi)
        return e.predict_entries(dict(queries[bi], flag=e.tflag))[0]

    def route_a(bi):
        return m.predict(dense[bi])[where[bi]]

    def route_b(bi):
        m._load(None, gen, bi)
        e.eval_step()

    dense_out = torch.empty(B, N, device=e.dev, dtype=torch.float32)

    def dec_new(bi):
        return e.predict_entries(dict(queries[bi], flag=e.tflag))[0]

    def dec_a(bi):
        e.predict_dense(dense[bi][-1], dense_out)
        return dense_out[where[bi]]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            for bi in range(nb):
                fn(bi)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / (args.inner * nb)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(0)
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - before)

    # the same numbers from both routes (fp32 accumulation of the same rounded operands, another order)
    diff = 0.0
    for bi in range(nb):
        diff = max(diff, float((new(bi) - route_a(bi)).abs().max()))
    routes = dict(new=new, a=route_a, b=route_b)
    for _ in range(args.warmup):
        for fn in routes.values():
            for bi in range(nb):
                fn(bi)
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(args.repeats):
        for k, fn in routes.items():
            t[k].append(timed(fn))
    e.take_stats()
    # the decoder halves alone, from the hidden activations of the last batch loaded
    load(nb - 1)
    e._finish_deferred_encoder()
    last = nb - 1
    halves = dict(new=lambda bi: dec_new(last), a=lambda bi: dec_a(last))
    for _ in range(args.warmup):
        for fn in halves.values():
            fn(0)
    td = {k: [] for k in halves}
    for _ in range(args.repeats):
        for k, fn in halves.items():
            td[k].append(timed(fn))
    mem = dict(new=peak_extra(new), a=peak_extra(route_a) + sum(x.numel() * x.element_size() for x in dense[0]),
               b=peak_extra(route_b))
    e.take_stats()

    es = 4 if args.dtype == "float32" else 2
    Hp = e.Hp[0]
    E1 = entries / nb
    bytes_new = E1 * Hp * es + E1 * (4 + 4 + 1 + 4 + 4) + e.Bp * Hp * es
    bytes_a = e.Np * Hp * 4 + e.Bp * Hp * es + 2 * B * N * 4 + E1 * (8 + 8 + 4 + 4)
    stat = lambda x: dict(mean=float(np.mean(x)), std=float(np.std(x)), min=float(np.min(x)), max=float(np.max(x)))
    tn, ta, tb = (np.array(t[k]) for k in ("new", "a", "b"))
    met = bool(tn.mean() <= ta.mean() + (tn.std() + ta.std()))
    Wt, _ = e._wop(1)
    line = dict(tool="predict_entries_bench", config=args.config, N=N, B=B, H=H, dtype=args.dtype, matrix_rows=rows,
                batches=nb, entries_per_batch=E1, repeats=args.repeats, inner=args.inner,
                device=torch.cuda.get_device_name(0), operand="shadow" if Wt is not e.W[1] else "master",
                route_ms_per_batch=dict(new=stat(tn), a_predict_then_index=stat(ta), b_eval_step=stat(tb)),
                ratio_a_over_new=float(ta.mean() / tn.mean()), ratio_b_over_new=float(tb.mean() / tn.mean()),
                condition_new_not_slower_than_a=met,
                decoder_only_ms=dict(new=stat(td["new"]), a_predict_dense_then_index=stat(td["a"]),
                                     ratio_a_over_new=float(np.mean(td["a"]) / np.mean(td["new"]))),
                max_abs_difference_new_vs_a=diff,
                peak_extra_bytes=dict(new=mem["new"], a_with_its_dense_inputs=mem["a"], b=mem["b"]),
                algorithmic_bytes_decoder=dict(new=int(bytes_new), a=int(bytes_a)),
                achieved_TBps_decoder=dict(new=float(bytes_new / (np.mean(td["new"]) * 1e-3) / 1e12),
                                           a=float(bytes_a / (np.mean(td["a"]) * 1e-3) / 1e12), hbm_peak=8.0))
    if not met:
        line["note"] = "condition NOT met: the new route's mean is above route (a)'s by more than the two spreads combined"
    s = json.dumps(line)
    print(s)
    out = args.out or os.path.join(ROOT, "profiles", "predict_entries_%s.json" % args.config)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(s + "\n")


if __name__ == "__main__":
    main()
