#!/usr/bin/env python
"""Times generator training with Adam, Adadelta and Adamax against each other, in one process on one device.

The three keep the same state per parameter (the fp32 weight and two fp32 slots, read and written once per step), so
Adam in the same run is the yardstick for the other two: the ratios adadelta / adam and adamax / adam are the result.
One model per optimizer at a BASELINE.json configuration (synthetic_fixed_split; B = 256, H = 500, f16 by default),
trained through Model.fit_generator over --steps batches of the train split; device events around each call; every
model warmed up; the three alternate for --repeats rounds, so drift of the box hits all of them alike.  Prints one JSON
line and writes it to profiles/optimizers_<config>.json.  A ratio above 1.10 is flagged in the line ("over_10_percent");
DESIGN.md explains such a case from the kernels' resource usage.

Only the batch's rows matter for the step time (N, H, B and the entries per row), so the synthetic matrix is built with
--rows rows at the configuration's density instead of all of them.

    python tools/optimizer_bench.py --config ml20m
    python tools/optimizer_bench.py --config ml1m
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("adam", "adadelta", "adamax")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ml20m", choices=["ml100k", "ml1m", "ml1m_u", "ml20m", "netflix"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=500)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--rows", type=int, default=4096, help="rows of the synthetic matrix (0: the configuration's)")
    ap.add_argument("--steps", type=int, default=10, help="batches per timed fit_generator call")
    ap.add_argument("--repeats", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
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
    train = lambda: rd.data_gen(B, [1.0, 1.0], "train", True, None, -1, pass_through_input_training=True)
    models = {}
    for name in NAMES:
        om = omni_model(1, H, N, B, dense_activation="sigmoid", use_causal_info=False, dropout_probability=0.2,
                        compute_dtype=args.dtype, seed=3)
        om.model.compile(O.get(name), "mean_squared_error")
        models[name] = om
    steps = min(args.steps, train().num_batches)
    if steps < 1:
        ap.error("the train split has no full batch at --rows %d" % rows)

    def timed(name):
        m = models[name].model
        gen = train()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        h = m.fit_generator(gen, steps, epochs=1, verbose=0)
        b.record()
        b.synchronize()
        loss = h.history["loss"][0]
        if not np.isfinite(loss):
            raise RuntimeError("%s: the loss is not finite" % name)
        return a.elapsed_time(b) / steps

    for _ in range(args.warmup):
        for name in NAMES:
            timed(name)
    t = {k: [] for k in NAMES}
    for _ in range(args.repeats):
        for name in NAMES:
            t[name].append(timed(name))
    paths = {k: dict(models[k].engine.step_paths) for k in NAMES}

    stat = lambda x: dict(mean=float(np.mean(x)), median=float(np.median(x)), std=float(np.std(x)),
                          min=float(np.min(x)), max=float(np.max(x)))
    med = {k: float(np.median(t[k])) for k in NAMES}
    ratios = {k: med[k] / med["adam"] for k in ("adadelta", "adamax")}
    line = dict(tool="optimizer_bench", config=args.config, N=N, B=B, H=H, dtype=args.dtype, matrix_rows=rows,
                steps_per_call=steps, repeats=args.repeats, device=torch.cuda.get_device_name(0),
                ms_per_step={k: stat(t[k]) for k in NAMES}, yardstick="adam, same run",
                ratio_of_medians_to_adam=ratios, over_10_percent=[k for k, r in ratios.items() if r > 1.10],
                state_bytes_per_parameter=24, step_paths=paths)
    s = json.dumps(line)
    print(s)
    out = args.out or os.path.join(ROOT, "profiles", "optimizers_%s.json" % args.config)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(s + "\n")


if __name__ == "__main__":
    main()
