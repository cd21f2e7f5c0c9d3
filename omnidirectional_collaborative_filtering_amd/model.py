"""Drop-in for the reference's ``omni_model`` (model.py:33-99) and the Keras ``Model`` subset that
train.py / train_jester.py use: compile, fit_generator, evaluate_generator, predict, fit,
train_on_batch, test_on_batch, save, metrics_names, get_weights / set_weights.

Graph (model.py:43-99):  x = concat([data, observed_mask?, second_mask?]);
L x [Dense(H, act) -> Dropout(p, noise_shape=[B, H])] ; y = output_mask * Dense(N, linear)(x)
Loss: Keras 'mean_squared_error' (train.py:49), or 'mean_absolute_error' / 'huber' / 'logcosh' (losses.py).
Everything runs through engine.Engine on the GPU.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import losses
from . import metrics as M
from . import optimizers
from .data_reader import BatchGenerator
from .engine import Engine


class History(object):
    def __init__(self):
        self.history = {}
        self.epoch = []


class EarlyStopping(object):
    """keras.callbacks.EarlyStopping(monitor, min_delta, patience, mode='auto') as train_jester.py:65 uses it."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, verbose=0, mode="auto"):
        self.monitor, self.min_delta, self.patience = monitor, min_delta, patience
        self.best = np.inf
        self.wait = 0
        self.stop = False

    def on_epoch_end(self, logs):
        v = logs.get(self.monitor)
        if v is None:
            return
        if v < self.best - self.min_delta:
            self.best, self.wait = v, 0
        else:
            self.wait += 1
            if self.wait > self.patience:
                self.stop = True


class Model(object):
    def __init__(self, engine, use_causal_info, use_both_masks, rating_range=1.0):
        self.engine = engine
        self.use_causal_info = use_causal_info
        self.use_both_masks = use_both_masks
        self.optimizer = None
        self.loss = engine.loss
        self.metric_names = []
        self.rating_range = float(rating_range)
        self.stop_training = False
        self.rank, self.world, self.dp = 0, 1, None
        # feature parallelism (engine built with shard / comm): (rank, world) for per-shard checkpoints
        self.fp = None

    def enable_data_parallel(self, rank, world, mode="sharded", grad_dtype="float32"):
        """Row data parallelism (parallel.DataParallel): call on every rank after torch.distributed is
        initialised and the model is compiled; rank 0's weights are broadcast."""
        from .parallel import DataParallel
        if int(world) > 1 and self.loss.code != losses.MeanSquaredError.code:
            raise NotImplementedError("loss %r is not implemented under data parallelism (only "
                                      "'mean_squared_error' is)" % (self.loss.name,))
        if int(world) > 1 and self.optimizer is not None:
            optimizers.check_single_gpu(self.optimizer, "data parallelism")
        if self.engine.comm is not None:
            raise ValueError("data parallelism over a feature-parallel (column-sharded) engine is not supported")
        self.rank, self.world = int(rank), int(world)
        self.dp = DataParallel(self.engine, rank, world, mode=mode, grad_dtype=grad_dtype) if world > 1 else None

    def enable_feature_parallel(self, rank, world):
        """record the column-shard layout (the engine was built with shard=/comm=) for checkpoints"""
        if int(world) > 1 and self.optimizer is not None:
            optimizers.check_single_gpu(self.optimizer, "feature parallelism")
        self.fp = (int(rank), int(world))

    def _train_one(self, gen):
        """One optimizer step; under data parallelism rank r takes the r-th of the next `world` batches."""
        if self.world > 1 and isinstance(gen, BatchGenerator):
            gen.dp_shard = (self.rank, self.world)
            idx = [gen.next_batch_index() for _ in range(self.world)]
            if idx[-1] is None:
                raise StopIteration("generator exhausted")
            self._check_gen(gen)
            self._load(None, gen, idx[self.rank])
        elif self.dp is None and isinstance(gen, BatchGenerator):
            self._check_gen(gen)
            bi = gen.next_batch_index()
            if bi is None:
                raise StopIteration("generator exhausted (data_reader.py:418 yields None)")
            # the whole step in one library call when the engine's template applies (Engine.fast_train_step)
            if not self.engine.fast_train_step(gen, bi):
                self._load(None, gen, bi)
                self.engine.train_step()
            return
        else:
            self._pull(gen)
        if self.dp is not None:
            self.dp.step()
        else:
            self.engine.train_step()

    # ------------------------------------------------------------------ compile
    def compile(self, optimizer, loss="mean_squared_error", metrics=None, rating_range=None, loss_params=None):
        """loss: 'mean_squared_error' / 'mse' (train.py:49), 'mean_absolute_error' / 'mae', 'huber' (with
        loss_params={"delta": d}, default 1.0), 'logcosh', or a losses.Loss instance.  ValueError for an unknown
        name or a bad delta; NotImplementedError for a Keras loss that is not built, and for any loss but the
        squared one on a multi-GPU layout (feature or data parallel)."""
        loss = losses.get(loss, loss_params)
        if loss.code != losses.MeanSquaredError.code and self.dp is not None:
            raise NotImplementedError("loss %r is not implemented under data parallelism (only "
                                      "'mean_squared_error' is)" % (loss.name,))
        optimizer = optimizers.get(optimizer)
        if self.dp is not None:
            optimizers.check_single_gpu(optimizer, "data parallelism")
        if self.fp is not None and self.fp[1] > 1:
            optimizers.check_single_gpu(optimizer, "feature parallelism")
        self.engine.set_loss(loss)
        self.loss = loss
        self.engine.set_optimizer(optimizer)
        self.optimizer = optimizer
        self.metric_names = [M.metric_name(m) for m in (metrics or [])]
        if rating_range is not None:
            self.rating_range = float(rating_range)

    @property
    def metrics_names(self):
        return ["loss"] + list(self.metric_names)

    def _take_stats(self):
        """Engine.take_stats with the steps' sums of rho(e), the compiled loss's numerator"""
        return self.engine.take_stats(loss_sums=True)

    def _logs_from_stats(self, st, rows=None):
        """st: ([steps, 4 + Bp] device stats, [steps] sums of rho(e)) from _take_stats -> epoch-mean logs.  rows:
        the row count of every step's batch (None: all full) -- Keras weights each batch's values by its size
        (BaseLogger for the training logs, _test_loop for evaluation), which matters only for Model.fit's trailing
        partial batch."""
        e = self.engine
        B = e.B
        st, rho = st
        rows = [B] * len(st) if rows is None else list(rows)
        assert len(rows) == len(st)
        out = {k: [] for k in self.metrics_names}
        for row, lsum, b in zip(st, rho, rows):
            sse, sae, cnt = row[0], row[1], row[2]
            # Keras' total loss = the mean of rho(e) over all b * N elements (MSE: rho = e^2, the SSE) + the
            # kernels' l2 penalty (row[3], 0 without l2); metrics have none
            out["loss"].append(lsum / (b * e.N_total) + row[3])
            for name in self.metric_names:
                out[name].append(M.from_stats(name, sse, sae, cnt, row[4:], B, e.N_total, self.rating_range, rows=b))
        w = np.asarray(rows, np.float64)
        return {k: float(np.dot(v, w) / w.sum()) if v else float("nan") for k, v in out.items()}

    # ------------------------------------------------------------------ batch plumbing
    def _split_inputs(self, x):
        """model.py:89-97 input order -> (layer-0 blocks, output mask)."""
        x = list(x)
        if self.use_causal_info:
            blocks = [x[0], x[1]]
            out_mask = x[2]
            rest = x[3:]
        else:
            blocks = [x[0]]
            out_mask = x[1]
            rest = x[2:]
        if self.use_both_masks:
            blocks.append(rest[0])
        return blocks, out_mask

    def _load(self, item, gen=None, bi=None):
        e = self.engine
        if gen is not None:
            args = gen.scatter_args(bi, engine_args=e.scatter_args())
            e.load_batch(args, gen.targets(bi, e.N), gather=gen.gather_tables(bi))
            return gen.target_count(bi)
        x, y = item[0], item[1]
        blocks, out_mask = self._split_inputs(x)
        e.load_dense(blocks, out_mask, y)
        return item[2] if len(item) > 2 else None

    def _pull(self, gen):
        if isinstance(gen, BatchGenerator):
            self._check_gen(gen)
            bi = gen.next_batch_index()
            if bi is None:
                raise StopIteration("generator exhausted (data_reader.py:418 yields None)")
            return self._load(None, gen, bi)
        item = next(gen)
        if item is None:
            raise StopIteration("generator yielded None")
        return self._load(item)

    def _check_gen(self, gen):
        e = self.engine
        if gen.B != e.B:
            raise ValueError("generator batch_size %d != model batch_size %d (Dropout noise_shape, model.py:73)"
                             % (gen.B, e.B))
        want_k = 1 + int(self.use_causal_info) + int(self.use_both_masks)
        have_k = 1 + int(gen.aux_type is not None) + int(gen.aux_type == "both")
        if want_k != have_k:
            raise ValueError("auxilliary_mask_type=%r does not match the model inputs" % (gen.aux_type,))

    # ------------------------------------------------------------------ training
    def train_on_batch(self, x, y):
        self._load((x, y))
        self.engine.train_step()
        return self._finish(self._take_stats())

    def test_on_batch(self, x, y):
        self._load((x, y))
        self.engine.eval_step()
        return self._finish(self._take_stats())

    def _finish(self, st):
        logs = self._logs_from_stats(st)
        vals = [logs[k] for k in self.metrics_names]
        return vals[0] if len(vals) == 1 else vals

    def fit_generator(self, generator, steps_per_epoch, epochs=1, verbose=1, callbacks=None, validation_data=None,
                      validation_steps=None, initial_epoch=0, **kw):
        hist = History()
        callbacks = callbacks or []
        steps = int(steps_per_epoch)
        for epoch in range(initial_epoch, epochs):
            t0 = time.time()
            for _ in range(steps // self.world if self.world > 1 else steps):
                self._train_one(generator)
            logs = self._logs_from_stats(self._take_stats())
            if self.world > 1:
                logs = self._mean_over_ranks(logs)
            if validation_data is not None:
                vals = self.evaluate_generator(validation_data, validation_steps)
                vals = vals if isinstance(vals, list) else [vals]
                for k, v in zip(self.metrics_names, vals):
                    logs["val_" + k] = v
            for k, v in logs.items():
                hist.history.setdefault(k, []).append(v)
            hist.epoch.append(epoch)
            if verbose:
                print("Epoch %d - %.1fs - " % (epoch + 1, time.time() - t0) +
                      " - ".join("%s: %.4f" % kv for kv in logs.items()))
            for cb in callbacks:
                cb.on_epoch_end(logs)
                self.stop_training |= getattr(cb, "stop", False)
            if self.stop_training:
                break
        return hist

    def _mean_over_ranks(self, logs):
        import torch.distributed as dist
        keys = sorted(logs)
        t = torch.tensor([logs[k] for k in keys], dtype=torch.float64, device=self.engine.dev)
        dist.all_reduce(t)
        return {k: float(v) / self.world for k, v in zip(keys, t.tolist())}

    def evaluate_generator(self, generator, steps, **kw):
        steps = int(steps)
        self.engine.take_stats()
        for _ in range(steps):
            self._pull(generator)
            self.engine.eval_step()
        return self._finish(self._take_stats())

    def evaluate_sse(self, generator, steps):
        """Fused form of train.py:225-255: (sum of squared errors, sum of target_count)."""
        self.engine.take_stats()
        count = 0
        for _ in range(int(steps)):
            c = self._pull(generator)
            self.engine.eval_step()
            count += int(c) if c is not None else 0
        st = self.engine.take_stats()
        return float(st[:, 0].sum()), count

    def predict(self, x, batch_size=None, verbose=0):
        """Returns y = output_mask * (h W_out + b_out) as a float32 CUDA tensor [B, N].

        Collective under data parallelism with ZeRO-1 (enable_data_parallel(mode="sharded")): the output
        layer reads the fp32 masters, which each rank holds only 1/G of, so every rank must call predict
        together (the masters are all-gathered first); a rank-0-only predict would wait forever."""
        e = self.engine
        blocks, out_mask = self._split_inputs(x)
        dummy_t = torch.zeros(e.B, e.N, device=e.dev)
        e.load_dense(blocks, out_mask, dummy_t)
        e.forward(training=False)
        out = torch.empty(e.B, e.N, device=e.dev, dtype=torch.float32)
        om = out_mask if torch.is_tensor(out_mask) else torch.as_tensor(np.asarray(out_mask, np.float32))
        om = om.to(e.dev, torch.float32).contiguous()
        e.predict_dense(om, out)
        return out

    def predict_entries(self, generator, steps, queries=None, clip=None):
        """The predictions themselves at listed entries of `steps` generator batches (engine.Engine.predict_entries:
        one decoder weight row read per entry, no dense [B, N] input, mask or output anywhere).

        queries=None: a valid or test generator; the entries are those of the split's target CSR at the batch rows
        whose live-target flag is set -- the set evaluate_sse counts.  queries = a dataset.RatingsCSR with as many
        rows as the generator's input CSR (row i = the same dataset row; RatingsCSR.from_coo, values optional):
        every entry of it is predicted, with any generator; statistics only if it carries values.
        clip: (lo, hi) or None; the statistics are taken on the clipped predictions.

        Returns a dict: rows (int64 dataset row per entry), cols (int32), targets (fp32 or None), predictions (fp32)
        as CUDA tensors, in batch order, then batch-row order, then the CSR's list order; sse, sae, count (floats
        from the device totals; None without targets) and rmse = sqrt(sse / entries).
        Collective under data parallelism with ZeRO-1, like predict.  The generator advances as it does under
        evaluate_generator; nothing of the training state changes."""
        if not isinstance(generator, BatchGenerator):
            raise ValueError("predict_entries takes a data_reader.data_gen generator (dense batches: predict)")
        if queries is None and generator.split == "train":
            raise ValueError("predict_entries needs a valid or test generator (a train generator has no held-out "
                             "entries), or a queries CSR")
        if clip is not None and not float(clip[0]) <= float(clip[1]):
            raise ValueError("predict_entries: clip = (lo, hi) with lo <= hi")
        e, gen, B = self.engine, generator, generator.B
        self._check_gen(gen)
        dev = e.dev
        qt = None
        out = dict(rows=[], cols=[], targets=[], predictions=[], flags=[])
        totals = []
        for _ in range(int(steps)):
            bi = gen.next_batch_index()
            if bi is None:
                raise StopIteration("generator exhausted (data_reader.py:418 yields None)")
            self._load(None, gen, bi)
            e.forward(training=False)
            rows_b = gen.rows_dev.view(-1)[bi * B:(bi + 1) * B]
            if queries is None:
                tab, src = gen.gather_tables(bi)["dec"], gen.src2
                rp, col, val = src.rp, src.col, src.val
                lb = gen.lboff2_dev[bi]
                E = int(gen.tlocal[bi])
                q = dict(tab, flag=e.tflag, aux=gen.aux, E=E)
            else:
                if qt is None:
                    qt = self._query_tables(gen, queries)
                rp, col, val = qt["rp"], qt["col"], qt["val"]
                lb = qt["lboff"][bi]
                E = int(qt["E"][bi])
                ch = qt["chunks"]
                c0 = int(ch["cbase"][bi])
                q = dict(rows=rows_b, rp=rp, col=col, val=val, lboff=lb, flag=None, aux=gen.aux, E=E,
                         ch_row=ch["ch_row"].data_ptr() + 4 * c0, ch_j0=ch["ch_j0"].data_ptr() + 4 * c0,
                         ch_j1=ch["ch_j1"].data_ptr() + 4 * c0, n_chunks=int(ch["cbase"][bi + 1]) - c0)
            y, _, total = e.predict_entries(q, clip=clip)
            # (dataset row, column, target) of every batch-local entry, on the device
            eb = torch.repeat_interleave(torch.arange(B, device=dev), lb[1:] - lb[:-1], output_size=E)
            r = rows_b[eb].to(torch.int64)
            pos = rp[r] + (torch.arange(E, device=dev) - lb[eb])
            out["rows"].append(r)
            out["cols"].append(col[pos])
            out["predictions"].append(y)
            if val is not None:
                out["targets"].append(val[pos])
                totals.append(total)
            if queries is None:
                out["flags"].append(e.tflag[:E].clone())
        cat = lambda xs, dt: torch.cat(xs) if xs else torch.zeros(0, device=dev, dtype=dt)
        res = dict(rows=cat(out["rows"], torch.int64), cols=cat(out["cols"], torch.int32),
                   predictions=cat(out["predictions"], torch.float32),
                   targets=cat(out["targets"], torch.float32) if (queries is None or queries.val is not None) else None)
        if queries is None:                # the kernel writes every entry; the entries that are no live target leave
            live = cat(out["flags"], torch.uint8) != 0
            for k in ("rows", "cols", "predictions", "targets"):
                res[k] = res[k][live]
        res.update(sse=None, sae=None, count=None, rmse=None)
        if res["targets"] is not None:
            t = torch.stack(totals).double().sum(0).tolist() if totals else [0.0, 0.0, 0.0, 0.0]
            n = int(res["predictions"].numel())
            res.update(sse=float(t[0]), sae=float(t[1]), count=float(t[2]),
                       rmse=float(np.sqrt(t[0] / n)) if n else float("nan"))
        return res

    def _query_tables(self, gen, queries):
        """a queries CSR on the device with the batch-local offsets and chunk tables of the generator's epoch plan"""
        src1 = gen.src1.host
        if queries.n_rows != src1.n_rows:
            raise ValueError("predict_entries: queries has %d rows, the generator's input CSR %d (row i is the same "
                             "dataset row)" % (queries.n_rows, src1.n_rows))
        e = self.engine
        if queries.nnz and (int(queries.col.min()) < 0 or int(queries.col.max()) >= e.N):
            raise ValueError("predict_entries: a queries column lies outside [0, %d)" % e.N)
        dev = e.dev
        lens = queries.row_lengths()
        lboff = BatchGenerator._local_offsets(lens, gen.rows_host)
        return dict(rp=torch.as_tensor(queries.row_ptr, device=dev), col=torch.as_tensor(queries.col, device=dev),
                    val=None if queries.val is None else torch.as_tensor(queries.val, device=dev),
                    lboff=torch.as_tensor(lboff, device=dev), E=lboff[:, -1],
                    chunks=BatchGenerator._chunk_tables(lens, gen.rows_host, dev))

    # ------------------------------------------------------------------ recommendations (engine.Engine.topk)
    # The k best columns of every batch row straight from the decoder GEMM (ocf.h ocf_topk): no [B, N] score
    # matrix is written, the scores are bit-identical to predict's with an all-ones output mask, ordered by
    # descending score and, for equal scores, ascending column; rows with fewer than k eligible columns end in
    # (-1, -inf).  The lists run along the batch row, whatever the model's orientation.  Like predict, the three
    # methods are collective under data parallelism with ZeRO-1 (the fp32 masters are all-gathered first): every
    # rank must call them together.  Nothing of the training state changes (no stats row, no optimizer step).
    def recommend_on_batch(self, x, k=10, exclude=None):
        """x: dense inputs in predict's order.  exclude: [B, N] array or tensor, nonzero = never recommended.
        Returns (items [B, k] int32, scores [B, k] fp32) as CUDA tensors."""
        e = self.engine
        blocks, _ = self._split_inputs(x)
        zeros = torch.zeros(e.B, e.N, device=e.dev)
        e.load_dense(blocks, zeros, zeros)
        e.forward(training=False)
        if exclude is not None:
            ex = exclude if torch.is_tensor(exclude) else torch.as_tensor(np.asarray(exclude, np.float32))
            if tuple(ex.shape) != (e.B, e.N):
                raise ValueError("exclude has shape %s, expected (%d, %d)" % (tuple(ex.shape), e.B, e.N))
            exclude = ex.to(e.dev, torch.float32).contiguous()
        return e.topk(k, exclude=exclude)

    def _rank_batch(self, gen, k, exclude_seen, relevance_min=None, relevance=False):
        """next batch of the generator -> (rows, Engine.topk's result)"""
        e = self.engine
        self._check_gen(gen)
        bi = gen.next_batch_index()
        if bi is None:
            raise StopIteration("generator exhausted (data_reader.py:418 yields None)")
        self._load(None, gen, bi)
        e.forward(training=False)
        rows_ptr = gen.rows_dev.data_ptr() + 4 * bi * gen.B
        ex = rel = None
        if exclude_seen:
            t = gen.src1.tiles(e.N)
            ex = dict(ex_rows=rows_ptr, ex_rp=gen.src1.rp, ex_tptr=t["t_tptr"], ex_col=t["t_col"],
                      ex_ntiles=t["t_ntiles"])
        if relevance:
            t = gen.src2.tiles(e.N)
            rel = dict(rel_rows=rows_ptr, rel_rp=gen.src2.rp, rel_col=t["t_col"], rel_val=t["t_val"],
                       rel_min=relevance_min)
        return gen.rows_dev.view(-1)[bi * gen.B:(bi + 1) * gen.B], e.topk(k, exclude=ex, relevance=rel)

    def recommend_generator(self, generator, steps, k=10, exclude_seen=True):
        """BatchGenerator batches of any split (the generator advances as under evaluate_generator).
        exclude_seen: the batch rows' input entries (every entry of the split's input CSR) are never recommended.
        Returns (rows [steps * B] int64 dataset row indices, items [steps * B, k] int32, scores [steps * B, k])."""
        if not isinstance(generator, BatchGenerator):
            raise ValueError("recommend_generator takes a data_reader.data_gen generator (dense batches: "
                             "recommend_on_batch)")
        out = [self._rank_batch(generator, k, exclude_seen) for _ in range(int(steps))]
        return (torch.cat([r for r, _ in out]).to(torch.int64), torch.cat([t[0] for _, t in out]),
                torch.cat([t[1] for _, t in out]))

    def evaluate_ranking(self, generator, steps, k=10, relevance_min=None):
        """Hit rate, recall and NDCG at k of a valid / test generator: the inputs are the split's input ratings,
        seen items are excluded, and the relevant items of a row are its held-out entries with a rating >=
        relevance_min (None: every held-out entry).  The per-row counts come from the merge kernel; returns
        metrics.ranking_from_rows of them: {"hit_rate@k", "recall@k", "ndcg@k", "rows"}."""
        if not isinstance(generator, BatchGenerator) or generator.split == "train":
            raise ValueError("evaluate_ranking needs a valid or test generator (a train generator has no held-out "
                             "entries)")
        rr = torch.cat([self._rank_batch(generator, k, True, relevance_min, True)[1][2] for _ in range(int(steps))])
        rr = rr.cpu().numpy()
        return M.ranking_from_rows(rr[:, 0], rr[:, 1], rr[:, 2], k)

    # ------------------------------------------------------------------ per-column recommendations
    # The lists above run along the batch row.  For an item-row model (I-AutoRec: rows = items, columns = users)
    # the question is the other one: the k best rows for every column.  The score h_i . W_out[u] + b_out[u] is
    # symmetric in its factors, so every candidate row is encoded once (encode_rows: a table of hidden codes, R x H)
    # and the same select / merge kernels run with the operands exchanged (Engine.topk_columns): the decoder weight
    # rows on the M side, the codes on the N side, exclusion and relevance from the transposed CSRs
    # (dataset.FixedSplit.catalogue).  No [R, N] score array exists anywhere.  Like predict, the three methods are
    # collective under data parallelism with ZeRO-1 (the fp32 masters are all-gathered first): every rank must call
    # them together.  Nothing of the training state changes, and nothing is drawn from NumPy's RNG.
    def _encode_catalogue(self, reader, split, auxilliary_mask_type, aux_var_value):
        gen = reader.catalogue_gen(self.engine.B, split, auxilliary_mask_type, aux_var_value)
        self._check_gen(gen)
        return gen.cat, self.engine.encode_rows(gen)

    def encode_rows(self, reader, split="valid", auxilliary_mask_type=None, aux_var_value=-1):
        """The embedding (last hidden activations, eval mode) of every candidate row of reader's catalogue for
        `split` (dataset.FixedSplit.catalogue: 'train' / 'valid' = the train rows encoded from their train ratings;
        'test' = those plus the rows first seen in validation, encoded from their test inputs).  The causal /
        dropout mask feeds mark the row's input entries.  Returns (keys, codes): the row keys and a CUDA tensor
        [R, H] in the compute dtype.  Collective under ZeRO-1 data parallelism, like predict."""
        cat, codes = self._encode_catalogue(reader, split, auxilliary_mask_type, aux_var_value)
        return cat["keys"], codes[:cat["n"], :self.engine.H[-1]]

    def recommend_columns(self, reader, split="valid", k=10, exclude_seen=True, columns=None,
                          auxilliary_mask_type=None, aux_var_value=-1):
        """The k best candidate rows for every column (for an item-row model: k items for every user).
        exclude_seen: the rows a column has an input rating for are never recommended to it.  columns: None = every
        column, or a list of column indices.  Returns (keys, items [C, k] int32 positions into keys, -1 past the
        eligible rows, scores [C, k] fp32) -- CUDA tensors, descending score, equal scores by ascending position.
        Collective under ZeRO-1 data parallelism, like predict."""
        cat, codes = self._encode_catalogue(reader, split, auxilliary_mask_type, aux_var_value)
        ex = None
        if exclude_seen:
            t = cat["seen"].tiles(codes.shape[0])
            ex = dict(ex_rp=cat["seen"].rp, ex_tptr=t["t_tptr"], ex_col=t["t_col"], ex_ntiles=t["t_ntiles"])
        items, scores = self.engine.topk_columns(codes, cat["n"], k, columns=columns, exclude=ex)
        return cat["keys"], items, scores

    def evaluate_ranking_columns(self, reader, split="valid", k=10, relevance_min=None, auxilliary_mask_type=None,
                                 aux_var_value=-1):
        """Hit rate, recall and NDCG at k per column (per user, for an item-row model), as the literature reports
        them: every column ranks the candidate rows it has not rated in the split's inputs, and its relevant rows
        are its held-out entries (valid / test targets) with a rating >= relevance_min (None: all of them).
        Returns metrics.ranking_from_rows of the per-column counts: {"hit_rate@k", "recall@k", "ndcg@k", "rows"},
        rows = the columns with a relevant row.  Collective under ZeRO-1 data parallelism, like predict."""
        if split not in ("valid", "test"):
            raise ValueError("evaluate_ranking_columns needs split='valid' or 'test' (the train split has no "
                             "held-out entries)")
        cat, codes = self._encode_catalogue(reader, split, auxilliary_mask_type, aux_var_value)
        rr = self._rank_columns(cat, codes, k, relevance_min)[2].cpu().numpy()
        return M.ranking_from_rows(rr[:, 0], rr[:, 1], rr[:, 2], k)

    def _rank_columns(self, cat, codes, k, relevance_min, columns=None):
        """Engine.topk_columns with the catalogue's seen rows excluded and its held-out entries as relevance"""
        seen, held = cat["seen"], cat["held"]
        t, h = seen.tiles(codes.shape[0]), held.tiles(codes.shape[0])
        ex = dict(ex_rp=seen.rp, ex_tptr=t["t_tptr"], ex_col=t["t_col"], ex_ntiles=t["t_ntiles"])
        rel = dict(rel_rp=held.rp, rel_col=h["t_col"], rel_val=h["t_val"], rel_min=relevance_min)
        return self.engine.topk_columns(codes, cat["n"], k, columns=columns, exclude=ex, relevance=rel)

    def fit(self, x, y, batch_size=None, epochs=1, verbose=1, callbacks=None, validation_split=0.0, shuffle=True,
            **kw):
        """Keras 2.0.4 Model.fit on dense arrays (train_jester.py:78-79): the last validation_split fraction
        held out (split_at = int(n (1 - validation_split))), np.random.shuffle of the training indices each
        epoch, ceil(n / batch_size) batches -- the last one partial --, epoch logs weighted by batch size
        (BaseLogger) and the validation logs by sample over every held-out row (_test_loop).  With a Dropout
        layer the reference fixes noise_shape = [batch_size, H] (model.py:73), so a partial batch cannot run
        there: with dropout only full TRAINING batches are taken.  Evaluation runs the layer through
        in_train_phase (its noise never applies at test time), so the validation logs always cover every
        held-out row, the trailing partial batch included."""
        e = self.engine
        bs = int(batch_size or e.B)
        if bs != e.B:
            raise ValueError("batch_size must equal the model batch_size (Dropout noise_shape, model.py:73)")
        partial = e.keep >= 1.0
        # the arrays go to the device once, plus one all-zero row that pads a partial batch (its input, output
        # mask and target are zero, so it adds nothing to the loss, the statistics or any gradient; the
        # gradient scale uses the real row count); every batch is then gathered there by row index (no per-step
        # host copies, no synchronisation between steps)
        dev = e.dev

        def on_dev(a):
            t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))
            out = torch.zeros(t.shape[0] + 1, t.shape[1], device=dev, dtype=torch.float32)
            out[:-1] = t.to(dev, torch.float32)
            return out
        xd = [on_dev(a) for a in x]
        yd = on_dev(y)
        n = xd[0].shape[0] - 1
        split_at = int(n * (1.0 - validation_split)) if validation_split else n
        hist = History()
        callbacks = callbacks or []

        def batches(m, allow_partial):
            full, rest = divmod(m, bs)
            return [(s * bs, bs) for s in range(full)] + ([(full * bs, rest)] if rest and allow_partial else [])

        def rows_of(ix, b):
            if b == bs:
                return ix
            return torch.cat([ix, torch.full((bs - b,), n, dtype=torch.int64, device=dev)])
        val_rows = torch.arange(split_at, n, dtype=torch.int64, device=dev)
        for epoch in range(epochs):
            idx = np.arange(split_at)
            if shuffle:
                np.random.shuffle(idx)
            idx_d = torch.as_tensor(idx, dtype=torch.int64).to(dev)
            tb = batches(split_at, partial)
            for s0, b in tb:
                self._load_rows(xd, yd, rows_of(idx_d[s0:s0 + b], b), b)
                e.train_step()
            logs = self._logs_from_stats(self._take_stats(), [b for _, b in tb])
            vb = batches(n - split_at, True)
            if vb:
                for s0, b in vb:
                    self._load_rows(xd, yd, rows_of(val_rows[s0:s0 + b], b), b)
                    e.eval_step()
                vl = self._logs_from_stats(self._take_stats(), [b for _, b in vb])
                for k, v in vl.items():
                    logs["val_" + k] = v
            for k, v in logs.items():
                hist.history.setdefault(k, []).append(v)
            hist.epoch.append(epoch)
            for cb in callbacks:
                cb.on_epoch_end(logs)
                self.stop_training |= getattr(cb, "stop", False)
            if self.stop_training:
                break
        return hist

    def _load_rows(self, xd, yd, rows, real=None):
        """batch = rows `rows` of the device-resident arrays of Model.fit (the first `real` of them real)"""
        blocks, out_mask = self._split_inputs(xd)
        self.engine.load_dense(blocks, out_mask, yd, rows=rows, rows_real=real)

    # ------------------------------------------------------------------ weights / checkpoints
    def get_weights(self):
        """Keras-layout weights.  Collective under data parallelism with ZeRO-1 (the sharded fp32 masters
        are all-gathered first): call it on every rank, as predict and save."""
        return self.engine.get_weights()

    def set_weights(self, weights):
        self.engine.set_weights(weights)

    def shard_path(self, path):
        """feature parallelism: every rank checkpoints its own column shard"""
        if self.fp is None:
            return path
        return "%s.shard%dof%d" % (path, self.fp[0], self.fp[1])

    def save(self, path):
        """Weights (Keras layout) + optimizer state in a safetensors file (replaces the h5 of train.py:169).
        Collective under data parallelism (the sharded optimizer slots are gathered first; rank 0 writes)
        and under feature parallelism (every rank writes its shard, Model.shard_path)."""
        from safetensors.numpy import save_file
        e = self.engine
        if self.dp is not None:
            self.dp.gather_slots()
            if e.master_sync is not None:       # ZeRO-1 masters: a collective, so on every rank
                e.master_sync()
            if self.rank != 0:
                return
        path = self.shard_path(path)
        tensors = {}
        for i, w in enumerate(e.get_weights()):
            tensors["param/%d" % i] = np.ascontiguousarray(w)
        if self.optimizer is not None and e.slots:
            for i, (sw, sb) in enumerate(e.slots):
                for j, t in enumerate(sw):
                    if t is not None:
                        tensors["opt/W%d/%d" % (i, j)] = t.cpu().numpy()
                for j, t in enumerate(sb):
                    if t is not None:
                        tensors["opt/b%d/%d" % (i, j)] = t.cpu().numpy()
            tensors["opt/iterations"] = np.array([self.optimizer.iterations], np.int64)
            # whose slots these are: the two-slot kinds give them different meanings (Adam's v, Adadelta's d,
            # Adamax's u), so a load into another optimizer must not reinterpret them
            tensors["opt/name"] = np.frombuffer(self.optimizer.name.encode("ascii"), np.uint8).copy()
        # the objective, with the optimizer state: a resumed run must not silently switch it
        tensors["loss/name"] = np.frombuffer(self.loss.name.encode("ascii"), np.uint8).copy()
        tensors["loss/param"] = np.array([self.loss.param], np.float64)
        save_file(tensors, path)

    def load(self, path, with_optimizer=True):
        from safetensors.numpy import load_file
        t = load_file(self.shard_path(path))
        opt_state = with_optimizer and self.optimizer is not None and "opt/iterations" in t
        # whose slots the file holds, before anything of the model changes: a refused load leaves it as it was
        if opt_state and "opt/name" in t:     # (a file from before the field: loads as it always did)
            name = bytes(bytearray(t["opt/name"].astype(np.uint8))).decode("ascii")
            if name != self.optimizer.name:
                raise ValueError("%s holds the optimizer state of %r, this model is compiled with %r: load it "
                                 "with with_optimizer=False or compile the model with %r"
                                 % (path, name, self.optimizer.name, name))
        n = len([k for k in t if k.startswith("param/")])
        self.set_weights([t["param/%d" % i] for i in range(n)])
        e = self.engine
        if with_optimizer:
            # the objective saved with the optimizer state (a file from before the losses: the squared loss)
            saved = self.saved_loss(t)
            e.set_loss(saved)
            self.loss = saved
        if opt_state:
            for i, (sw, sb) in enumerate(e.slots):
                for j, s in enumerate(sw):
                    if s is not None:
                        s.copy_(torch.as_tensor(t["opt/W%d/%d" % (i, j)]))
                for j, s in enumerate(sb):
                    if s is not None:
                        s.copy_(torch.as_tensor(t["opt/b%d/%d" % (i, j)]))
            self.optimizer.iterations = int(t["opt/iterations"][0])


    @staticmethod
    def saved_loss(tensors):
        """the losses.Loss a Model.save file holds (its load_file dict); files without one mean MSE"""
        if "loss/name" not in tensors:
            return losses.MeanSquaredError()
        name = bytes(bytearray(tensors["loss/name"].astype(np.uint8))).decode("ascii")
        param = float(tensors["loss/param"][0])
        return losses.get(name, {"delta": param} if name == losses.Huber.name else None)


class _Donor(object):
    """weights of a saved model (Model.save safetensors) in the Keras order, for the transfer helpers"""

    def __init__(self, weights):
        self.weights = weights

    def get_weights(self):
        return self.weights


def load_donor(path):
    """the donor model of train.py:136-145 (keras.models.load_model there; a Model.save file here)"""
    from safetensors.numpy import load_file
    t = load_file(path)
    return _Donor([t["param/%d" % i] for i in range(len([k for k in t if k.startswith("param/")]))])


class omni_model(object):
    """model.py:34-35 signature; extra keyword ``compute_dtype`` ('float32' = exact-fp32 MFMA, the
    parity mode; 'float16' / 'bfloat16' MFMA with fp32 accumulation) and ``seed``."""

    def __init__(self, numlayers, num_hidden_units, input_shape, batch_size, dense_activation="tanh",
                 use_causal_info=True, use_timestamps=False, use_both_masks=False, l2_weight_regulatization=None,
                 sparse_representation=False, dropout_probability=None, use_sparse_masking_layer=False,
                 compute_dtype="float32", seed=None, device=None, rating_range=1.0, shard=None, comm=None):
        if use_timestamps:
            raise NotImplementedError("use_timestamps: broken in the reference; not supported")
        if sparse_representation:
            raise NotImplementedError("sparse_representation: needs a patched Keras in the reference; dense only")
        if use_sparse_masking_layer:
            raise NotImplementedError("Dynamic_Masking_Layer is broken in the reference (model.py:186)")
        self.numlayers = numlayers
        self.num_hidden_units = num_hidden_units
        self.input_shape = input_shape
        self.batch_size = batch_size
        k = 1 + int(bool(use_causal_info)) + int(bool(use_both_masks))
        self.engine = Engine(input_shape, [num_hidden_units] * numlayers, batch_size, k_blocks=k,
                             activation=dense_activation, dropout=dropout_probability, l2=l2_weight_regulatization,
                             compute_dtype=compute_dtype, device=device, seed=seed, shard=shard, comm=comm)
        self.model = Model(self.engine, bool(use_causal_info), bool(use_both_masks), rating_range)

    def save_weights(self, filename):
        self.model.save(filename)

    def load_weights(self, weights):
        self.model.set_weights(weights)

    # ---- transfer / denoising-autoencoder helpers (model.py:107-170) ------------------------
    # Every dense layer of the omni model has an input or output width equal to the hidden width, so
    # the reference's layer filter selects all of them, in order: hidden layers, then the output
    # layer.  ``trainable`` takes effect immediately (Keras needs a recompile, model.py:135).
    @staticmethod
    def _dense_weights(donor):
        eng = donor.engine if hasattr(donor, "engine") else donor
        w = eng.get_weights()
        return [[w[2 * i], w[2 * i + 1]] for i in range(len(w) // 2)]

    def _set_layer(self, i, wb):
        w = self.model.get_weights()
        w[2 * i], w[2 * i + 1] = wb
        self.model.set_weights(w)

    def replace_dense_layer_weights(self, donor_model, layers_to_replace, make_layers_trainable=False):
        """model.py:107-125: copy the selected dense layers from the donor; set their trainable flag."""
        donor = self._dense_weights(donor_model)
        if layers_to_replace == "all":
            layers_to_replace = [True] * len(donor)
        for i in range(len(self.engine.W)):
            if i < len(layers_to_replace) and layers_to_replace[i]:
                self._set_layer(i, donor[i])
                self.engine.trainable[i] = bool(make_layers_trainable)
                print("Loaded weights for dense layer ", i)

    def manually_load_all_weights(self, donor_model):
        """model.py:127-132: every layer's weights from the donor (same architecture)."""
        eng = donor_model.engine if hasattr(donor_model, "engine") else donor_model
        self.model.set_weights(eng.get_weights())

    def make_trainable(self):
        """model.py:134-138: layers whose OUTPUT width is the hidden width become trainable (the
        output layer keeps its flag -- the reference's filter)."""
        for i in range(len(self.engine.W) - 1):
            self.engine.trainable[i] = True

    def load_and_fix_for_denoising_autoencoders(self, donor_model):
        """model.py:140-170: the outer floor(D/2) donor layers on each side are copied into this
        model's first / last layers and frozen; the middle layers stay trainable."""
        donor = self._dense_weights(donor_model)
        print("Number of weight layers to donate", len(donor))
        k = len(donor) // 2
        n_new = len(self.engine.W)
        for i in range(n_new):
            if i < k:
                self._set_layer(i, donor[i])
                self.engine.trainable[i] = False
                print("Loaded and fixed weights for dense layer ", i, " from donor dense layer ", i)
            elif i >= n_new - k:
                src = len(donor) - (n_new - i)
                self._set_layer(i, donor[src])
                self.engine.trainable[i] = False
                print("Loaded and fixed weights for dense layer ", i, " from donor dense layer ", src)
