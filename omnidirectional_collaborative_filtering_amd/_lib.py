"""ctypes binding of libocf.so (the C ABI declared in include/ocf.h).

The product path has no CPU fallback: if the shared library is missing or fails to load, every
entry point raises.  Build it with ``python -m omnidirectional_collaborative_filtering_amd.build``
(or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCF_LIB_PATH") or os.path.join(_HERE, "libocf.so")   # override: variant builds

DT_F32, DT_F16, DT_BF16 = 0, 1, 2
ACT = {"linear": 0, None: 0, "sigmoid": 1, "tanh": 2, "relu": 3}
OPT_SGD, OPT_ADAGRAD, OPT_RMSPROP, OPT_ADAM, OPT_ADADELTA, OPT_ADAMAX = 0, 1, 2, 3, 4, 5
LIVE_REC = 144                 # ocf.h OCF_LIVE_REC
EPI_SLAB, EPI_BIAS_ACT, EPI_GRAD_ACT, EPI_GRAD, EPI_OPTIM, EPI_PREDICT, EPI_MASKED_MSE = range(7)
LOSS_MSE, LOSS_MAE, LOSS_HUBER, LOSS_LOGCOSH = range(4)     # ocf.h OCF_LOSS_*

P = ctypes.c_void_p
I32 = ctypes.c_int
I64 = ctypes.c_int64
U64 = ctypes.c_uint64
F32 = ctypes.c_float


class OcfOptParams(ctypes.Structure):
    _fields_ = [("kind", I32), ("lr", F32), ("eps", F32), ("rho", F32), ("beta2", F32), ("l2", F32),
                ("gscale", F32)]


class OcfScatterArgs(ctypes.Structure):
    _fields_ = [
        ("rp1", P), ("col1", P), ("val1", P), ("dup1", P), ("rows1", P), ("keep1", P), ("boff1", P),
        ("s0", F32), ("s1", F32), ("seed", U64), ("stream", U64), ("mode", I32), ("pass_through", I32),
        ("rp2", P), ("col2", P), ("val2", P), ("dup2", P), ("rows2", P),
        ("B", I32), ("B_pad", I32), ("N", I32), ("aux", F32),
        ("X", P), ("Min", P), ("Mout", P), ("T", P), ("Mmiss", P), ("ld", I64),
        ("xin", P), ("xin_dtype", I32), ("xin_ld", I64), ("xin_block", I64), ("feed", I32), ("both", I32),
        ("tile_cnt", P), ("bk_ptr", P), ("bk_cur", P), ("bk_rc", P), ("bk_t", P), ("bk_m", P), ("n_tiles", I32),
        ("pos1", P),
        ("lboff1", P), ("lboff2", P), ("E1", I64), ("E2", I64), ("tflag1", P), ("tflag2", P),
        ("xin_clean", I32), ("xval1", P), ("tb_cnt", P), ("tb_nk", I32),
        ("rtag_in", P), ("rtag_out", P), ("rtag", I32), ("col_cnt", P), ("ecb", P),
    ]


class OcfRowListArgs(ctypes.Structure):
    _fields_ = [
        ("ecb", P), ("E", I64), ("col_cnt", P), ("cursor", P), ("n_cols", I32), ("row_ptr", P), ("row_ent", P),
        ("rtag_in", P), ("rtag_out", P), ("rtag", I32), ("live_in", P), ("live_out", P),
    ]


class OcfEpochScatterArgs(ctypes.Structure):
    _fields_ = [
        ("n_sel", I32), ("sel", P), ("ebase", P), ("max_e", I64), ("keep_off", P), ("stream_mul", U64),
        ("xval", P), ("tflag", P), ("ebase0", I64),
    ]


class OcfEpochRowListArgs(ctypes.Structure):
    _fields_ = [
        ("n_sel", I32), ("B", I32), ("n_cols", I32), ("rows", P), ("rp", P), ("col", P), ("lboff", P),
        ("sel", P), ("ebase", P), ("cnt", P), ("row_ptr", P), ("row_ent", P), ("live", P), ("n_rg", I32),
        ("ebase0", I64), ("max_list", I32), ("entries", I64),
    ]


class OcfEncTileArgs(ctypes.Structure):
    _fields_ = [
        ("rows", P), ("rp", P), ("tptr", P), ("tcol", P), ("tlidx", P), ("lboff", P), ("xval", P),
        ("W", P), ("ldw", I64), ("w_dtype", I32), ("B", I32), ("Bp", I32), ("n_tiles", I32), ("H", I32),
        ("splits", I32), ("part", P), ("nnz", I64), ("n_entries", I64), ("work", P), ("work_bytes", I64),
        ("max_row_len", I64),
    ]


class OcfGatherArgs(ctypes.Structure):
    _fields_ = [
        ("rows", P), ("rp", P), ("col", P), ("val", P), ("lboff", P), ("xval", P), ("flag", P),
        ("ch_row", P), ("ch_j0", P), ("ch_j1", P), ("n_chunks", I32),
        ("W", P), ("w_dtype", I32), ("ldw", I64), ("w_blocked", I32), ("H", I32), ("part", P),
        ("h", P), ("h_dtype", I32), ("bias", P), ("aux", F32), ("delta_e", P), ("chunk_stats", P),
        ("d_out", P), ("d_dtype", I32), ("ld_d", I64),
        ("enc_part", P), ("enc_cptr", P), ("bias_h", P), ("act", I32), ("keep", F32), ("seed", U64), ("stream", U64),
        ("a_out", P), ("mask_out", P), ("m_real", I32), ("n_real", I32), ("zero_word", P),
        ("jr", P), ("row_arrive", P),
        ("loss", I32), ("loss_param", F32),
    ]


REDUCE_RAW, REDUCE_BIAS_ACT, REDUCE_GRAD_ACT = 0, 1, 2


class OcfRowsReduceArgs(ctypes.Structure):
    _fields_ = [
        ("part", P), ("row_cptr", P), ("B", I32), ("Bp", I32), ("H", I32), ("mode", I32), ("out", P),
        ("bias", P), ("act", I32), ("keep", F32), ("seed", U64), ("stream", U64),
        ("mask_in", P), ("mask_out", P), ("a_out", P), ("a_in", P), ("h_out", P), ("h_dtype", I32), ("n_real", I32),
        ("db_part", P), ("gscale", F32), ("chunk_stats", P), ("stats_part", P), ("row_sse", P),
        ("stats4", I32),
    ]


class OcfGemmArgs(ctypes.Structure):
    _fields_ = [
        ("compute_dtype", I32),
        ("A", P), ("a_dtype", I32), ("a_col", I32), ("lda", I64),
        ("B", P), ("b_dtype", I32), ("b_col", I32), ("ldb", I64),
        ("M", I32), ("N", I32), ("K", I32), ("splits", I32), ("order", I32), ("epi", I32),
        ("out", P), ("ld_out", I64), ("split_stride", I64),
        ("bias", P), ("act", I32), ("keep", F32), ("seed", U64), ("stream", U64),
        ("mask_in", P), ("mask_out", P), ("a_out", P), ("h_out", P), ("h_dtype", I32), ("a_in", P),
        ("db_part", P), ("ld_db", I64), ("m_real", I32), ("n_real", I32),
        ("p", P), ("s1", P), ("s2", P), ("opt", OcfOptParams),
        ("pmask", P), ("ld_pmask", I64),
        ("bk_ptr", P), ("bk_rc", P), ("bk_t", P), ("bk_m", P), ("stats_part", P), ("row_sse_part", P),
        ("t_rows", P), ("t_rp", P), ("t_tptr", P), ("t_col", P), ("t_val", P), ("t_lidx", P), ("t_flag", P),
        ("t_lboff", P), ("t_ntiles", I32), ("t_aux", F32),
        ("p_shadow", P), ("a_nt", I32), ("b_nt", I32), ("b_blocked", I32), ("shadow_blocked", I32),
        ("a_sparse", I32), ("sp_rows", P), ("sp_rp", P), ("sp_tptr", P), ("sp_col", P), ("sp_lidx", P),
        ("sp_lboff", P), ("sp_vals", P), ("sp_ntiles", I32), ("sp_krows", I32), ("sp_colsum", P),
        ("sp_bptr", P), ("sp_ent", P),
        ("cb_p", P), ("cb_s1", P), ("cb_s2", P), ("cb_op", OcfOptParams),
        ("jb_part", P), ("jb_parts", I32), ("jb_n", I32), ("jb_ld", I64), ("jb_p", P), ("jb_s1", P), ("jb_s2", P),
        ("jb_op", OcfOptParams),
        ("js_sp", P), ("js_rs", P), ("js_out", P), ("js_nparts", I32), ("js_ntiles", I32), ("js_M", I32),
        ("row_live", P), ("sp_rowptr", P), ("sp_rowent", P), ("jr", P), ("sp_nent", I64),
        ("dn_t", P), ("dn_m", P), ("ld_dn", I64), ("dn_rows", P),
        ("loss", I32), ("loss_param", F32),
    ]


TOPK_MAX_K = 128               # ocf.h OCF_TOPK_MAX_K


class OcfTopkArgs(ctypes.Structure):
    """ocf.h OcfTopkArgs: the k best decoder scores per batch row (ocf_topk)"""
    _fields_ = [
        ("compute_dtype", I32), ("h", P), ("ldh", I64), ("W", P), ("w_dtype", I32), ("ldw", I64), ("w_blocked", I32),
        ("bias", P), ("M", I32), ("N", I32), ("K", I32), ("m_real", I32), ("n_real", I32), ("k", I32), ("groups", I32),
        ("ex_rows", P), ("ex_rp", P), ("ex_tptr", P), ("ex_col", P), ("ex_ntiles", I32),
        ("ex_mask", P), ("ld_ex", I64), ("ex_mrows", P),
        ("out_idx", P), ("out_val", P), ("ld_out", I64), ("work", P), ("work_bytes", I64),
        ("rel_rows", P), ("rel_rp", P), ("rel_col", P), ("rel_val", P), ("rel_min", F32), ("row_rank", P),
        ("bias_by_row", I32), ("h_dtype1", I32), ("h_blocked", I32),      # the transposed call (0 = as before)
    ]


class OcfPredictArgs(ctypes.Structure):
    """ocf.h OcfPredictArgs: the decoder's prediction at listed entries (ocf_predict_entries)"""
    _fields_ = [
        ("rows", P), ("rp", P), ("col", P), ("val", P), ("lboff", P), ("flag", P),
        ("ch_row", P), ("ch_j0", P), ("ch_j1", P), ("n_chunks", I32), ("B", I32), ("Bp", I32),
        ("h", P), ("h_dtype", I32), ("ldh", I64), ("H", I32),
        ("W", P), ("w_dtype", I32), ("ldw", I64), ("w_blocked", I32),
        ("bias", P), ("aux", F32), ("clip", I32), ("clip_lo", F32), ("clip_hi", F32),
        ("y", P), ("chunk_stats", P), ("row_stats", P), ("total", P),
    ]


class OcfPairSync(ctypes.Structure):
    """ocf.h OcfPairSync: ocf_gemm_pair's hand-off counter (device word + its host-side running count)"""
    _fields_ = [("word", P), ("count", U64)]


ASYNC_PAIR_WAIT = 1            # ocf.h OCF_ASYNC_PAIR_WAIT


class OcfRowStepArgs(ctypes.Structure):
    _fields_ = [("enc", OcfGatherArgs), ("dec", OcfGatherArgs), ("dw_out", OcfGemmArgs), ("dw_in", OcfGemmArgs),
                ("jr", OcfRowsReduceArgs), ("jr_on", I32), ("ev", P * 8), ("pair_sync", P), ("enc_arrive", P)]


class OcfBiasActArgs(ctypes.Structure):
    """ocf.h: ocf_splitk_bias_act's arguments as a block (without the stream)"""
    _fields_ = [("slabs", P), ("splits", I32), ("split_stride", I64), ("M", I32), ("N", I32), ("ld", I64),
                ("bias", P), ("act", I32), ("keep", F32), ("seed", U64), ("stream", U64), ("mask_in", P),
                ("mask_out", P), ("a_out", P), ("h_out", P), ("h_dtype", I32), ("m_real", I32), ("n_real", I32)]


class OcfGradActArgs(ctypes.Structure):
    """ocf.h: ocf_splitk_grad_act's arguments as a block"""
    _fields_ = [("slabs", P), ("splits", I32), ("split_stride", I64), ("M", I32), ("N", I32), ("ld", I64),
                ("a_in", P), ("mask", P), ("keep", F32), ("act", I32), ("d_out", P), ("d_dtype", I32), ("db", P),
                ("gscale", F32), ("m_real", I32), ("n_real", I32)]


class OcfStatsArgs(ctypes.Structure):
    """ocf.h: ocf_stats_finalize's arguments as a block"""
    _fields_ = [("stats_part", P), ("n_parts", I32), ("row_sse_part", P), ("n_tiles", I32), ("M", I32), ("out", P)]


class OcfBiasOptArgs(ctypes.Structure):
    """ocf.h: ocf_bias_opt_from_partials' arguments as a block (opt by value)"""
    _fields_ = [("b", P), ("db_part", P), ("parts", I32), ("ld", I64), ("n", I32), ("s1", P), ("s2", P),
                ("g_out", P), ("opt", OcfOptParams)]


class OcfRankStepArgs(ctypes.Structure):
    _fields_ = [("enc", OcfGatherArgs), ("enc_sum", OcfRowsReduceArgs), ("hidden", OcfBiasActArgs),
                ("dec", OcfGatherArgs), ("dec_sum", OcfRowsReduceArgs), ("stats", OcfStatsArgs),
                ("dw_out", OcfGemmArgs), ("out_bias", OcfBiasOptArgs), ("hidden_grad", OcfGradActArgs),
                ("dw_in", OcfGemmArgs), ("side", P), ("fork", P * 2), ("join", P), ("ev", P * 8)]


class OcfMlpStepArgs(ctypes.Structure):
    """ocf.h OcfMlpStepArgs: a small dense model's whole step in one launch (ocf_mlp_step)"""
    _L = 8 + 1
    _fields_ = [("n_hidden", I32), ("B", I32), ("Bp", I32), ("N", I32), ("Np", I32), ("k_blocks", I32),
                ("hidden", I32 * 8), ("hidden_p", I32 * 8), ("x", P * 3), ("ld_x", I64), ("rows", P),
                ("out_mask", P), ("targets", P), ("ld_t", I64), ("W", P * _L), ("b", P * _L), ("sW1", P * _L),
                ("sW2", P * _L), ("sb1", P * _L), ("sb2", P * _L), ("shadow", P * _L), ("shadow_blocked", I32),
                ("act", I32), ("compute_dtype", I32), ("opt", OcfOptParams), ("stats", P), ("work", P),
                ("work_bytes", I64), ("barrier", P), ("wgs", I32), ("trace", P), ("keep", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint64), ("mask", P * 8),
                ("loss", I32), ("loss_param", ctypes.c_float)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if "keep" not in kw:
            self.keep = 1.0


ASYNC_MLP_BARRIER = 2          # ocf.h OCF_ASYNC_MLP_BARRIER


class OcfTileBucketArgs(ctypes.Structure):
    _fields_ = [
        ("rows", P), ("rp", P), ("tptr", P), ("col", P), ("lidx", P), ("lboff", P),
        ("krows", I32), ("ntiles", I32), ("gm", I32), ("nk", I32),
        ("cnt", P), ("bptr", P), ("ent", P), ("cap", I64), ("counted", I32), ("cnt_clear", P),
        ("rtag_in", P), ("rtag_out", P), ("rtag", I32), ("live_in", P), ("live_out", P),
        ("row_ptr", P), ("row_ent", P),
    ]


class OcfOptStepArgs(ctypes.Structure):
    _fields_ = [("p", P), ("g", P), ("g_dtype", I32), ("s1", P), ("s2", P), ("n", I64), ("opt", OcfOptParams),
                ("shadow", P), ("shadow_dtype", I32)]


class OcfRecipKeepArgs(ctypes.Structure):
    _fields_ = [
        ("key", ctypes.c_uint32 * 624), ("pos", ctypes.c_int32), ("nb", ctypes.c_int32), ("B", ctypes.c_int32),
        ("n_entries", I64), ("boff", P), ("ebase", P), ("s0", ctypes.c_double), ("s1", ctypes.c_double),
        ("keep", P), ("doubles", P), ("workspace", P), ("workspace_bytes", I64),
    ]


MAX_HIDDEN = 8                 # ocf.h OCF_MAX_HIDDEN


class OcfModelDesc(ctypes.Structure):
    _fields_ = [
        ("n_hidden", I32), ("N", I32), ("k_blocks", I32), ("hidden", I32 * MAX_HIDDEN), ("act", I32),
        ("dropout", F32), ("compute_dtype", I32), ("max_batch", I32), ("seed", U64),
        ("W", P * (MAX_HIDDEN + 1)), ("b", P * (MAX_HIDDEN + 1)),
    ]


# every symbol include/ocf.h declares, with its ctypes signature
SIGNATURES = {
    "ocf_scatter_batch": (I32, [ctypes.POINTER(OcfScatterArgs), P]),
    "ocf_dense_targets": (I32, [P, P, I64, I32, I32, I32, P, P, P, P, P, P, P, P]),
    "ocf_pack_input": (I32, [P, P, P, I64, I32, I32, P, I32, I64, I64, I32, P, P]),
    "ocf_gemm": (I32, [ctypes.POINTER(OcfGemmArgs), P]),
    "ocf_topk": (I32, [ctypes.POINTER(OcfTopkArgs), P]),
    "ocf_topk_workspace": (I64, [ctypes.POINTER(OcfTopkArgs)]),
    "ocf_predict_entries": (I32, [ctypes.POINTER(OcfPredictArgs), P]),
    "ocf_gemm_pair": (I32, [ctypes.POINTER(OcfGemmArgs), ctypes.POINTER(OcfGemmArgs), P, P]),   # P: OcfPairSync*
    "ocf_train_step_rows": (I32, [ctypes.POINTER(OcfRowStepArgs), P]),
    "ocf_rank_step": (I32, [ctypes.POINTER(OcfRankStepArgs), I32, P]),
    "ocf_mlp_step_workspace": (I64, [ctypes.POINTER(OcfMlpStepArgs)]),
    "ocf_mlp_step": (I32, [ctypes.POINTER(OcfMlpStepArgs), P]),
    "ocf_splitk_bias_act": (I32, [P, I32, I64, I32, I32, I64, P, I32, F32, U64, U64, P, P, P, P, I32, I32, I32, P]),
    "ocf_splitk_grad_act": (I32, [P, I32, I64, I32, I32, I64, P, P, F32, I32, P, I32, P, F32, I32, I32, P]),
    "ocf_opt_step": (I32, [P, P, P, P, I64, ctypes.POINTER(OcfOptParams), P]),
    "ocf_opt_step_ex": (I32, [ctypes.POINTER(OcfOptStepArgs), P]),
    "ocf_bias_opt_from_partials": (I32, [P, P, I32, I64, I32, P, P, P, ctypes.POINTER(OcfOptParams), P]),
    "ocf_stats_finalize": (I32, [P, I32, P, I32, I32, P, P]),
    "ocf_loss_sum": (I32, [P, I32, P, P]),
    "ocf_sumsq": (I32, [P, I64, F32, P, P, P]),
    "ocf_gather_encoder": (I32, [ctypes.POINTER(OcfGatherArgs), P]),
    "ocf_gather_decoder": (I32, [ctypes.POINTER(OcfGatherArgs), P]),
    "ocf_gather_encdec": (I32, [ctypes.POINTER(OcfGatherArgs), ctypes.POINTER(OcfGatherArgs), P, P]),
    "ocf_rows_reduce": (I32, [ctypes.POINTER(OcfRowsReduceArgs), P]),
    "ocf_colsum": (I32, [P, I32, I64, I32, I32, F32, P, P]),
    "ocf_sparse_tiles": (I32, [ctypes.POINTER(OcfTileBucketArgs), P]),
    "ocf_row_lists": (I32, [ctypes.POINTER(OcfRowListArgs), P]),
    "ocf_epoch_row_lists": (I32, [ctypes.POINTER(OcfEpochRowListArgs), P]),
    "ocf_epoch_scatter": (I32, [ctypes.POINTER(OcfScatterArgs), ctypes.POINTER(OcfEpochScatterArgs), P]),
    "ocf_recip_keep_workspace": (I64, [I32, I32, I64, I32]),
    "ocf_recip_keep": (I32, [ctypes.POINTER(OcfRecipKeepArgs), P]),
    "ocf_mt_host_random_sample": (I32, [P, P, I64, P]),
    "ocf_mt_host_jump": (I32, [P, I64, P]),
    "ocf_model_dims": (I32, [ctypes.POINTER(OcfModelDesc), P, P]),
    "ocf_ctx_create": (I32, [ctypes.POINTER(OcfModelDesc), ctypes.POINTER(P)]),
    "ocf_ctx_destroy": (I32, [P]),
    "ocf_forward": (I32, [P, P, I64, I32, I32, U64, P, I64, P, I64, P, P]),
    "ocf_masked_mse": (I32, [P, P, P, I64, I32, I32, P, I64, P, P]),
    "ocf_masked_loss": (I32, [I32, F32, P, P, P, I64, I32, I32, P, I64, P, P]),
    "ocf_backward": (I32, [P, P, I64, I32, F32, P, P, P]),
    "ocf_set_tuning": (I32, [ctypes.c_char_p, I32, ctypes.POINTER(I32)]),
    "ocf_check_async": (I32, []),
    "ocf_encoder_tiles": (I32, [ctypes.POINTER(OcfEncTileArgs), P]),
    "ocf_encoder_tiles_workspace": (I64, [ctypes.POINTER(OcfEncTileArgs)]),
    "ocf_timing_event_create": (I32, [ctypes.POINTER(P)]),
    "ocf_event_record": (I32, [P, P]),
    "ocf_event_elapsed_ms": (I32, [P, P, ctypes.POINTER(F32)]),
    "ocf_event_destroy": (I32, [P]),
    "ocf_version": (I32, []),
    "ocf_last_error": (ctypes.c_char_p, []),
}

_lib = None


class OcfError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load libocf.so (raises if absent -- there is deliberately no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OcfError("libocf.so not built at %s (run omnidirectional_collaborative_filtering_amd.build)" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# called (no arguments) when a library call reports OCF_ASYNC_ENC_WAIT: engines register a reset of their
# encoder -> decoder hand-off counters (an encoder chunk that arrived after its row's decoder gave up leaves a
# count behind; ocf.h ocf_gather_encdec)
enc_wait_hooks = []


class TimingEvent:
    """A HIP event for timing only (ocf_timing_event_create: hipEventDisableSystemFence -- a record costs no
    system-scope cache write-back / invalidate); the torch.cuda.Event surface the engine's timers use
    (cuda_event, record, elapsed_time).  Read it after a device synchronisation."""
    __slots__ = ("cuda_event",)

    def __init__(self):
        p = P()
        call("ocf_timing_event_create", ctypes.byref(p))
        self.cuda_event = p.value

    def record(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        call("ocf_event_record", self.cuda_event, s.cuda_stream)

    def elapsed_time(self, end):
        ms = F32()
        call("ocf_event_elapsed_ms", self.cuda_event, end.cuda_event, ctypes.byref(ms))
        return ms.value

    def __del__(self):
        if _lib is not None and self.cuda_event:
            _lib.ocf_event_destroy(self.cuda_event)


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.ocf_last_error().decode()
        if "ocf_gather_encdec: a decoder chunk gave up" in msg:
            for hook in list(enc_wait_hooks):
                hook()
        raise OcfError("%s failed: %s" % (name, msg))
    return rc
