"""ctypes binding of libpdmk.so (include/pdmk.h) — the only route from the Python host side to the HIP kernels.

There is NO fallback: if the shared library is missing or a call returns a non-zero status this module raises.
torch is used for device memory and streams only (tensors are passed as raw device pointers).
"""
import ctypes as C
import os
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDMK_LIB: another build of the same library (same-box A/B of kernel variants, tools/); never a fallback - it must exist
LIB_PATH = os.environ.get("PDMK_LIB") or os.path.join(os.path.dirname(_HERE), "libpdmk.so")

F32, BF16 = 0, 1
EPI_NONE, EPI_GEGLU, EPI_GEGLU_BWD = 0, 1, 2
A_ROWK, A_CONV, A_COLK = 0, 1, 2
B_ROWK, B_COLK, B_COLK_CONV = 0, 1, 2


class PdmkError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise PdmkError(f"libpdmk.so not found at {LIB_PATH}: build it with `python __graft_entry__.py` "
                        f"(or `make -C unlearn-ft_amd/csrc`); there is no CPU/PyTorch fallback for the hot path")
    return C.CDLL(LIB_PATH)


_lib = _load()

vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double


class GemmArgs(C.Structure):
    _fields_ = [("A", vp), ("B", vp), ("C", vp), ("bias", vp), ("rowvec", vp), ("R", vp), ("colsum_out", vp),
                ("M", i32), ("N", i32), ("K", i32),
                ("lda", i32), ("ldb", i32), ("ldc", i32), ("ldr", i32),
                ("rows_per_b", i32), ("a_mode", i32), ("b_mode", i32),
                ("conv_b", i32), ("conv_hi", i32), ("conv_wi", i32), ("conv_ci", i32), ("conv_ho", i32),
                ("conv_wo", i32), ("conv_mode", i32), ("conv_ld", i32),
                ("dtype", i32), ("out_f32", i32), ("accumulate", i32), ("splitk", i32), ("alpha", f32), ("ldrv", i32),
                ("epilogue", i32), ("ldc2", i32), ("C2", vp), ("colstat", vp), ("cs_ld", i32), ("cs_col0", i32),
                ("ln_gamma", vp), ("ln_beta", vp), ("ln_stats", vp), ("ln_out", vp), ("ld_ln_out", i32), ("ln_eps", f32)]


class PlmsRow(C.Structure):
    """pdmk_plms_row (include/pdmk.h): one step of the fused guidance + PLMS update."""
    _fields_ = [("t", i64), ("mode", i32), ("nterms", i32), ("wslot", i32), ("rslot", i32 * 3), ("coef", f32 * 4),
                ("v_x", f32), ("v_v", f32), ("eps_scale", f32), ("x_scale", f32), ("vpred", i32), ("pad_", i32)]


class DdimRow(C.Structure):
    """pdmk_ddim_row (include/pdmk.h): one step of the fused guidance + DDIM update."""
    _fields_ = [("t", i64), ("c_x", f32), ("c_m", f32), ("pad_", i64)]


class LmsRow(C.Structure):
    """pdmk_lms_row (include/pdmk.h): one step of the fused guidance + K-LMS update."""
    _fields_ = [("t", f32), ("nterms", i32), ("wslot", i32), ("rslot", i32 * 3), ("coef", f32 * 4), ("d_x", f32), ("d_m", f32),
                ("dmode", i32), ("in_div", f32), ("pad_", i32 * 2)]


class SldParams(C.Structure):
    """pdmk_sld_params (include/pdmk.h): Safe Latent Diffusion's scalars as the kernels take them.  Build it with
    sld_params(): the fp32 fields are rounded from doubles, one_minus_beta from the double 1 - mom_beta."""
    _fields_ = [("sld_guidance_scale", f32), ("threshold", f32), ("momentum_scale", f32), ("mom_beta", f32),
                ("one_minus_beta", f32), ("warmup_steps", i32)]

    def key(self):
        return (self.sld_guidance_scale, self.threshold, self.momentum_scale, self.mom_beta, self.one_minus_beta,
                self.warmup_steps)


_SIGS = {
    "pdmk_version": ([], i32),
    "pdmk_gemm": ([C.POINTER(GemmArgs), vp], i32),
    "pdmk_gemm_group": ([C.POINTER(GemmArgs), i32, vp, C.POINTER(i32)], i32),
    "pdmk_gemm_plan": ([C.POINTER(GemmArgs), vp, C.POINTER(i32)], i32),
    "pdmk_gemm_ln_supported": ([C.POINTER(GemmArgs)], i32),
    "pdmk_conv_up2_supported": ([i32, i32, i32, i32, i32, i32], i32),
    "pdmk_up2_pack_weights": ([vp, vp, vp, i32, i32, i32, vp], i32),
    "pdmk_up2_combine_wgrad": ([vp, vp, i32, i32, vp], i32),
    "pdmk_gemm_last_candidate": ([], i32),
    "pdmk_gemm_last_form": ([], i32),
    "pdmk_gemm_candidate_name": ([i32, i32, i32, C.c_char_p, i32], i32),
    "pdmk_splitk_finish": ([vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_splitk_finish_colstat": ([vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp], i32),
    "pdmk_groupnorm_fwd": ([vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, vp], i32),
    "pdmk_groupnorm_apply_colstat": ([vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, vp], i32),
    "pdmk_groupnorm_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, vp], i32),
    "pdmk_groupnorm_bwd_partial_dims": ([i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)], i32),
    "pdmk_layernorm_bwd_partial_dims": ([i32, i32, C.POINTER(i32), C.POINTER(i32)], i32),
    "pdmk_reduce_partials_group": ([vp, i32, vp], i32),
    "pdmk_splitk_finish_group": ([vp, i32, vp], i32),
    "pdmk_layernorm_fwd": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, vp], i32),
    "pdmk_layernorm_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, i32, i32, vp], i32),
    "pdmk_attn_fwd": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, i32, i64, i32, i64, i32, i64, i32, f32, i32, vp], i32),
    "pdmk_attn_bwd": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32,
                       i64, i32, i64, i32, i64, i32, i64, i32, i64, i32, i64, i32, i64, i32, f32, vp, i64, i32, vp], i32),
    "pdmk_geglu_fwd": ([vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_geglu_bwd": ([vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_quantize_e4m3": ([vp, vp, i64, i32, vp], i32),
    "pdmk_silu_fwd": ([vp, vp, i64, i32, vp], i32),
    "pdmk_silu_bwd": ([vp, vp, vp, i64, i32, vp], i32),
    "pdmk_copy2d": ([vp, vp, i64, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_cast_permute": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_colsum": ([vp, vp, i64, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_pool2x2_sum": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_timestep_embed": ([vp, vp, vp, i32, i32, i32, vp], i32),
    "pdmk_timestep_embed_f32": ([vp, vp, vp, i32, i32, i32, vp], i32),
    "pdmk_scale_div": ([vp, vp, f32, i64, vp], i32),
    "pdmk_add_noise_velocity": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_nchw_to_nhwc": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_nhwc_to_nchw": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_mse_fwd": ([vp, i32, vp, i32, vp, vp, i32, i32, i64, i32, i32, i32, f64, vp], i32),
    "pdmk_mse_bwd": ([vp, i32, vp, i32, vp, vp, i32, i64, i32, i32, i32, i32, f32, i32, vp], i32),
    "pdmk_mse_fwd_bwd": ([vp, i32, vp, i32, vp, vp, i32, vp, i32, i64, i32, i32, i32, i32, f64, f32, i32, vp], i32),
    "pdmk_axpby": ([vp, vp, f32, f32, i64, i32, vp], i32),
    "pdmk_adamw": ([vp, vp, vp, vp, i64, vp, f32, f32, f32, f32, vp, f32, i32, vp, vp], i32),
    "pdmk_adamw_segments": ([vp, vp, vp, vp, vp, i32, vp, f32, f32, f32, f32, vp, f32, i32, vp, vp], i32),
    "pdmk_esd_head": ([vp, vp, vp, vp, f32, vp, i32, vp, i64, i32, i32, i32, i32, f64, f32, i32, vp], i32),
    "pdmk_transpose_tiles": ([vp, vp, vp, i32, i32, vp], i32),
    "pdmk_sumsq": ([vp, i64, vp, i32, vp], i32),
    "pdmk_zero": ([vp, i64, vp], i32),
    "pdmk_skinny_gemm": ([vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_skinny_wgrad": ([vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_softmax_rows": ([vp, vp, i64, i32, i64, i64, i32, vp], i32),
    "pdmk_latent_sample": ([vp, i32, vp, vp, i32, i32, i32, f32, i32, vp], i32),
    "pdmk_embed_tokens": ([vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_attn_fwd_causal": ([vp, vp, vp, vp, vp, i32, i32, i32, i64, i32, i64, i32, i64, i32, i64, i32, f32, i32, vp], i32),
    "pdmk_gelu_fwd": ([vp, vp, i64, i32, vp], i32),
    "pdmk_image_prep": ([vp, i64, vp, vp, i32, i32, vp, vp], i32),
    "pdmk_image_prep_ex": ([vp, i64, vp, vp, i32, i32, i32, vp, vp, vp, vp], i32),
    "pdmk_patch_im2col": ([vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_vit_tokens": ([vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_quick_gelu_fwd": ([vp, vp, i64, i32, vp], i32),
    "pdmk_gather_rows": ([vp, i32, vp, i32, vp, i32, i32, i32, i32, vp], i32),
    "pdmk_clip_score_head": ([vp, i32, vp, i32, vp, vp, vp, i32, i32, vp], i32),
    "pdmk_cosine_pairs": ([vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp], i32),
    "pdmk_plms_step": ([vp, i32, f32, f32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_ddim_step": ([vp, i32, f32, f32, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_sld_guidance": ([vp, vp, vp, i32, i32, i32, f32, C.POINTER(SldParams), i32, vp], i32),
    "pdmk_sld_plms_step": ([vp, i32, f32, C.POINTER(SldParams), vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32,
                            vp], i32),
    "pdmk_sld_ddim_step": ([vp, i32, f32, C.POINTER(SldParams), vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_calg_workspace_elems": ([i32, i32, i32], i64),
    "pdmk_calg_dots": ([vp, i32, i32, i32, i32, i32, vp, i64, vp], i32),
    "pdmk_calg_guidance": ([vp, vp, i32, i32, i32, f32, vp, i64, vp, vp], i32),
    "pdmk_calg_plms_step": ([vp, i32, f32, vp, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_calg_ddim_step": ([vp, i32, f32, vp, i64, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_lms_step": ([vp, i32, f32, f32, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_sld_lms_step": ([vp, i32, f32, C.POINTER(SldParams), vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp],
                          i32),
    "pdmk_calg_lms_step": ([vp, i32, f32, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_image_to_u8": ([vp, vp, i32, i32, i32, vp], i32),
    "pdmk_image_to_u8_ex": ([vp, vp, i32, i32, i32, i32, vp], i32),
    "pdmk_resize_bilinear_u8": ([vp, i64, vp, vp, i32, i32, vp, vp], i32),
    "pdmk_image_resize_u8": ([vp, i64, vp, vp, i32, i32, i32, vp, vp], i32),
    "pdmk_conv2d_fwd": ([vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_conv2d_fwd_res": ([vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_softmax_topk": ([vp, i32, i32, i32, i32, vp, vp, vp], i32),
    "pdmk_zeroshot_head": ([vp, i32, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp], i32),
    "pdmk_pool2d": ([vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_global_avgpool": ([vp, i32, vp, i32, i32, i32, vp], i32),
    "pdmk_fid_accumulate": ([vp, i32, i32, i32, vp, vp, vp], i32),
    "pdmk_relu_pool": ([vp, i32, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    "pdmk_lpips_layer": ([vp, vp, i32, vp, vp, i32, i32, i32, vp], i32),
    "pdmk_gram_workspace_elems": ([i32, i32, i32], i64),
    "pdmk_gram_pair": ([vp, vp, i32, i32, i32, i32, vp, i64, vp, vp, vp], i32),
    "pdmk_rownorm_colsq_workspace_elems": ([i32, i32], i64),
    "pdmk_rownorm_colsq": ([vp, i32, i32, i32, i32, vp, vp, i64, vp], i32),
    "pdmk_wanda_count": ([vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp], i32),
    "pdmk_wanda_apply": ([vp, i32, i32, i32, i32, vp, f32, vp], i32),
    "pdmk_wanda_select": ([vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, i64, vp], i32),
    "pdmk_masked_weights": ([vp, vp, i32, vp, i32, vp, i64, i32, i32, vp, i32, vp], i32),
    "pdmk_spd_workspace_elems": ([i32, i32], i64),
    "pdmk_spd_system_f64": ([vp, f64, vp, f64, f64, vp, i32, i32, vp], i32),
    "pdmk_pair_gram_f64": ([vp, i32, i32, i32, f64, f64, vp, i32, vp], i32),
    "pdmk_spd_factor_f64": ([vp, i32, i32, vp, vp], i32),
    "pdmk_spd_solve_f64": ([vp, i32, i32, vp, i32, i32, vp, i32, vp, i32, vp, i64, vp], i32),
    "pdmk_uce_delta": ([vp, vp, vp, i32, i32, vp, i32, vp, i32, i32, vp, vp], i32),
    "pdmk_uce_debias_delta": ([vp, vp, vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, i64, vp], i32),
    "pdmk_gemm_splitk_workspace_bytes": ([i64, i32, i32], i64),
    "pdmk_groupnorm_workspace_bytes": ([i32, i32], i64),
    "pdmk_groupnorm_bwd_part_workspace_bytes": ([i32, i32], i64),
    "pdmk_layernorm_bwd_part_workspace_bytes": ([i32, i32], i64),
    "pdmk_attn_bwd_workspace_bytes": ([i32, i32, i32, i32], i64),
    "pdmk_attn_last_forms": ([], i32),
    "pdmk_plan_export": ([C.c_char_p], i32),
    "pdmk_plan_import": ([C.c_char_p], i32),
    "pdmk_plan_size": ([], i32),
    "pdmk_plan_clear": ([], i32),
    "pdmk_debug_scratch_violations": ([], i32),
    "pdmk_comm_unique_id": ([vp], i32),
    "pdmk_comm_create": ([vp, i32, i32, C.POINTER(vp)], i32),
    "pdmk_comm_allreduce_sum_f32": ([vp, vp, i64, vp], i32),
    "pdmk_comm_world": ([vp], i32),
    "pdmk_comm_rank": ([vp], i32),
    "pdmk_comm_reduce_scatter_sum_f32": ([vp, vp, i64, vp], i32),
    "pdmk_comm_allgather_f32": ([vp, vp, i64, vp], i32),
    "pdmk_stream_create": ([i32, C.POINTER(vp)], i32),
    "pdmk_stream_destroy": ([vp], i32),
    "pdmk_comm_destroy": ([vp], i32),
}
for _n, (_a, _r) in _SIGS.items():
    _f = getattr(_lib, _n)          # AttributeError here = header/library mismatch: fail at import
    _f.argtypes, _f.restype = _a, _r

EXPORTS = tuple(_SIGS)


def version():
    return _lib.pdmk_version()


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise PdmkError(f"unsupported dtype {t.dtype}")


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _chk(rc, name):
    if rc != 0:
        raise PdmkError(f"{name} failed with status {rc}")


PROFILE = None   # bench.py sets this to a list: every gemm launch is then bracketed by HIP events on the launch stream

# ---- grouped launches (pdmk_gemm_group): while RECORD is a list gemm() appends its filled argument block instead of launching;
# gemm_group() then issues the collected problems as one launch where the library has a kernel shape for all of them.
RECORD = None
GROUP_MAX = 8
STATS = {"launches": 0, "grouped": 0}      # launches issued through gemm_group since the last reset (tests / bench bookkeeping)


class Rec:
    """One recorded gemm() call: the argument block, the logical MACs (profiling) and the operand tensors, kept alive until
    the grouped launch has been issued."""
    __slots__ = ("g", "macs", "keep")
    kind = "gemm"       # the only kind left; the grouped-launch tests still assert it of every record

    def __init__(self, g, macs=None, keep=()):
        self.g, self.macs, self.keep = g, macs, keep


class Recorder:
    """with Recorder() as r: ...gemm() calls...;  r.recs is the list for gemm_group().  It collects the argument blocks of
    gemm() for one grouped launch and nothing else: every other launch wrapper runs at once, recording or not."""

    def __enter__(self):
        global RECORD
        self.prev, self.recs = RECORD, []
        RECORD = self.recs
        return self

    def __exit__(self, *exc):
        global RECORD
        RECORD = self.prev
        return False


def _prof_begin():
    """The HIP-event bracket of bench.py's per-kernel profile: (start, end) with start recorded on the launch stream, or None."""
    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    return ev


def _prof_end(ev, g, flops, shape, *tail):
    """Closes the bracket: PROFILE gets (kind, flops, e0, e1, shape), kind = (dtype, a_mode, b_mode, the candidate that ran) + tail."""
    if ev is not None:
        ev[1].record()
        kind = ("bf16" if g.dtype == BF16 else "f32", g.a_mode, g.b_mode, _lib.pdmk_gemm_last_candidate()) + tail
        PROFILE.append((kind, flops, ev[0], ev[1], shape))


def _launch_gemm(g, macs, shape):
    """pdmk_gemm on a filled argument block, bracketed by HIP events when PROFILE is a list.  Returns the status: what a
    non-zero one means is the caller's business (-2 = no fused kernel, for the GEGLU forms)."""
    ev = _prof_begin()
    rc = _lib.pdmk_gemm(C.byref(g), _st())
    if rc == 0:
        _prof_end(ev, g, 2.0 * (macs if macs is not None else g.M * g.N * g.K), shape)
    return rc


def gemm_group(recs):
    """Issue the GEMM records `recs` (2..GROUP_MAX independent problems) through pdmk_gemm_group: one launch where the
    library has a kernel shape for all of them (bit-identical to the separate launches), else one by one."""
    n = len(recs)
    arr = (GemmArgs * n)()
    for i, r in enumerate(recs):
        arr[i] = r.g
    got = i32(0)
    ev = _prof_begin()
    _chk(_lib.pdmk_gemm_group(arr, n, _st(), C.byref(got)), "pdmk_gemm_group")
    STATS["launches"] += 1 if got.value == n else n
    STATS["grouped"] += got.value
    _prof_end(ev, recs[0].g, sum(2.0 * (r.macs if r.macs is not None else r.g.M * r.g.N * r.g.K) for r in recs),
              [(r.g.M, r.g.N, r.g.K, int(r.g.splitk), int(bool(r.g.R) or r.g.accumulate == 1)) for r in recs], int(got.value))
    return int(got.value)


def _gemm_args(A, B, Cout, M, N, K, lda, ldb, ldc, *, bias=None, rowvec=None, rows_per_b=0, R=None, ldr=0, a_mode=A_ROWK,
               b_mode=B_ROWK, conv=None, dtype=None, out_f32=False, accumulate=False, splitk=1, alpha=1.0, colsum_out=None,
               ldrv=0, epilogue=EPI_NONE, C2=None, ldc2=0, colstat=None, ln=None):
    """The one place a pdmk_gemm_args block is filled (launches, plan and support queries alike).
    conv = (b, hi, wi, ci, ho, wo, mode, ld) or None; accumulate: False / True / 2 (= split-K slabs, see pdmk.h);
    colstat = (accumulator [B, 4, cs_ld] int64 limbs, first accumulator column of this output);
    ln = (gamma, beta, stats or None, out or None, eps): LayerNorm(A) in the GEMM's prologue (pdmk_gemm_args.ln_gamma)."""
    g = GemmArgs()
    g.A, g.B, g.C = _p(A), _p(B), _p(Cout)
    g.bias, g.rowvec, g.R, g.colsum_out = _p(bias), _p(rowvec), _p(R), _p(colsum_out)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc, g.ldr = lda, ldb, ldc, ldr
    g.rows_per_b, g.ldrv = rows_per_b, ldrv
    g.a_mode, g.b_mode = a_mode, b_mode
    if conv is not None:
        (g.conv_b, g.conv_hi, g.conv_wi, g.conv_ci, g.conv_ho, g.conv_wo, g.conv_mode, g.conv_ld) = conv
    g.dtype = dt(A) if dtype is None else dtype
    g.out_f32, g.accumulate, g.splitk, g.alpha = int(out_f32), int(accumulate), int(splitk), float(alpha)
    g.epilogue, g.C2, g.ldc2 = int(epilogue), _p(C2), int(ldc2)
    if colstat is not None:
        g.colstat, g.cs_ld, g.cs_col0 = _p(colstat[0]), colstat[0].shape[2], int(colstat[1])
    if ln is not None:
        gamma, beta, stats, out, eps = ln
        g.ln_gamma, g.ln_beta, g.ln_stats, g.ln_out = _p(gamma), _p(beta), _p(stats), _p(out)
        g.ld_ln_out, g.ln_eps = (0 if out is None else out.stride(0)), float(eps)
    return g


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, *, macs=None, **kw):
    """One pdmk_gemm launch (or, while a Recorder is open, one record of a grouped launch).  kw: every keyword of _gemm_args.
    macs: logical (un-padded) multiply-accumulates, profiling only."""
    g = _gemm_args(A, B, Cout, M, N, K, lda, ldb, ldc, **kw)
    if RECORD is not None:
        RECORD.append(Rec(g, macs, keep=(A, B, Cout, kw)))        # (kw holds every other operand tensor)
        return
    shape = (M, N, K, g.splitk, int(bool(g.R) or g.accumulate == 1))         # last: the epilogue also READS an [M, N] tensor
    _chk(_launch_gemm(g, macs, shape), "pdmk_gemm")


def gemm_ln_supported(A, B, M, N, K, lda, ldb, *, geglu=False, residual=False, bias=False):
    """Would pdmk_gemm take this Linear with the LayerNorm of its input fused into the prologue (one launch)?  Shape question only:
    the pointers are placeholders."""
    g = _gemm_args(A, B, A, M, N, K, lda, ldb, N // 2 if geglu else N, epilogue=EPI_GEGLU if geglu else EPI_NONE,
                   R=A if residual else None, ldr=N if residual else 0, bias=B if bias or geglu else None,
                   ln=(B, B, None, None, 1e-5))
    return bool(_lib.pdmk_gemm_ln_supported(C.byref(g)))


def _ws_bytes(n):
    if n < 0:
        raise PdmkError("workspace query rejected its arguments")
    return int(n)


def plan_export(path):
    _chk(_lib.pdmk_plan_export(os.fsencode(path)), "pdmk_plan_export")


def plan_import(path):
    n = _lib.pdmk_plan_import(os.fsencode(path))
    if n < 0:
        raise PdmkError(f"pdmk_plan_import({path!r}) failed with status {n}")
    return n


def plan_size():
    return int(_lib.pdmk_plan_size())


def plan_clear():
    _chk(_lib.pdmk_plan_clear(), "pdmk_plan_clear")


def debug_scratch_violations():
    """Tuning passes that overran their scratch since the process started (PDMK_DEBUG_SCRATCH=1; else 0)."""
    return int(_lib.pdmk_debug_scratch_violations())


class Comm:
    """pdmk_comm_t: RCCL communicator behind the C ABI (one per rank; `uid` = the 128 bytes rank 0 got from unique_id())."""

    def __init__(self, uid, rank, world):
        h = vp()
        buf = C.create_string_buffer(bytes(uid), 128)
        _chk(_lib.pdmk_comm_create(buf, rank, world, C.byref(h)), "pdmk_comm_create")
        self._h, self.rank, self.world = h, rank, world

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _chk(_lib.pdmk_comm_unique_id(buf), "pdmk_comm_unique_id")
        return bytes(buf.raw)

    def world_size(self):
        """What the HANDLE says (pdmk_comm_world / pdmk_comm_rank), not what the constructor was told."""
        return int(_lib.pdmk_comm_world(self._h))

    def rank_id(self):
        return int(_lib.pdmk_comm_rank(self._h))

    def all_reduce_sum_(self, t):
        """In-place sum over the ranks of a contiguous fp32 tensor, asynchronous on torch's current HIP stream."""
        assert t.dtype == torch.float32 and t.is_contiguous()
        _chk(_lib.pdmk_comm_allreduce_sum_f32(self._h, _p(t), t.numel(), _st()), "pdmk_comm_allreduce_sum_f32")

    def reduce_scatter_sum_(self, t):
        """t: contiguous fp32 bucket of world * n elements; afterwards this rank's share t[rank*n:(rank+1)*n] holds the sum."""
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() % self.world == 0
        _chk(_lib.pdmk_comm_reduce_scatter_sum_f32(self._h, _p(t), t.numel() // self.world, _st()),
             "pdmk_comm_reduce_scatter_sum_f32")

    def all_gather_(self, t):
        """Completes every rank's share of the bucket on every rank (second half of the all-reduce)."""
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() % self.world == 0
        _chk(_lib.pdmk_comm_allgather_f32(self._h, _p(t), t.numel() // self.world, _st()), "pdmk_comm_allgather_f32")

    def close(self):
        if self._h is not None:
            _lib.pdmk_comm_destroy(self._h)
            self._h = None


_ROLE_STREAMS = {}


def role_stream(device, role):
    """The process-wide dedicated HIP stream of a role ("teacher", "opt", "wt", "comm", "capture", ...) on `device`:
    created once through pdmk_stream_create and wrapped for torch - never one of torch's 32 pooled streams, which are handed
    out round-robin and start to alias after a few stepper / graph instances.  Never destroyed (work may be queued on it)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), role)
    s = _ROLE_STREAMS.get(key)
    if s is None:
        h = vp()
        with torch.cuda.device(key[0]):
            _chk(_lib.pdmk_stream_create(0, C.byref(h)), "pdmk_stream_create")
        s = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", key[0]))
        _ROLE_STREAMS[key] = s
    return s


def groupnorm_ws(device, B, G, have=None):
    """fp64 scratch of pdmk_groupnorm_fwd / _bwd, sized by the library; `have` is returned when it is already big enough."""
    need = _ws_bytes(_lib.pdmk_groupnorm_workspace_bytes(B, G)) // 8
    if have is not None and have.numel() >= need:
        return have
    return torch.empty(max(need, 1 << 17), device=device, dtype=torch.float64)


def zeros(shape, device, dtype):
    """torch.zeros without a memset node (see pdmk_zero in include/pdmk.h); byte size padded to 16."""
    n = 1
    for d in shape:
        n *= d
    esz = torch.empty((), dtype=dtype).element_size()
    pad = (-(n * esz)) % 16 // esz
    flat = torch.empty(n + pad, device=device, dtype=dtype)
    _chk(_lib.pdmk_zero(_p(flat), (n + pad) * esz, _st()), "pdmk_zero")
    return flat[:n].view(*shape)


def zero_(t):
    assert t.is_contiguous() and (t.numel() * t.element_size()) % 16 == 0
    _chk(_lib.pdmk_zero(_p(t), t.numel() * t.element_size(), _st()), "pdmk_zero")
    return t


def attn_last_forms():
    """(forward form, dQ form, dK/dV form, nsplit) of the calling thread's last attn_fwd[_causal] / attn_bwd: forms are 1 (16
    rows per wave) or 2 (32), nsplit the query split of dK/dV that ran."""
    w = int(_lib.pdmk_attn_last_forms())
    return w & 15, (w >> 4) & 15, (w >> 8) & 15, w >> 12


def last_candidate():
    """Candidate id of the calling thread's last pdmk_gemm launch (0 = K-step-32 kernels, 1.. = ring / halo shapes)."""
    return int(_lib.pdmk_gemm_last_candidate())


def last_form():
    """Form of candidate 0 the calling thread's last pdmk_gemm launched: 0 = none (an LDS-DMA candidate ran), 1 / 2 = igemm_kernel
    KCH 8 / KCH 4, 3 / 4 = igemm_dma_kernel BM 128 / BM 256."""
    return int(_lib.pdmk_gemm_last_form())


def candidate_name(a_mode, b_mode, cand):
    buf = C.create_string_buffer(160)
    _chk(_lib.pdmk_gemm_candidate_name(a_mode, b_mode, cand, buf, 160), "pdmk_gemm_candidate_name")
    return buf.value.decode()


def _plan(g):
    sk = i32(1)
    _chk(_lib.pdmk_gemm_plan(C.byref(g), _st(), C.byref(sk)), "pdmk_gemm_plan")
    return int(sk.value)


def splitk_plan(A, B, M, N, K, lda, ldb, a_mode=A_ROWK, conv=None):
    """Split-K factor for a forward/dgrad GEMM, from the library's plan cache (tuned on first sight of the shape)."""
    return _plan(_gemm_args(A, B, None, M, N, K, lda, ldb, N, a_mode=a_mode, conv=conv))


def wgrad_plan(dy, x, M, N, K, lda, ldb, b_mode=B_COLK, conv=None, slabs=False):
    """Split-K factor for a weight-gradient GEMM dW[M,N] += dy[K,M]^T x[K,N] (both operands reduction-major).
    slabs: the splits will store partial slabs (accumulate = 2) instead of adding with atomics - planned apart."""
    return _plan(_gemm_args(dy, x, None, M, N, K, lda, ldb, N, a_mode=A_COLK, b_mode=b_mode, conv=conv, dtype=dt(x),
                            out_f32=True, accumulate=2 if slabs else 0))


def gemm_auto(A, B, Cout, M, N, K, lda, ldb, ldc, *, bias=None, rowvec=None, rows_per_b=0, R=None, ldr=0,
              a_mode=A_ROWK, conv=None, accumulate=False, macs=None, ldrv=0, colstat=None):
    """Forward / dgrad GEMM with the split-K decision made by the planner: split shapes go through an fp32 workspace.
    colstat: (accumulator, first column): GroupNorm statistics of the stored output from the GEMM's epilogue, or from the finish
    pass of a split plan (M % 64 == 0 and rows_per_b % 64 == 0, bf16).  Returns True when the statistics were accumulated."""
    sk = splitk_plan(A, B, M, N, K, lda, ldb, a_mode, conv)
    if sk == 1:
        gemm(A, B, Cout, M, N, K, lda, ldb, ldc, bias=bias, rowvec=rowvec, rows_per_b=rows_per_b, R=R, ldr=ldr,
             a_mode=a_mode, conv=conv, accumulate=accumulate, macs=macs, ldrv=ldrv, colstat=colstat)
        return colstat is not None
    # split-K: every split stores its fp32 partial into its own slab (plain stores: no atomics, no zero-fill, the sum
    # order is fixed), the finish pass adds the slabs and applies the epilogue
    ws = torch.empty(_ws_bytes(_lib.pdmk_gemm_splitk_workspace_bytes(M, N, sk)) // 4, device=A.device, dtype=torch.float32)
    gemm(A, B, ws, M, N, K, lda, ldb, N, a_mode=a_mode, conv=conv, out_f32=True, splitk=sk, accumulate=2, macs=macs)
    splitk_finish(ws, Cout, M, N, ldc, sk, bias=bias, rowvec=rowvec, R=R, ldr=ldr, rows_per_b=rows_per_b, ldrv=ldrv,
                  accumulate=accumulate, colstat=colstat)
    return colstat is not None


def splitk_finish(ws, Cout, M, N, ldc, nslab, *, bias=None, rowvec=None, R=None, ldr=0, rows_per_b=0, ldrv=0,
                  accumulate=False, colstat=None):
    """colstat = (accumulator [B, 4, ld] int64, first column): the GroupNorm statistics of the stored output leave with this pass."""
    if colstat is not None:
        _chk(_lib.pdmk_splitk_finish_colstat(_p(ws), _p(Cout), _p(bias), _p(rowvec), _p(R), M, N, ldc, ldr, rows_per_b, ldrv,
                                             nslab, int(accumulate), _p(colstat[0]), colstat[0].shape[2], int(colstat[1]),
                                             dt(Cout), _st()), "pdmk_splitk_finish_colstat")
        return
    _chk(_lib.pdmk_splitk_finish(_p(ws), _p(Cout), _p(bias), _p(rowvec), _p(R), M, N, ldc, ldr, rows_per_b, ldrv, nslab,
                                 int(accumulate), dt(Cout), _st()), "pdmk_splitk_finish")


class SlabItem(C.Structure):
    _fields_ = [("ws", vp), ("dst", vp), ("n", i64), ("nslab", i32), ("pad_", i32)]


SLAB_GROUP_MAX = 32


class SlabQueue:
    """Deferred sums of weight-gradient split-K slabs (pdmk_splitk_finish_group): a weight gradient whose splits stored
    their partials into a [sk][M][N] workspace is added into its gradient later, up to 32 weights per launch."""

    def __init__(self, max_bytes=1 << 30):
        self.items, self.bytes, self.max_bytes = [], 0, max_bytes

    def add(self, ws, dW, n, nslab):
        self.items.append((ws, dW, n, nslab))       # ws stays referenced until the flush
        self.bytes += ws.numel() * 4

    def full(self):
        return len(self.items) >= SLAB_GROUP_MAX or self.bytes >= self.max_bytes

    def flush(self):
        while self.items:
            chunk, self.items = self.items[:SLAB_GROUP_MAX], self.items[SLAB_GROUP_MAX:]
            arr = (SlabItem * len(chunk))()
            for a, (ws, dW, n, nslab) in zip(arr, chunk):
                a.ws, a.dst, a.n, a.nslab = _p(ws), _p(dW), n, nslab
            _chk(_lib.pdmk_splitk_finish_group(C.cast(arr, vp), len(chunk), _st()), "pdmk_splitk_finish_group")
        self.bytes = 0


# one weight gradient dW[M, N] (fp32, row stride N) += dy[K, M]^T x[K, N]; colsum_out (or None) += the column sums of dy (the bias
# gradient); macs: logical multiply-accumulates, profiling only
WgradItem = namedtuple("WgradItem", "dy x dW M N K lda ldb colsum_out macs")


def _slab_ok(it):
    return (it.M * it.N) % 4 == 0 and it.dW.is_contiguous()


def _wgrad_gemm(it, sk, slab, b_mode=B_COLK, conv=None):
    """The gemm() of one weight gradient at split factor sk.  slab: the splits store their partials with plain stores into a fresh
    [sk][M][N] workspace - returned as a SlabQueue entry - else they add into dW (in the epilogue when unsplit, with fp32
    atomics when split)."""
    out = torch.empty(sk * it.M * it.N, device=it.dy.device, dtype=torch.float32) if slab else it.dW
    gemm(it.dy, it.x, out, it.M, it.N, it.K, it.lda, it.ldb, it.N, a_mode=A_COLK, b_mode=b_mode, conv=conv, out_f32=True,
         splitk=sk, accumulate=2 if slab else sk == 1, dtype=dt(it.x), macs=it.macs, colsum_out=it.colsum_out)
    return (out, it.dW, it.M * it.N, sk) if slab else None


def wgrad(dy, x, dW, M, N, K, lda, ldb, *, b_mode=B_COLK, conv=None, colsum_out=None, macs=None, queue=None):
    """dW[M, N] (fp32, row stride N) += dy[K, M]^T x[K, N] (3x3 gather of x for b_mode = B_COLK_CONV), split over the
    pixel dimension K as the planner says.  Without a queue the splits add into dW with fp32 atomics (a slab + finish pass
    PER WEIGHT was measured 4 % slower for the step: one more launch per weight outweighs the atomics).  queue (a
    SlabQueue): the splits store partial slabs with plain stores and the queue adds them into dW at its next flush, many
    weights per launch - no atomics and no per-weight launch."""
    it = WgradItem(dy, x, dW, M, N, K, lda, ldb, colsum_out, macs)
    slab = queue is not None and _slab_ok(it)
    sk = wgrad_plan(dy, x, M, N, K, lda, ldb, b_mode, conv, slabs=slab)
    if slab and sk > 1:
        if queue.full():
            queue.flush()
        queue.add(*_wgrad_gemm(it, sk, True, b_mode, conv))
    else:
        _wgrad_gemm(it, sk, False, b_mode, conv)


_WG_TARGET = int(os.environ.get("PDMK_WG_TARGET", "512"))     # workgroups a block's grouped weight-gradient launch aims for
_WG_MINK = int(os.environ.get("PDMK_WG_MINK", "32"))           # and the fewest 64-row K-steps a split may be left with


def wgrad_group(items, queue, target_wgs=None):
    """The Linear weight gradients of one transformer block (blocks.py:705-867 backward: to_q/k/v, to_out, ff.net.0.proj, ff.net.2,
    proj_in, proj_out; reached from accelerator.backward, trainer.py:2782) as grouped launches (pdmk_gemm_group): every item
    reduces over the SAME K pixel rows into a small [M, N] output, so one problem alone fills the 256 CUs only by cutting its
    reduction into 16-32 splits (16 K-steps each behind a cold prologue, 16-32 slabs to add); together the problems have the
    tiles, so they share ONE split factor chosen for the group (>= _WG_MINK K-steps per split) and one launch.
    items: WgradItem (or plain tuples in its field order) with dW contiguous; the splits of a reduction store their slabs for
    `queue` (a SlabQueue) to add later.  Problems the grouped kernels do not take go out one by one (same results)."""
    items = [WgradItem(*it) for it in items]
    while items:
        K = items[0].K
        same = [it for it in items if it.K == K][:GROUP_MAX]
        items = [it for it in items if not any(it is s_ for s_ in same)]
        if len(same) == 1 or queue is None:
            for it in same:
                wgrad(*it[:8], colsum_out=it.colsum_out, macs=it.macs, queue=queue)
            continue
        tiles = sum(((it.M + 127) // 128) * ((it.N + 127) // 128) for it in same)
        sk = max(1, min((target_wgs or _WG_TARGET) // max(tiles, 1), max(1, K // 64) // _WG_MINK, 64))
        with Recorder() as r:
            slabs = [_wgrad_gemm(it, sk, True) if sk > 1 and _slab_ok(it) else _wgrad_gemm(it, 1, False) for it in same]
        gemm_group(r.recs)
        for slab in filter(None, slabs):
            if queue.full():
                queue.flush()
            queue.add(*slab)


def groupnorm_apply_colstat(x, y, gamma, beta, stats, colstat, col0, B, HW, Cc, ldx, ldy, G, gs, eps, silu):
    """GroupNorm(+SiLU) forward with the statistics taken from a producing GEMM's epilogue sums (colstat [B, 4, cs_ld] int64 limbs)."""
    _chk(_lib.pdmk_groupnorm_apply_colstat(_p(x), _p(y), _p(gamma), _p(beta), _p(stats), _p(colstat), colstat.shape[2], int(col0),
                                           B, HW, Cc, ldx, ldy, G, gs, eps, int(silu), dt(x), _st()),
         "pdmk_groupnorm_apply_colstat")


def groupnorm_fwd(x, y, gamma, beta, stats, ws, B, HW, Cc, ldx, ldy, G, gs, eps, silu):
    _chk(_lib.pdmk_groupnorm_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(stats), _p(ws), B, HW, Cc, ldx, ldy, G, gs,
                                 eps, int(silu), dt(x), _st()), "pdmk_groupnorm_fwd")


_PART_WS = {}


def part_ws(device, elems):
    """Per-device fp32 scratch for the two-stage per-channel gradient reductions (reused launch after launch: all users
    are ordered on one stream)."""
    buf = _PART_WS.get(device)
    if buf is None or buf.numel() < elems:
        buf = torch.empty(max(elems, 1 << 22), device=device, dtype=torch.float32)
        _PART_WS[device] = buf
    return buf


class PartialItem(C.Structure):
    _fields_ = [("part", vp), ("out0", vp), ("out1", vp), ("nblk", i32), ("n", i32)]


PARTIAL_GROUP_MAX = 32


class PartialQueue:
    """Deferred second stage of the GroupNorm / LayerNorm parameter-gradient reductions (pdmk.h): each backward call leaves
    its per-block partials in a slab of its own; flush() sums up to 32 slabs per launch into dgamma / dbeta."""

    def __init__(self):
        self.items = []          # (slab tensor, dgamma, dbeta, nblk, n): the slab stays referenced until the flush

    def slab(self, device, nblk, n, dgamma, dbeta):
        if len(self.items) >= PARTIAL_GROUP_MAX:       # before the new slab joins: its kernel has not been launched yet
            self.flush()
        t = torch.empty(nblk * 2 * n, device=device, dtype=torch.float32)
        self.items.append((t, dgamma, dbeta, nblk, n))
        return t

    def flush(self):
        while self.items:
            chunk, self.items = self.items[:PARTIAL_GROUP_MAX], self.items[PARTIAL_GROUP_MAX:]
            arr = (PartialItem * len(chunk))()
            for a, (t, g0, g1, nblk, n) in zip(arr, chunk):
                a.part, a.out0, a.out1, a.nblk, a.n = _p(t), _p(g0), _p(g1), nblk, n
            _chk(_lib.pdmk_reduce_partials_group(C.cast(arr, vp), len(chunk), _st()), "pdmk_reduce_partials_group")


def _dims(fn, *args):
    a, b = i32(0), i32(0)
    _chk(fn(*args, C.byref(a), C.byref(b)), fn.__name__)
    return a.value, b.value


def groupnorm_bwd(x, dy, dx, gamma, beta, stats, dgamma, dbeta, ws, B, HW, Cc, ldx, lddy, lddx, G, gs, silu, acc, add=None,
                  queue=None):
    """queue: a PartialQueue - the dgamma / dbeta reduction is deferred to its next flush (one launch for many layers).
    add: a second finished gradient of x, [B * HW, Cc] with any row stride (the stride is taken from the tensor)."""
    if add is not None and add.dim() != 2:          # stride(0) of a [B, HW, C] view is the image stride: rows far out of the buffer
        raise PdmkError(f"groupnorm_bwd: add must be [B * HW, C] rows, got {tuple(add.shape)}")
    if queue is not None:
        nblk, n = _dims(_lib.pdmk_groupnorm_bwd_partial_dims, B, HW, Cc, G, gs, dt(x))
        pw = queue.slab(x.device, nblk, n, dgamma, dbeta)
        dgamma = dbeta = None
    else:
        pw = part_ws(x.device, _ws_bytes(_lib.pdmk_groupnorm_bwd_part_workspace_bytes(G, gs)) // 4)
    _chk(_lib.pdmk_groupnorm_bwd(_p(x), _p(dy), _p(dx), _p(gamma), _p(beta), _p(stats), _p(dgamma), _p(dbeta), _p(ws),
                                 _p(pw), pw.numel(), B, HW, Cc, ldx, lddy, lddx, G, gs, int(silu), int(acc), _p(add),
                                 0 if add is None else add.stride(0), dt(x), _st()), "pdmk_groupnorm_bwd")


def layernorm_fwd(x, y, gamma, beta, stats, M, Cc, ldx, ldy, eps):
    _chk(_lib.pdmk_layernorm_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(stats), M, Cc, ldx, ldy, eps, dt(x), _st()),
         "pdmk_layernorm_fwd")


def layernorm_bwd(x, dy, dx, gamma, stats, dgamma, dbeta, M, Cc, ldx, lddy, lddx, acc, queue=None, add=None):
    """add: a second finished gradient of x ([M, Cc], any row stride) folded into the store of dx."""
    if queue is not None:
        nblk, n = _dims(_lib.pdmk_layernorm_bwd_partial_dims, M, Cc)
        pw = queue.slab(x.device, nblk, n, dgamma, dbeta)
        dgamma = dbeta = None
    else:
        pw = part_ws(x.device, _ws_bytes(_lib.pdmk_layernorm_bwd_part_workspace_bytes(M, Cc)) // 4)
    _chk(_lib.pdmk_layernorm_bwd(_p(x), _p(dy), _p(dx), _p(gamma), _p(stats), _p(dgamma), _p(dbeta), _p(pw),
                                 pw.numel(), M, Cc, ldx, lddy, lddx, int(acc), _p(add), 0 if add is None else add.stride(0),
                                 dt(x), _st()), "pdmk_layernorm_bwd")


def attn_fwd(q, k, v, o, lse, B, H, Nq, Nk, qs, ks, vs, os_, scale):
    """qs/ks/vs/os_ = (batch_stride, row_stride) in elements."""
    _chk(_lib.pdmk_attn_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, H, Nq, Nk, qs[0], qs[1], ks[0], ks[1], vs[0],
                            vs[1], os_[0], os_[1], scale, dt(q), _st()), "pdmk_attn_fwd")


def attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, Nq, Nk, qs, ks, vs, os_, dqs, dks, dvs, scale, ws_elems=None):
    """ws_elems: floats of dK/dV split workspace to pass (None = what the library asks for, 0 = none; tests of the clamp)."""
    nws = _ws_bytes(_lib.pdmk_attn_bwd_workspace_bytes(B, H, Nq, Nk)) // 4   # > 0: few keys, the dK/dV pass also splits the queries
    if ws_elems is not None:
        nws = min(nws, int(ws_elems))
    ws = torch.empty(nws, device=q.device, dtype=torch.float32) if nws else None
    _chk(_lib.pdmk_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, H, Nq,
                            Nk, qs[0], qs[1], ks[0], ks[1], vs[0], vs[1], os_[0], os_[1], dqs[0], dqs[1], dks[0],
                            dks[1], dvs[0], dvs[1], scale, _p(ws), 0 if ws is None else ws.numel(), dt(q), _st()),
         "pdmk_attn_bwd")


def geglu_fwd(x, y, M, Fd, ldx, ldy, layout=0):
    """layout 0: x = [h | g] halves; 1: (h, g) interleaved in blocks of 8 columns (what EPI_GEGLU consumes)."""
    _chk(_lib.pdmk_geglu_fwd(_p(x), _p(y), M, Fd, ldx, ldy, int(layout), dt(x), _st()), "pdmk_geglu_fwd")


def geglu_bwd(x, dy, dx, M, Fd, ldx, lddy, lddx, layout=0):
    _chk(_lib.pdmk_geglu_bwd(_p(x), _p(dy), _p(dx), M, Fd, ldx, lddy, lddx, int(layout), dt(x), _st()), "pdmk_geglu_bwd")


_GEGLU_REFUSED = set()     # (M, N, K) the library has no fused GEGLU kernel for (learnt from eager calls: status -2)


def gemm_geglu(A, B, gl, f, M, N, K, lda, ldb, *, bias=None, macs=None, ln=None):
    """gl[M, N/2] = GEGLU(A @ B^T + bias) in the GEMM's epilogue, (hidden, gate) columns interleaved in blocks of 8; f (or
    None) receives the [M, N] pre-activation for the backward.  Returns False when the library has no fused kernel for
    the shape (status -2) - the caller then runs the projection and pdmk_geglu_fwd(layout=1) as two passes."""
    if (M, N, K) in _GEGLU_REFUSED:
        return False
    g = _gemm_args(A, B, gl, M, N, K, lda, ldb, gl.stride(0), bias=bias, epilogue=EPI_GEGLU, C2=f,
                   ldc2=0 if f is None else f.stride(0), ln=ln)
    if RECORD is not None:      # a member of a grouped launch: the library answers for the whole group (pdmk_gemm_group)
        RECORD.append(Rec(g, macs, keep=(A, B, gl, f, bias, ln)))
        return True
    rc = _launch_gemm(g, macs, (M, N, K, 1))
    if rc == -2:
        if ln is None:
            _GEGLU_REFUSED.add((M, N, K))
        return False
    _chk(rc, "pdmk_gemm[geglu]")
    return True


def gemm_geglu_bwd(dy, wt, pre, dpre, M, N, K, lddy, ldwt, *, macs=None):
    """dpre[M, 2N] = gradient of the GEGLU pre-activation `pre` [M, 2N] (interleaved layout) given dy [M, K], the gradient of the
    Linear that consumed hidden * gelu(gate): (dy @ wt^T) pushed through GEGLU's backward in the GEMM's epilogue
    (PDMK_EPI_GEGLU_BWD).  Returns False when the library has no fused kernel for the shape (the caller then runs the plain
    input-gradient GEMM and pdmk_geglu_bwd)."""
    g = _gemm_args(dy, wt, dpre, M, N, K, lddy, ldwt, dpre.stride(0), epilogue=EPI_GEGLU_BWD, C2=pre, ldc2=pre.stride(0))
    rc = _launch_gemm(g, macs, (M, N, K, 1))
    if rc != -2:
        _chk(rc, "pdmk_gemm[geglu_bwd]")
    return rc == 0


def quantize_e4m3_(x):
    """In place: every element of the contiguous tensor x rounded to the nearest e4m3fn value (pdmk_quantize_e4m3)."""
    assert x.is_contiguous()
    _chk(_lib.pdmk_quantize_e4m3(_p(x), _p(x), x.numel(), dt(x), _st()), "pdmk_quantize_e4m3")


def silu_fwd(x, y):
    _chk(_lib.pdmk_silu_fwd(_p(x), _p(y), x.numel(), dt(x), _st()), "pdmk_silu_fwd")


def silu_bwd(x, dy, dx):
    _chk(_lib.pdmk_silu_bwd(_p(x), _p(dy), _p(dx), x.numel(), dt(x), _st()), "pdmk_silu_bwd")


def copy2d(src, dst, rows, cols, lds, ldd, accumulate=False):
    _chk(_lib.pdmk_copy2d(_p(src), _p(dst), rows, cols, lds, ldd, int(accumulate), dt(src), _st()), "pdmk_copy2d")


def cast_permute(src, dst, n0, n1, n2, mode):
    _chk(_lib.pdmk_cast_permute(_p(src), _p(dst), n0, n1, n2, mode, dt(dst), _st()), "pdmk_cast_permute")


def colsum(x, out, rows, N, ld, accumulate=False, nbatch=1, ldo=0):
    _chk(_lib.pdmk_colsum(_p(x), _p(out), rows, N, ld, int(accumulate), nbatch, ldo, dt(x), _st()), "pdmk_colsum")


def skinny_gemm(x, w, y, M, N, K, ldx, ldw, ldy, bias=None, accumulate=False):
    """y[M<=16, N] (+)= x @ w[N, K]^T + bias  (w in the compute dtype; x bf16/fp32; y fp32 or the compute dtype)."""
    _chk(_lib.pdmk_skinny_gemm(_p(x), dt(x), _p(w), _p(y), _p(bias), M, N, K, ldx, ldw, ldy, dt(w),
                               int(y.dtype == torch.float32), int(accumulate), _st()), "pdmk_skinny_gemm")


def skinny_wgrad(dy, x, dw, dbias, M, N, K, lddy, ldx, lddw):
    _chk(_lib.pdmk_skinny_wgrad(_p(dy), dt(dy), _p(x), _p(dw), _p(dbias), M, N, K, lddy, ldx, lddw, dt(x), _st()),
         "pdmk_skinny_wgrad")


def pool2x2_sum(src, dst, B, H, W, Cc):
    _chk(_lib.pdmk_pool2x2_sum(_p(src), _p(dst), B, H, W, Cc, dt(src), _st()), "pdmk_pool2x2_sum")


def timestep_embed(t, freqs, out, B, dim):
    """t int64 [B] (pdmk_timestep_embed) or float32 [B] (pdmk_timestep_embed_f32: K-LMS's fractional timesteps)."""
    if t.dtype == torch.int64:
        _chk(_lib.pdmk_timestep_embed(_p(t), _p(freqs), _p(out), B, dim, dt(out), _st()), "pdmk_timestep_embed")
    elif t.dtype == torch.float32:
        _chk(_lib.pdmk_timestep_embed_f32(_p(t), _p(freqs), _p(out), B, dim, dt(out), _st()), "pdmk_timestep_embed_f32")
    else:
        raise PdmkError(f"timestep_embed: timesteps are int64 or float32, not {t.dtype}")


def scale_div(x, y, div):
    """y = x / div on contiguous fp32 tensors of one size: one fp32 division per element (pdmk_scale_div)."""
    if not _f32c(x, y) or x.numel() != y.numel() or x.numel() == 0:
        raise PdmkError("scale_div: x, y fp32 contiguous of one size")
    _chk(_lib.pdmk_scale_div(_p(x), _p(y), float(div), x.numel(), _st()), "pdmk_scale_div")


def add_noise_velocity(x0, noise, t, sa, sb, noisy, target, B, Cc, HW, cpad):
    _chk(_lib.pdmk_add_noise_velocity(_p(x0), _p(noise), _p(t), _p(sa), _p(sb), _p(noisy), _p(target), B, Cc, HW, cpad,
                                      dt(noisy), _st()), "pdmk_add_noise_velocity")


def nchw_to_nhwc(src, dst, B, Cc, HW, cpad):
    _chk(_lib.pdmk_nchw_to_nhwc(_p(src), _p(dst), B, Cc, HW, cpad, dt(dst), _st()), "pdmk_nchw_to_nhwc")


def embed_tokens(ids, tok, pos, out, ntok, T, D, vocab, ldt, ldp, ldo):
    _chk(_lib.pdmk_embed_tokens(_p(ids), _p(tok), _p(pos), _p(out), ntok, T, D, vocab, ldt, ldp, ldo, dt(out), _st()),
         "pdmk_embed_tokens")


def attn_fwd_causal(q, kk, v, o, lse, B, H, N, qs, ks, vs, os_, scale):
    """qs / ks / vs / os_ = (batch stride, row stride) in elements, as attn_fwd."""
    _chk(_lib.pdmk_attn_fwd_causal(_p(q), _p(kk), _p(v), _p(o), _p(lse), B, H, N, qs[0], qs[1], ks[0], ks[1], vs[0], vs[1],
                                   os_[0], os_[1], float(scale), dt(q), _st()), "pdmk_attn_fwd_causal")


def gelu_fwd(x, y):
    _chk(_lib.pdmk_gelu_fwd(_p(x), _p(y), x.numel(), dt(x), _st()), "pdmk_gelu_fwd")


def image_prep(src, desc, desc_dev, out):
    """Resize / crop / flip / normalise a packed batch of uint8 RGB images into out ([B, 3, R, R] fp32 on the device).
    src: uint8 device tensor holding the images back to back (offsets in desc); desc: int64 [B, 8] HOST tensor
    (offset, h, w, rh, rw, top, left, flip); desc_dev: the same descriptors on the device (what the kernel reads)."""
    B, R = out.shape[0], out.shape[-1]
    if (desc.device.type != "cpu" or desc.dtype != torch.int64 or tuple(desc.shape) != (B, 8) or not desc.is_contiguous()
            or desc_dev.dtype != torch.int64 or desc_dev.numel() != 8 * B or not desc_dev.is_contiguous()
            or src.dtype != torch.uint8 or out.dtype != torch.float32 or tuple(out.shape) != (B, 3, R, R)
            or not out.is_contiguous()):
        raise PdmkError("image_prep: src uint8, desc int64 [B, 8] on the host, desc_dev its device copy, out fp32 [B, 3, R, R]")
    _chk(_lib.pdmk_image_prep(_p(src), src.numel(), _p(desc), _p(desc_dev), B, R, _p(out), _st()), "pdmk_image_prep")


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def image_prep_ex(src, desc, desc_dev, out, filter=1, mean=CLIP_MEAN, std=CLIP_STD):
    """image_prep with the resample filter (0 bilinear, 1 Pillow bicubic) and the Normalize(mean, std) as parameters."""
    B, R = out.shape[0], out.shape[-1]
    if (desc.device.type != "cpu" or desc.dtype != torch.int64 or tuple(desc.shape) != (B, 8) or not desc.is_contiguous()
            or desc_dev.dtype != torch.int64 or desc_dev.numel() != 8 * B or not desc_dev.is_contiguous()
            or src.dtype != torch.uint8 or out.dtype != torch.float32 or tuple(out.shape) != (B, 3, R, R)
            or not out.is_contiguous()):
        raise PdmkError("image_prep_ex: src uint8, desc int64 [B, 8] on the host, desc_dev its device copy, out fp32 [B, 3, R, R]")
    m, s = (f32 * 3)(*mean), (f32 * 3)(*std)
    _chk(_lib.pdmk_image_prep_ex(_p(src), src.numel(), _p(desc), _p(desc_dev), B, R, int(filter), m, s, _p(out), _st()),
         "pdmk_image_prep_ex")


def patch_im2col(x, out, B, S, p):
    """x fp32 [B, 3, S, S] -> out [B * (S / p)^2, ld] rows in the compute dtype, columns (c, ky, kx), padding columns 0."""
    _chk(_lib.pdmk_patch_im2col(_p(x), _p(out), B, S, p, out.stride(0), dt(out), _st()), "pdmk_patch_im2col")


def vit_tokens(patches, cls, pos, ldpos, out, B, G2, E):
    _chk(_lib.pdmk_vit_tokens(_p(patches), patches.stride(0), _p(cls), _p(pos), ldpos, _p(out), out.stride(0), B, G2, E,
                              dt(out), _st()), "pdmk_vit_tokens")


def quick_gelu_fwd(x, y):
    _chk(_lib.pdmk_quick_gelu_fwd(_p(x), _p(y), x.numel(), dt(x), _st()), "pdmk_quick_gelu_fwd")


def gather_rows(x, ids, T, out, B, D):
    """out[b] = x[b * T + j] with j = 0 (ids None: CLS) or the first argmax of ids[b] (EOT), computed on the device."""
    _chk(_lib.pdmk_gather_rows(_p(x), x.stride(0), _p(ids), T, _p(out), out.stride(0), B, D, dt(x), _st()),
         "pdmk_gather_rows")


def clip_score_head(a, b, an, bn, acc, B, D):
    """fp32 rows: an = a / |a|, bn = b / |b|, acc (fp64 [1] on the device) += sum of the row dot products."""
    _chk(_lib.pdmk_clip_score_head(_p(a), a.stride(0), _p(b), 0 if b is None else b.stride(0), _p(an), _p(bn), _p(acc), B,
                                   D, _st()), "pdmk_clip_score_head")


def cosine_pairs(t, a, b, sim_a, sim_b, b_lt_a):
    """fp32 rows t / a / b [B, D] (unit column stride): sim_a[r] = cos(t_r, a_r), sim_b[r] = cos(t_r, b_r) (norms clamped at
    1e-8), b_lt_a[r] = sim_b[r] < sim_a[r].  sim_a / sim_b fp32 [B], b_lt_a int32 [B], contiguous."""
    B, D = t.shape
    for x in (t, a, b):
        if x.dtype != torch.float32 or x.dim() != 2 or tuple(x.shape) != (B, D) or x.stride(1) != 1 or x.stride(0) < D:
            raise PdmkError("cosine_pairs: t, a, b fp32 [B, D] of one shape with unit column stride")
    for x, d in ((sim_a, torch.float32), (sim_b, torch.float32), (b_lt_a, torch.int32)):
        if x.dtype != d or tuple(x.shape) != (B,) or not x.is_contiguous():
            raise PdmkError("cosine_pairs: sim_a, sim_b fp32 [B] and b_lt_a int32 [B], contiguous")
    _chk(_lib.pdmk_cosine_pairs(_p(t), t.stride(0), _p(a), a.stride(0), _p(b), b.stride(0), _p(sim_a), _p(sim_b),
                                _p(b_lt_a), B, D, _st()), "pdmk_cosine_pairs")


def plms_table(rows, device):
    """A list of PlmsRow -> the uint8 device tensor pdmk_plms_step reads (one host-to-device copy)."""
    arr = (PlmsRow * len(rows))(*rows)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def plms_step(pred, ld, g_u, g_t, cfg, sample, cur, ets, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """One fused guidance + PLMS step (include/pdmk.h pdmk_plms_step).  pred / x_next in the engine dtype; sample, cur
    fp32 [B*Cc*HW]; ets fp32 [4, B*Cc*HW]; table from plms_table() with nsteps rows; state int32 [2]; t_out int64."""
    n = B * Cc * HW
    rows = (2 * B if cfg else B) * HW
    avail = pred.untyped_storage().nbytes() // pred.element_size() - pred.storage_offset()     # (pred may be a strided view)
    if (pred.dtype != x_next.dtype or avail < (rows - 1) * ld + Cc or x_next.numel() < rows * cpad
            or any(t.dtype != torch.float32 or not t.is_contiguous() for t in (sample, cur, ets))
            or sample.numel() != n or cur.numel() != n or ets.numel() != 4 * n or table.dtype != torch.uint8
            or table.numel() != nsteps * C.sizeof(PlmsRow) or state.dtype != torch.int32 or state.numel() != 2
            or t_out.dtype != torch.int64 or t_out.numel() < (2 * B if cfg else B)):
        raise PdmkError("plms_step: inconsistent buffers")
    _chk(_lib.pdmk_plms_step(_p(pred), ld, float(g_u), float(g_t), int(bool(cfg)), _p(sample), _p(cur), _p(ets), _p(table),
                             nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()), "pdmk_plms_step")


def ddim_table(rows, device):
    """A list of DdimRow -> the uint8 device tensor pdmk_ddim_step reads (one host-to-device copy)."""
    arr = (DdimRow * len(rows))(*rows)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def ddim_step(pred, ld, g_u, g_t, cfg, sample, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """One fused guidance + DDIM step (include/pdmk.h pdmk_ddim_step).  pred / x_next in the engine dtype; sample fp32
    [B*Cc*HW]; table from ddim_table() with nsteps rows; state int32 [2]; t_out int64."""
    n = B * Cc * HW
    rows = (2 * B if cfg else B) * HW
    avail = pred.untyped_storage().nbytes() // pred.element_size() - pred.storage_offset()     # (pred may be a strided view)
    if (pred.dtype != x_next.dtype or ld < Cc or cpad < Cc or avail < (rows - 1) * ld + Cc or x_next.numel() < rows * cpad
            or sample.dtype != torch.float32 or not sample.is_contiguous() or sample.numel() != n
            or table.dtype != torch.uint8 or table.numel() != nsteps * C.sizeof(DdimRow) or state.dtype != torch.int32
            or state.numel() != 2 or t_out.dtype != torch.int64 or t_out.numel() < (2 * B if cfg else B)):
        raise PdmkError("ddim_step: inconsistent buffers")
    _chk(_lib.pdmk_ddim_step(_p(pred), ld, float(g_u), float(g_t), int(bool(cfg)), _p(sample), _p(table), nsteps, _p(state),
                             _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()), "pdmk_ddim_step")


def lms_table(rows, device):
    """A list of LmsRow -> the uint8 device tensor pdmk_lms_step reads (one host-to-device copy)."""
    arr = (LmsRow * len(rows))(*rows)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def lms_step(pred, ld, g_u, g_t, cfg, sample, hist, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """One fused guidance + K-LMS step (include/pdmk.h pdmk_lms_step).  pred / x_next in the engine dtype; sample fp32
    [B*Cc*HW]; hist fp32 [4, B*Cc*HW]; table from lms_table() with nsteps rows; state int32 [2]; t_out FLOAT32."""
    n = B * Cc * HW
    rows = (2 * B if cfg else B) * HW
    if (pred.dtype != x_next.dtype or ld < Cc or cpad < Cc or _avail(pred) < (rows - 1) * ld + Cc
            or x_next.numel() < rows * cpad or not x_next.is_contiguous() or not _f32c(sample, hist) or sample.numel() != n
            or hist.numel() != 4 * n or table.dtype != torch.uint8 or table.numel() != nsteps * C.sizeof(LmsRow)
            or state.dtype != torch.int32 or state.numel() != 2 or t_out.dtype != torch.float32
            or t_out.numel() < (2 * B if cfg else B)):
        raise PdmkError("lms_step: inconsistent buffers")
    _chk(_lib.pdmk_lms_step(_p(pred), ld, float(g_u), float(g_t), int(bool(cfg)), _p(sample), _p(hist), _p(table), nsteps,
                            _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()), "pdmk_lms_step")


def sld_params(sld_guidance_scale, warmup_steps, threshold, momentum_scale, mom_beta):
    """The five SLD scalars (Python numbers, i.e. doubles) -> SldParams: each rounded once to fp32, `1 - mom_beta` formed in
    double first - what torch does with a Python scalar operand of an fp32 tensor."""
    return SldParams(sld_guidance_scale=float(sld_guidance_scale), threshold=float(threshold),
                     momentum_scale=float(momentum_scale), mom_beta=float(mom_beta), one_minus_beta=1.0 - float(mom_beta),
                     warmup_steps=int(warmup_steps))


def _f32c(*ts):
    return all(t.dtype == torch.float32 and t.is_contiguous() for t in ts)


def sld_guidance(pred, out, mom, guidance_scale, params, apply):
    """SLD guidance of the eager loop (include/pdmk.h pdmk_sld_guidance): pred fp32 [3B, C, H, W] contiguous (uncond, text,
    safety) -> out fp32 [B, C, H, W]; mom fp32 [B, C, H, W] updated in place.  apply: call index >= warm-up."""
    if (not _f32c(pred, out, mom) or pred.dim() != 4 or pred.shape[0] % 3 or out.shape != mom.shape
            or tuple(out.shape) != (pred.shape[0] // 3,) + tuple(pred.shape[1:]) or not isinstance(params, SldParams)):
        raise PdmkError("sld_guidance: pred fp32 [3B, C, H, W], out / mom fp32 [B, C, H, W], contiguous; params SldParams")
    B, Cc, H, W = out.shape
    _chk(_lib.pdmk_sld_guidance(_p(pred), _p(out), _p(mom), B, Cc, H * W, float(guidance_scale), C.byref(params),
                                int(bool(apply)), _st()), "pdmk_sld_guidance")


def _sld_step_ok(pred, ld, params, mom, sample, table, row, nsteps, state, t_out, x_next, cpad, B, Cc, HW, tdtype=torch.int64):
    n, rows = B * Cc * HW, 3 * B * HW
    return (isinstance(params, SldParams) and pred.dtype == x_next.dtype and ld >= Cc and cpad >= Cc
            and _avail(pred) >= (rows - 1) * ld + Cc and x_next.numel() >= rows * cpad and x_next.is_contiguous()
            and _f32c(mom, sample) and mom.numel() == n and sample.numel() == n and table.dtype == torch.uint8
            and table.numel() == nsteps * C.sizeof(row) and state.dtype == torch.int32 and state.numel() == 2
            and t_out.dtype == tdtype and t_out.numel() >= 3 * B)


def sld_plms_step(pred, ld, guidance_scale, params, mom, sample, cur, ets, table, nsteps, state, t_out, x_next, cpad, B, Cc,
                  HW):
    """plms_step with SLD guidance (include/pdmk.h pdmk_sld_plms_step): pred / x_next rows of 3B * HW pixels (uncond, text,
    safety); mom fp32 [B*Cc*HW]; the warm-up is decided on the device from state[0] and params.warmup_steps."""
    n = B * Cc * HW
    if (not _sld_step_ok(pred, ld, params, mom, sample, table, PlmsRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW)
            or not _f32c(cur, ets) or cur.numel() != n or ets.numel() != 4 * n):
        raise PdmkError("sld_plms_step: inconsistent buffers")
    _chk(_lib.pdmk_sld_plms_step(_p(pred), ld, float(guidance_scale), C.byref(params), _p(mom), _p(sample), _p(cur), _p(ets),
                                 _p(table), nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()),
         "pdmk_sld_plms_step")


def sld_ddim_step(pred, ld, guidance_scale, params, mom, sample, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """ddim_step with SLD guidance (include/pdmk.h pdmk_sld_ddim_step); buffers as sld_plms_step, no history."""
    if not _sld_step_ok(pred, ld, params, mom, sample, table, DdimRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
        raise PdmkError("sld_ddim_step: inconsistent buffers")
    _chk(_lib.pdmk_sld_ddim_step(_p(pred), ld, float(guidance_scale), C.byref(params), _p(mom), _p(sample), _p(table), nsteps,
                                 _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()), "pdmk_sld_ddim_step")


def sld_lms_step(pred, ld, guidance_scale, params, mom, sample, hist, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """lms_step with SLD guidance (include/pdmk.h pdmk_sld_lms_step); buffers as sld_plms_step, hist fp32 [4, B*Cc*HW],
    t_out float32."""
    if (not _sld_step_ok(pred, ld, params, mom, sample, table, LmsRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW,
                         tdtype=torch.float32) or not _f32c(hist) or hist.numel() != 4 * B * Cc * HW):
        raise PdmkError("sld_lms_step: inconsistent buffers")
    _chk(_lib.pdmk_sld_lms_step(_p(pred), ld, float(guidance_scale), C.byref(params), _p(mom), _p(sample), _p(hist), _p(table),
                                nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()),
         "pdmk_sld_lms_step")


def calg_workspace_elems(B, Cc, HW):
    """fp64 elements of concept algebra's partial-sum workspace for a [B, Cc, HW] latent (pdmk_calg_workspace_elems)."""
    return int(_lib.pdmk_calg_workspace_elems(B, Cc, HW))


def _calg_ws_ok(ws, scalars, B, Cc, HW):
    return (ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= calg_workspace_elems(B, Cc, HW) > 0
            and (scalars is None or (scalars.dtype == torch.float32 and scalars.is_contiguous() and scalars.numel() >= 2)))


def calg_dots(pred, ld, B, Cc, HW, ws):
    """Concept algebra's two sums as per-workgroup fp64 pairs in ws (include/pdmk.h pdmk_calg_dots): pred rows of 5B * HW
    pixels (uncond, text, p0, p1, p2), f32 or bf16.  fp32 NCHW fifths go in as (ld = 1, Cc = 1, HW = C * H * W): same bits."""
    if not _calg_ws_ok(ws, None, B, Cc, HW) or ld < Cc or _avail(pred) < (5 * B * HW - 1) * ld + Cc:
        raise PdmkError("calg_dots: inconsistent buffers")
    _chk(_lib.pdmk_calg_dots(_p(pred), ld, B, Cc, HW, dt(pred), _p(ws), ws.numel(), _st()), "pdmk_calg_dots")


def calg_guidance(pred, out, guidance_scale, ws, scalars=None):
    """Concept-algebra guidance of the eager loop (include/pdmk.h pdmk_calg_guidance): pred fp32 [5B, C, H, W] contiguous ->
    out fp32 [B, C, H, W]; ws as calg_dots left it; scalars (fp32 [2], optional) receives nrm, dot."""
    if (not _f32c(pred, out) or pred.dim() != 4 or pred.shape[0] % 5
            or tuple(out.shape) != (pred.shape[0] // 5,) + tuple(pred.shape[1:])
            or not _calg_ws_ok(ws, scalars, out.shape[0], out.shape[1], out.shape[2] * out.shape[3])):
        raise PdmkError("calg_guidance: pred fp32 [5B, C, H, W], out fp32 [B, C, H, W], contiguous; ws fp64 of "
                        "calg_workspace_elems, scalars fp32 [2]")
    B, Cc, H, W = out.shape
    _chk(_lib.pdmk_calg_guidance(_p(pred), _p(out), B, Cc, H * W, float(guidance_scale), _p(ws), ws.numel(), _p(scalars),
                                 _st()), "pdmk_calg_guidance")


def _calg_step_ok(pred, ld, ws, scalars, sample, table, row, nsteps, state, t_out, x_next, cpad, B, Cc, HW, tdtype=torch.int64):
    n, rows = B * Cc * HW, 5 * B * HW
    return (_calg_ws_ok(ws, scalars, B, Cc, HW) and pred.dtype == x_next.dtype and ld >= Cc and cpad >= Cc
            and _avail(pred) >= (rows - 1) * ld + Cc and x_next.numel() >= rows * cpad and x_next.is_contiguous()
            and _f32c(sample) and sample.numel() == n and table.dtype == torch.uint8
            and table.numel() == nsteps * C.sizeof(row) and state.dtype == torch.int32 and state.numel() == 2
            and t_out.dtype == tdtype and t_out.numel() >= 5 * B)


def calg_plms_step(pred, ld, guidance_scale, ws, scalars, sample, cur, ets, table, nsteps, state, t_out, x_next, cpad, B, Cc,
                   HW):
    """plms_step with concept-algebra guidance (include/pdmk.h pdmk_calg_plms_step): pred / x_next rows of 5B * HW pixels;
    ws holds the pairs of calg_dots on the same pred."""
    n = B * Cc * HW
    if (not _calg_step_ok(pred, ld, ws, scalars, sample, table, PlmsRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW)
            or not _f32c(cur, ets) or cur.numel() != n or ets.numel() != 4 * n):
        raise PdmkError("calg_plms_step: inconsistent buffers")
    _chk(_lib.pdmk_calg_plms_step(_p(pred), ld, float(guidance_scale), _p(ws), ws.numel(), _p(scalars), _p(sample), _p(cur),
                                  _p(ets), _p(table), nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred),
                                  _st()), "pdmk_calg_plms_step")


def calg_ddim_step(pred, ld, guidance_scale, ws, scalars, sample, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """ddim_step with concept-algebra guidance (include/pdmk.h pdmk_calg_ddim_step); buffers as calg_plms_step, no history."""
    if not _calg_step_ok(pred, ld, ws, scalars, sample, table, DdimRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
        raise PdmkError("calg_ddim_step: inconsistent buffers")
    _chk(_lib.pdmk_calg_ddim_step(_p(pred), ld, float(guidance_scale), _p(ws), ws.numel(), _p(scalars), _p(sample), _p(table),
                                  nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()),
         "pdmk_calg_ddim_step")


def calg_lms_step(pred, ld, guidance_scale, ws, scalars, sample, hist, table, nsteps, state, t_out, x_next, cpad, B, Cc, HW):
    """lms_step with concept-algebra guidance (include/pdmk.h pdmk_calg_lms_step); buffers as calg_plms_step, hist fp32
    [4, B*Cc*HW], t_out float32."""
    if (not _calg_step_ok(pred, ld, ws, scalars, sample, table, LmsRow, nsteps, state, t_out, x_next, cpad, B, Cc, HW,
                          tdtype=torch.float32) or not _f32c(hist) or hist.numel() != 4 * B * Cc * HW):
        raise PdmkError("calg_lms_step: inconsistent buffers")
    _chk(_lib.pdmk_calg_lms_step(_p(pred), ld, float(guidance_scale), _p(ws), ws.numel(), _p(scalars), _p(sample), _p(hist),
                                 _p(table), nsteps, _p(state), _p(t_out), _p(x_next), cpad, B, Cc, HW, dt(pred), _st()),
         "pdmk_calg_lms_step")


def _u8_shape(src, dst, name):
    B, Cc, H, W = src.shape
    if (src.dtype != torch.float32 or not src.is_contiguous() or dst.dtype != torch.uint8 or not dst.is_contiguous()
            or tuple(dst.shape) != (B, H, W, Cc)):
        raise PdmkError(f"{name}: src fp32 contiguous [B, C, H, W], dst uint8 contiguous [B, H, W, C]")
    return B, Cc, H * W


def image_to_u8(src, dst):
    """uint8 NHWC dst [B, H, W, C] = trunc(255 * clamp(src / 2 + 0.5, 0, 1)) of the fp32 NCHW decoder output src."""
    _chk(_lib.pdmk_image_to_u8(_p(src), _p(dst), *_u8_shape(src, dst, "image_to_u8"), _st()), "pdmk_image_to_u8")


def image_to_u8_ex(src, dst, rounding):
    """image_to_u8 with the last step chosen: rounding 0 truncates (image_to_u8), 1 rounds half to even first (diffusers'
    numpy_to_pil)."""
    _chk(_lib.pdmk_image_to_u8_ex(_p(src), _p(dst), *_u8_shape(src, dst, "image_to_u8_ex"), int(rounding), _st()),
         "pdmk_image_to_u8_ex")


def _avail(t):
    """Elements from t's first element to the end of its storage (t may be a strided view of a wider buffer)."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _desc_ok(desc, desc_dev, B):
    return (desc.device.type == "cpu" and desc.dtype == torch.int64 and tuple(desc.shape) == (B, 8) and desc.is_contiguous()
            and desc_dev.dtype == torch.int64 and desc_dev.numel() == 8 * B and desc_dev.is_contiguous())


def resize_bilinear_u8(src, desc, desc_dev, out):
    """Packed uint8 HWC images (desc as image_prep: offset, h, w used) -> out fp32 NHWC [B, S, S, 3] in [-1, 1]: torch's
    CPU bilinear F.interpolate (no antialiasing), clip, / 255, * 2 - 1."""
    B, S = out.shape[0], out.shape[1]
    if (not _desc_ok(desc, desc_dev, B) or src.dtype != torch.uint8 or out.dtype != torch.float32
            or tuple(out.shape) != (B, S, S, 3) or not out.is_contiguous()):
        raise PdmkError("resize_bilinear_u8: src uint8, desc int64 [B, 8] on the host, desc_dev its device copy, out fp32 [B, S, S, 3]")
    _chk(_lib.pdmk_resize_bilinear_u8(_p(src), src.numel(), _p(desc), _p(desc_dev), B, S, _p(out), _st()),
         "pdmk_resize_bilinear_u8")


def image_resize_u8(src, desc, desc_dev, out):
    """Pillow's 8-bpc bicubic Image.resize((OW, OH)) of the packed images into out uint8 [B, OH, OW, 3]."""
    B, OH, OW = out.shape[:3]
    if (not _desc_ok(desc, desc_dev, B) or src.dtype != torch.uint8 or out.dtype != torch.uint8
            or tuple(out.shape) != (B, OH, OW, 3) or not out.is_contiguous()):
        raise PdmkError("image_resize_u8: src uint8, desc int64 [B, 8] on the host, desc_dev its device copy, out uint8 [B, OH, OW, 3]")
    _chk(_lib.pdmk_image_resize_u8(_p(src), src.numel(), _p(desc), _p(desc_dev), B, OH, OW, _p(out), _st()),
         "pdmk_image_resize_u8")


def conv2d_fwd(x, lda, w, bias, y, ldc, B, H, W, Ci, Co, kh, kw, stride, pad_h, pad_w, relu=True):
    """NHWC fp32 convolution + bias + ReLU (include/pdmk.h pdmk_conv2d_fwd).  x / y may be column slices of wider buffers
    (row strides lda / ldc in elements); w [Co, kh * kw * Ci] with k = (ky, kx, ci)."""
    Ho, Wo = (H + 2 * pad_h - kh) // stride + 1, (W + 2 * pad_w - kw) // stride + 1
    if (any(t.dtype != torch.float32 for t in (x, w, y)) or (bias is not None and (bias.dtype != torch.float32 or bias.numel() < Co))
            or w.numel() < Co * kh * kw * Ci or not w.is_contiguous() or _avail(x) < (B * H * W - 1) * lda + Ci
            or _avail(y) < (B * Ho * Wo - 1) * ldc + Co):
        raise PdmkError("conv2d_fwd: fp32 buffers, x >= [B*H*W rows of lda], y >= [B*Ho*Wo rows of ldc], w [Co, kh*kw*Ci]")
    _chk(_lib.pdmk_conv2d_fwd(_p(x), lda, _p(w), _p(bias), _p(y), ldc, B, H, W, Ci, Co, kh, kw, stride, pad_h, pad_w,
                              int(bool(relu)), _st()), "pdmk_conv2d_fwd")


def conv2d_fwd_res(x, lda, w, bias, res, ldr, y, ldc, B, H, W, Ci, Co, kh, kw, stride, pad_h, pad_w, relu=True):
    """conv2d_fwd with a residual added before the ReLU (include/pdmk.h pdmk_conv2d_fwd_res): res fp32, laid out like y with
    row stride ldr; it may be y itself (in place), no other overlap.  res None is conv2d_fwd."""
    Ho, Wo = (H + 2 * pad_h - kh) // stride + 1, (W + 2 * pad_w - kw) // stride + 1
    if (any(t.dtype != torch.float32 for t in (x, w, y)) or (bias is not None and (bias.dtype != torch.float32 or bias.numel() < Co))
            or w.numel() < Co * kh * kw * Ci or not w.is_contiguous() or _avail(x) < (B * H * W - 1) * lda + Ci
            or _avail(y) < (B * Ho * Wo - 1) * ldc + Co
            or (res is not None and (res.dtype != torch.float32 or ldr < Co or _avail(res) < (B * Ho * Wo - 1) * ldr + Co))):
        raise PdmkError("conv2d_fwd_res: fp32 buffers, x >= [B*H*W rows of lda], y / res >= [B*Ho*Wo rows of ldc / ldr], "
                        "w [Co, kh*kw*Ci]")
    _chk(_lib.pdmk_conv2d_fwd_res(_p(x), lda, _p(w), _p(bias), _p(res), ldr, _p(y), ldc, B, H, W, Ci, Co, kh, kw, stride, pad_h,
                                  pad_w, int(bool(relu)), _st()), "pdmk_conv2d_fwd_res")


def softmax_topk(logits, k, probs=None, idx=None):
    """Top-k of softmax(logits) per row (include/pdmk.h pdmk_softmax_topk): logits fp32 [B, N] with unit column stride (a
    column slice of a wider buffer is fine) -> (probs fp32 [B, k], idx int32 [B, k]); ties lower column first."""
    if (logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1 or logits.shape[0] < 1
            or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1])):
        raise PdmkError("softmax_topk: logits fp32 [B, N], unit column stride, row stride >= N")
    B, N = logits.shape
    probs = torch.empty((B, k), device=logits.device, dtype=torch.float32) if probs is None else probs
    idx = torch.empty((B, k), device=logits.device, dtype=torch.int32) if idx is None else idx
    if (probs.dtype != torch.float32 or idx.dtype != torch.int32 or tuple(probs.shape) != (B, k) or tuple(idx.shape) != (B, k)
            or not probs.is_contiguous() or not idx.is_contiguous()):
        raise PdmkError("softmax_topk: probs fp32 [B, k], idx int32 [B, k], both contiguous")
    ld = logits.stride(0) if B > 1 else max(N, logits.stride(0))
    _chk(_lib.pdmk_softmax_topk(_p(logits), ld, B, N, int(k), _p(probs), _p(idx), _st()), "pdmk_softmax_topk")
    return probs, idx


def pool2d(x, ldx, y, ldy, B, H, W, Cc, mode, stride, pad):
    """3x3 NHWC pool: mode "max" or "avg" (valid-count divisor: count_include_pad=False)."""
    Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    if (x.dtype != torch.float32 or y.dtype != torch.float32 or mode not in ("max", "avg")
            or _avail(x) < (B * H * W - 1) * ldx + Cc or _avail(y) < (B * Ho * Wo - 1) * ldy + Cc):
        raise PdmkError("pool2d: fp32 buffers, x >= [B*H*W rows of ldx], y >= [B*Ho*Wo rows of ldy], mode max / avg")
    _chk(_lib.pdmk_pool2d(_p(x), ldx, _p(y), ldy, B, H, W, Cc, 1 if mode == "avg" else 0, stride, pad, _st()), "pdmk_pool2d")


def global_avgpool(x, ldx, y, B, HW, Cc):
    if (x.dtype != torch.float32 or y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != B * Cc
            or _avail(x) < (B * HW - 1) * ldx + Cc):
        raise PdmkError("global_avgpool: x fp32 >= [B*HW rows of ldx], y fp32 contiguous [B, C]")
    _chk(_lib.pdmk_global_avgpool(_p(x), ldx, _p(y), B, HW, Cc, _st()), "pdmk_global_avgpool")


def fid_accumulate(x, total, outer):
    """total [D] += column sums, outer [D, D] += x^T x (upper-triangle 64 x 64 tiles) in fp64 on the device; x fp32 [B, D]."""
    B, D = x.shape
    if (x.dtype != torch.float32 or x.stride(1) != 1 or total.dtype != torch.float64 or outer.dtype != torch.float64
            or tuple(total.shape) != (D,) or tuple(outer.shape) != (D, D) or not total.is_contiguous()
            or not outer.is_contiguous()):
        raise PdmkError("fid_accumulate: x fp32 [B, D], total fp64 [D], outer fp64 [D, D] contiguous")
    _chk(_lib.pdmk_fid_accumulate(_p(x), x.stride(0), B, D, _p(total), _p(outer), _st()), "pdmk_fid_accumulate")


def relu_pool(x, ldx, y, ldy, B, H, W, Cc, pool):
    """y = max(x, 0) (pool 0), then a 2 x 2 stride-2 max pool with floor sizes (pool 2); NHWC fp32, strided rows."""
    Ho, Wo = (H // 2, W // 2) if pool == 2 else (H, W)
    if (x.dtype != torch.float32 or y.dtype != torch.float32 or min(B, H, W, Cc) < 1
            or _avail(x) < (B * H * W - 1) * ldx + Cc or _avail(y) < (B * Ho * Wo - 1) * ldy + Cc):
        raise PdmkError("relu_pool: fp32 buffers, x >= [B*H*W rows of ldx], y >= [B*Ho*Wo rows of ldy]")
    _chk(_lib.pdmk_relu_pool(_p(x), ldx, _p(y), ldy, B, H, W, Cc, int(pool), _st()), "pdmk_relu_pool")


def lpips_layer(f0, f1, ld, w, out, B, HW, Cc):
    """out[b] += one LPIPS layer of the pair of maps f0, f1 ([B, HW, ld] fp32, C channels), w fp32 [C], out fp64 [B]."""
    if (f0.dtype != torch.float32 or f1.dtype != torch.float32 or w.dtype != torch.float32 or out.dtype != torch.float64
            or min(B, HW, Cc) < 1 or w.numel() < Cc or not w.is_contiguous() or out.numel() < B or not out.is_contiguous()
            or min(_avail(f0), _avail(f1)) < (B * HW - 1) * ld + Cc):
        raise PdmkError("lpips_layer: f0 / f1 fp32 >= [B*HW rows of ld], w fp32 [C], out fp64 [B] contiguous")
    _chk(_lib.pdmk_lpips_layer(_p(f0), _p(f1), ld, _p(w), _p(out), B, HW, Cc, _st()), "pdmk_lpips_layer")


def gram_workspace_elems(B, HW, Cc):
    n = _lib.pdmk_gram_workspace_elems(B, HW, Cc)
    if n < 0:
        raise PdmkError(f"pdmk_gram_workspace_elems({B}, {HW}, {Cc}): sizes out of range")
    return n


def gram_pair(f0, f1, ld, B, HW, Cc, ws, style_out, content_out=None):
    """style_out[b] += mean((G_0 - G_1)^2), content_out[b] += mean((f0 - f1)^2) (None: not taken); maps [B, HW, ld] fp32,
    outputs fp64 [B], ws fp32 scratch of gram_workspace_elems(B, HW, C) elements."""
    if (f0.dtype != torch.float32 or f1.dtype != torch.float32 or ws.dtype != torch.float32 or not ws.is_contiguous()
            or min(B, HW, Cc) < 1 or min(_avail(f0), _avail(f1)) < (B * HW - 1) * ld + Cc
            or any(o is not None and (o.dtype != torch.float64 or o.numel() < B or not o.is_contiguous())
                   for o in (style_out, content_out)) or style_out is None):
        raise PdmkError("gram_pair: f0 / f1 fp32 >= [B*HW rows of ld], ws fp32, style_out / content_out fp64 [B] contiguous")
    _chk(_lib.pdmk_gram_pair(_p(f0), _p(f1), ld, B, HW, Cc, _p(ws), ws.numel(), _p(style_out), _p(content_out), _st()),
         "pdmk_gram_pair")


def softmax_rows(s, p, rows, cols, lds, ldp):
    """p[r, :cols] = softmax(s[r, :cols]) for fp32 scores s; p in the compute dtype."""
    _chk(_lib.pdmk_softmax_rows(_p(s), _p(p), rows, cols, lds, ldp, dt(p), _st()), "pdmk_softmax_rows")


def latent_sample(moments, eps, latents, B, Cc, HW, ld, scale):
    _chk(_lib.pdmk_latent_sample(_p(moments), ld, _p(eps), _p(latents), B, Cc, HW, float(scale), dt(moments), _st()),
         "pdmk_latent_sample")


def nhwc_to_nchw(src, dst, B, Cc, HW, ld):
    _chk(_lib.pdmk_nhwc_to_nchw(_p(src), _p(dst), B, Cc, HW, ld, dt(src), _st()), "pdmk_nhwc_to_nchw")


def mse_fwd(a, b, w, out, slot, B, rows_per_b, cols, lda, ldb, scale):
    _chk(_lib.pdmk_mse_fwd(_p(a), dt(a), _p(b), dt(b), _p(w), _p(out), slot, B, rows_per_b, cols, lda, ldb,
                           float(scale), _st()), "pdmk_mse_fwd")


def mse_bwd(a, b, w, da, B, rows_per_b, cols, lda, ldb, ldda, gscale, accumulate):
    _chk(_lib.pdmk_mse_bwd(_p(a), dt(a), _p(b), dt(b), _p(w), _p(da), B, rows_per_b, cols, lda, ldb, ldda,
                           float(gscale), int(accumulate), _st()), "pdmk_mse_bwd")


def mse_fwd_bwd(a, b, w, out, slot, da, B, rows_per_b, cols, lda, ldb, ldda, scale, gscale, accumulate):
    """Loss value (out[slot] +=, skipped when out is None) and gradient seed (da, skipped when None) in one vectorised pass;
    falls back to the two scalar kernels when the shape is not 16-byte friendly."""
    ok = cols % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and (da is None or da.data_ptr() % 16 == 0)
    va, vb = (8 if a.dtype == torch.bfloat16 else 4), (8 if b.dtype == torch.bfloat16 else 4)
    ok = ok and lda % va == 0 and ldb % vb == 0 and (da is None or ldda % va == 0)
    if ok:
        _chk(_lib.pdmk_mse_fwd_bwd(_p(a), dt(a), _p(b), dt(b), _p(w), _p(out), slot, _p(da), B, rows_per_b, cols, lda, ldb,
                                   ldda, float(scale), float(gscale), int(accumulate), _st()), "pdmk_mse_fwd_bwd")
        return
    if out is not None:
        mse_fwd(a, b, w, out, slot, B, rows_per_b, cols, lda, ldb, scale)
    if da is not None:
        mse_bwd(a, b, w, da, B, rows_per_b, cols, lda, ldb, ldda, gscale, accumulate)


def axpby(x, y, alpha, beta):
    _chk(_lib.pdmk_axpby(_p(x), _p(y), float(alpha), float(beta), x.numel(), dt(x), _st()), "pdmk_axpby")


def adamw(p, g, m, v, n, lr, b1, b2, eps, wd, bias_corr, grad_scale, zero_grad, w_bf16=None):
    _chk(_lib.pdmk_adamw(_p(p), _p(g), _p(m), _p(v), n, _p(lr), b1, b2, eps, wd, _p(bias_corr), grad_scale,
                         int(zero_grad), _p(w_bf16), _st()), "pdmk_adamw")


ADAMW_ROW = 8192       # elements one workgroup of pdmk_adamw_segments works through (a segment is cut into rows of this size)


class AdamwTable:
    """Segments [(arena offset, length)] as the device table of pdmk_adamw_segments.  The compact moment offsets follow the
    segments in the given order; long segments are cut into rows of ADAMW_ROW elements (one workgroup each).  `extent` (one
    past the last arena element a row touches) and `compact` (the moments' length) are what adamw_segments checks the
    buffers against."""

    def __init__(self, segments, device, row=ADAMW_ROW):
        import numpy as np
        segments = [(int(o), int(n)) for o, n in segments]
        if not segments or row <= 0 or row % 4:
            raise PdmkError("adamw_segments: no segments")
        end = -1
        for o, n in sorted(segments):
            if o < 0 or n <= 0 or (o | n) & 3 or o < end:
                raise PdmkError(f"adamw_segments: segment ({o}, {n}) is not a positive multiple of 4 elements at a multiple of "
                                f"4, or overlaps its neighbour")
            end = o + n
        recs, moff = [], 0
        for o, n in segments:
            starts = np.arange(0, n, row, dtype=np.int64)
            recs.append(np.stack([o + starts, moff + starts, np.minimum(row, n - starts)], 1))
            moff += n
        tab = np.ascontiguousarray(np.concatenate(recs, 0))
        self.segments, self.nrows, self.extent, self.compact = segments, int(tab.shape[0]), end, moff
        self.dev = torch.from_numpy(tab).to(device)


def adamw_segments(p, g, m, v, table, lr, b1, b2, eps, wd, bias_corr, grad_scale, zero_grad, w_bf16=None):
    """pdmk_adamw on the arena elements an AdamwTable names; m / v are compact (table.compact elements)."""
    if (not isinstance(table, AdamwTable) or any(t.dtype != torch.float32 or not t.is_contiguous() for t in (p, g, m, v)) or p.numel() < table.extent
            or g.numel() < table.extent or m.numel() < table.compact or v.numel() < table.compact
            or (w_bf16 is not None and (w_bf16.dtype != torch.bfloat16 or w_bf16.numel() < table.extent))
            or table.dev.device != p.device):
        raise PdmkError("adamw_segments: inconsistent buffers")
    _chk(_lib.pdmk_adamw_segments(_p(p), _p(g), _p(m), _p(v), _p(table.dev), table.nrows, _p(lr), b1, b2, eps, wd,
                                  _p(bias_corr), grad_scale, int(zero_grad), _p(w_bf16), _st()), "pdmk_adamw_segments")


def esd_head(pred, e_p, e_n, e_f, ng, out, slot, dpred, rows, cols, ldp, lde, lddp, scale, gscale):
    """ESD's loss and gradient seed in one pass (include/pdmk.h pdmk_esd_head): out[slot] += scale * sum (pred - tgt)^2 with
    tgt = e_f - ng (e_p - e_n) in fp32; dpred = gscale * (pred - tgt) over `cols`, zeros in [cols, lddp)."""
    def avail(t):
        return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
    ts = (pred, e_p, e_n, e_f) + (() if dpred is None else (dpred,))
    if (any(t.dtype != pred.dtype for t in ts) or rows <= 0 or cols <= 0 or ldp < cols or lde < cols
            or avail(pred) < (rows - 1) * ldp + cols or any(avail(t) < (rows - 1) * lde + cols for t in (e_p, e_n, e_f))
            or (dpred is not None and (lddp < cols or avail(dpred) < rows * lddp))
            or (out is not None and (out.dtype != torch.float64 or not 0 <= slot < out.numel()))):
        raise PdmkError("esd_head: inconsistent buffers")
    _chk(_lib.pdmk_esd_head(_p(pred), _p(e_p), _p(e_n), _p(e_f), float(ng), _p(out), slot, _p(dpred), rows, cols, ldp, lde,
                            lddp, float(scale), float(gscale), dt(pred), _st()), "pdmk_esd_head")


def transpose_tiles(src, dst, table, ntiles):
    _chk(_lib.pdmk_transpose_tiles(_p(src), _p(dst), _p(table), ntiles, dt(src), _st()), "pdmk_transpose_tiles")


def conv_up2_supported(B, H, W, Ci, Co, dtype):
    """True when the library serves nearest-x2 upsample + 3x3 conv of a [B, H, W, Ci] image as four 2x2 phase convs."""
    return dtype == torch.bfloat16 and bool(_lib.pdmk_conv_up2_supported(B, H, W, Ci, Co, BF16))


def up2_pack_weights(w3, wp, wpt, Co, Ci):
    _chk(_lib.pdmk_up2_pack_weights(_p(w3), _p(wp), _p(wpt), Co, Ci, dt(wp), _st()), "pdmk_up2_pack_weights")


def up2_combine_wgrad(dwp, dw3, Co, Ci):
    _chk(_lib.pdmk_up2_combine_wgrad(_p(dwp), _p(dw3), Co, Ci, _st()), "pdmk_up2_combine_wgrad")


def sumsq(x, n, out, slot):
    _chk(_lib.pdmk_sumsq(_p(x), n, _p(out), slot, _st()), "pdmk_sumsq")


# ---- ConceptPrune (pdmk.h "ConceptPrune")
WANDA_MAX_F = 5120


def rownorm_colsq(x, acc, M=None, F=None, ld=None):
    """acc[F] (fp32) += the squared column norms of the row-normalised x [M, F] (f32 / bf16, row stride ld)."""
    M = x.shape[0] if M is None else M
    F = x.shape[1] if F is None else F
    ld = x.stride(0) if ld is None else ld
    if acc.dtype != torch.float32 or acc.numel() < F or not acc.is_contiguous():
        raise PdmkError(f"rownorm_colsq: acc must be contiguous fp32 with at least F = {F} elements")
    ws = part_ws(x.device, _lib.pdmk_rownorm_colsq_workspace_elems(M, F))
    _chk(_lib.pdmk_rownorm_colsq(_p(x), dt(x), M, F, ld, _p(acc), _p(ws), ws.numel(), _st()), "pdmk_rownorm_colsq")


def wanda_count(w, n_base, n_target, k, count, O=None, F=None, ldw=None):
    """count[O, F] (int32) += over the T rows of n_base / n_target (fp32 [T, F]): f among the k largest |w[o]| * n_target[t] of
    row o (ties in ascending f) and |w[o, f]| * n_target[t, f] > |w[o, f]| * n_base[t, f]."""
    O = w.shape[0] if O is None else O
    F = w.shape[1] if F is None else F
    ldw = w.stride(0) if ldw is None else ldw
    if F > WANDA_MAX_F:
        raise PdmkError(f"wanda_count: F = {F} is wider than the {WANDA_MAX_F} columns the selection kernel keeps on chip")
    T = n_base.shape[0]
    for n in (n_base, n_target):
        if n.dtype != torch.float32 or tuple(n.shape) != (T, F) or not n.is_contiguous():
            raise PdmkError(f"wanda_count: norms must be contiguous fp32 [T, {F}], got {tuple(n.shape)} {n.dtype}")
    if count.dtype != torch.int32 or tuple(count.shape) != (O, F) or not count.is_contiguous():
        raise PdmkError(f"wanda_count: count must be contiguous int32 [{O}, {F}]")
    _chk(_lib.pdmk_wanda_count(_p(w), dt(w), O, F, ldw, _p(n_base), _p(n_target), T, int(k), _p(count), _st()),
         "pdmk_wanda_count")


def wanda_apply(w, count, threshold, O=None, F=None, ldw=None):
    """w[o, f] = 0 where float(count[o, f]) > threshold (w: f32 / bf16 [O, F] view with row stride ldw)."""
    O = w.shape[0] if O is None else O
    F = w.shape[1] if F is None else F
    ldw = w.stride(0) if ldw is None else ldw
    if count.dtype != torch.int32 or tuple(count.shape) != (O, F) or not count.is_contiguous():
        raise PdmkError(f"wanda_apply: count must be contiguous int32 [{O}, {F}]")
    _chk(_lib.pdmk_wanda_apply(_p(w), dt(w), O, F, ldw, _p(count), float(threshold), _st()), "pdmk_wanda_apply")


def mask_row_words(F):
    """32-bit words of one weight row's mask bits (bit f & 31 of word f >> 5)."""
    return (int(F) + 31) // 32


def wanda_select(w, n_base, n_target, k, bits, O=None, F=None, ldw=None):
    """wanda_count's selection as bits: bits [T, >= O * row_words] (int32, unit word stride, any row stride) - bit f & 31 of
    bits[t, o * row_words + (f >> 5)] is set where wanda_count would add one at timestep t.  The O * row_words words of every t
    are overwritten, the others are not touched."""
    O = w.shape[0] if O is None else O
    F = w.shape[1] if F is None else F
    ldw = w.stride(0) if ldw is None else ldw
    if F > WANDA_MAX_F:
        raise PdmkError(f"wanda_select: F = {F} is wider than the {WANDA_MAX_F} columns the selection kernel keeps on chip")
    T = n_base.shape[0]
    for n in (n_base, n_target):
        if n.dtype != torch.float32 or tuple(n.shape) != (T, F) or not n.is_contiguous():
            raise PdmkError(f"wanda_select: norms must be contiguous fp32 [T, {F}], got {tuple(n.shape)} {n.dtype}")
    words = O * mask_row_words(F)
    if (bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[0] != T or bits.shape[1] < words or bits.stride(1) != 1
            or bits.stride(0) < words):
        raise PdmkError(f"wanda_select: bits must be int32 [{T}, >= {words}] with unit word stride")
    _chk(_lib.pdmk_wanda_select(_p(w), dt(w), O, F, ldw, _p(n_base), _p(n_target), T, int(k), _p(bits), bits.stride(0), _st()),
         "pdmk_wanda_select")


MASK_PIECE = 16384     # elements one workgroup of pdmk_masked_weights works through (a layer is cut into row blocks of about this)


class MaskTable:
    """Layers [(dst element offset, O, F, ld)] as the device table of pdmk_masked_weights.  The pristine copy `src` is compact:
    layer after layer in the given order, each O * ld elements (rounded up to 8, so every layer starts 16-byte aligned); so are
    the mask words of one timestep, each layer O * row_words.  `layers` keeps (dst_off, src_off, bits_off, O, F, ld) per layer;
    `extent` (one past the last dst element a layer owns), `src_elems` and `words` are what masked_weights checks the buffers
    against.  A layer is cut into blocks of whole weight rows of about `piece` elements, one workgroup each."""

    def __init__(self, layers, device, piece=MASK_PIECE):
        import numpy as np
        rec = np.dtype([("dst", "<i8"), ("src", "<i8"), ("bits", "<i8"), ("O", "<i4"), ("F", "<i4"), ("ld", "<i4"), ("pad", "<i4")])
        if not layers or piece <= 0:
            raise PdmkError("masked_weights: no layers")
        self.layers, rows, soff, boff, end = [], [], 0, 0, 0
        for d, O, F, ld in layers:
            d, O, F, ld = int(d), int(O), int(F), int(ld)
            if d < 0 or O <= 0 or F <= 0 or ld < F:
                raise PdmkError(f"masked_weights: layer ({d}, {O}, {F}, {ld})")
            rw = mask_row_words(F)
            self.layers.append((d, soff, boff, O, F, ld))
            per = max(1, piece // F)
            for o0 in range(0, O, per):
                rows.append((d + o0 * ld, soff + o0 * ld, boff + o0 * rw, min(per, O - o0), F, ld, 0))
            soff += (O * ld + 7) // 8 * 8
            boff += O * rw
            end = max(end, d + O * ld)
        tab = np.array(rows, dtype=rec)
        self.nrows, self.extent, self.src_elems, self.words = len(rows), end, soff, boff
        self.dev = torch.frombuffer(bytearray(tab.tobytes()), dtype=torch.uint8).to(device)


def masked_weights(dst, src, table, bits=None, slot=-1, state=None, repeat_first=False):
    """dst = src * (1 - mask[slot]) on the layers a MaskTable names, one launch (include/pdmk.h pdmk_masked_weights).  bits: int32
    [T, >= table.words] or None (the unmasked weights); slot: the host value, or with `state` (int32 device tensor) the U-Net
    call number state[0], mapped through repeat_first.  A slot outside [0, T) writes the unmasked weights."""
    if (not isinstance(table, MaskTable) or dst.dtype != src.dtype or not dst.is_contiguous() or not src.is_contiguous()
            or dst.numel() < table.extent or src.numel() < table.src_elems or table.dev.device != dst.device
            or src.device != dst.device):
        raise PdmkError("masked_weights: inconsistent buffers")
    T, stride = 0, 0
    if bits is not None:
        if (bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[1] < table.words or bits.stride(1) != 1
                or bits.stride(0) < table.words or bits.device != dst.device):
            raise PdmkError(f"masked_weights: bits must be int32 [T, >= {table.words}] with unit word stride on the weights' device")
        T, stride = bits.shape[0], bits.stride(0)
    if state is not None and (state.dtype != torch.int32 or state.numel() < 1 or state.device != dst.device):
        raise PdmkError("masked_weights: state must be an int32 tensor on the weights' device")
    _chk(_lib.pdmk_masked_weights(_p(dst), _p(src), dt(dst), _p(table.dev), table.nrows, _p(bits), stride, T, int(slot),
                                  _p(state), int(bool(repeat_first)), _st()), "pdmk_masked_weights")


# ---- UCE (pdmk.h "UCE")
SPD_MAX_N = 4096


def _f64_matrix(t, n, name, what):
    """t: fp64 [n, >= n] view with unit column stride; returns its row stride."""
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != n or t.shape[1] != n or t.stride(1) != 1 or t.stride(0) < n:
        raise PdmkError(f"{name}: {what} must be an fp64 [{n}, {n}] view with contiguous rows")
    return t.stride(0)


def spd_system(g_a, s_a, g_b, s_b, lam, A):
    """A = lam I + s_a sym(g_a) + s_b sym(g_b) (g_b may be None); g: the `outer` of fid_accumulate, A fp64 [n, n] (row stride >= n)."""
    n = g_a.shape[0]
    for g in (g_a, g_b):
        if g is not None and (g.dtype != torch.float64 or tuple(g.shape) != (n, n) or not g.is_contiguous()):
            raise PdmkError(f"spd_system: the Gram matrices must be contiguous fp64 [{n}, {n}]")
    if not 1 <= n <= SPD_MAX_N:
        raise PdmkError(f"spd_system: n = {n} outside 1 .. {SPD_MAX_N}")
    lda = _f64_matrix(A, n, "spd_system", "A")
    _chk(_lib.pdmk_spd_system_f64(_p(g_a), float(s_a), _p(g_b), float(s_b), float(lam), _p(A), n, lda, _st()),
         "pdmk_spd_system_f64")


def pair_gram(z, scale, lam, A):
    """A = lam I + scale sum_p (z[2p] - z[2p+1]) (z[2p] - z[2p+1])^T in fp64 (include/pdmk.h pdmk_pair_gram_f64): z fp32
    [2 * npairs, d] and A fp64 [d, d], views with contiguous rows."""
    if z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] < 2 or z.shape[0] % 2 or z.stride(1) != 1 or z.stride(0) < z.shape[1]:
        raise PdmkError("pair_gram: z must be an fp32 [2 * npairs, d] view with contiguous rows")
    d = z.shape[1]
    if not 1 <= d <= SPD_MAX_N:
        raise PdmkError(f"pair_gram: d = {d} outside 1 .. {SPD_MAX_N}")
    lda = _f64_matrix(A, d, "pair_gram", "A")
    _chk(_lib.pdmk_pair_gram_f64(_p(z), z.stride(0), z.shape[0] // 2, d, float(scale), float(lam), _p(A), lda, _st()),
         "pdmk_pair_gram_f64")


def spd_factor(A, info):
    """Cholesky A = L L^T in place (lower triangle); info: int32 [1] on the device, zeroed by the caller (0, or first bad column + 1)."""
    n = A.shape[0]
    if not 1 <= n <= SPD_MAX_N:
        raise PdmkError(f"spd_factor: n = {n} outside 1 .. {SPD_MAX_N}")
    lda = _f64_matrix(A, n, "spd_factor", "A")
    if info.dtype != torch.int32 or info.numel() != 1 or info.device != A.device:
        raise PdmkError("spd_factor: info must be one int32 on the matrix' device")
    _chk(_lib.pdmk_spd_factor_f64(_p(A), n, lda, _p(info), _st()), "pdmk_spd_factor_f64")


def spd_solve(L, B, X, X64=None):
    """X = B (L L^T)^-1: B, X fp32 [m, n] and X64 fp64 [m, n] (optional) views with contiguous rows."""
    n = L.shape[0]
    ldl = _f64_matrix(L, n, "spd_solve", "L")
    m = B.shape[0]
    for t, dtype, name in ((B, torch.float32, "B"), (X, torch.float32, "X"), (X64, torch.float64, "X64")):
        if t is not None and (t.dtype != dtype or t.dim() != 2 or tuple(t.shape) != (m, n) or t.stride(1) != 1 or t.stride(0) < n):
            raise PdmkError(f"spd_solve: {name} must be a {dtype} [{m}, {n}] view with contiguous rows")
    if m < 1:
        raise PdmkError("spd_solve: m >= 1")
    ws = torch.empty(_lib.pdmk_spd_workspace_elems(n, m), device=L.device, dtype=torch.float64)
    _chk(_lib.pdmk_spd_solve_f64(_p(L), n, ldl, _p(B), m, B.stride(0), _p(X), X.stride(0), _p(X64),
                                 0 if X64 is None else X64.stride(0), _p(ws), ws.numel(), _st()), "pdmk_spd_solve_f64")


def uce_delta(O, N, D, row_seg, col_seg, technique):
    """D = N - O (technique 0) or N - (1 + <O, N> / <O, O>) O per (pair, projection) block (technique 1) on fp32 [m, ld]
    matrices of one layout; row_seg / col_seg: host lists of P + 1 first rows / Q + 1 first columns.  Rows from row_seg[-1] on
    are zeroed."""
    m, ld = O.shape[0], O.stride(0)
    for t in (O, N, D):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != O.shape or t.stride() != O.stride() or t.stride(1) != 1:
            raise PdmkError("uce_delta: O, N, D must be fp32 [m, w] views of one shape and row stride")
    row_seg, col_seg = [int(v) for v in row_seg], [int(v) for v in col_seg]
    P, Q = len(row_seg) - 1, len(col_seg) - 1
    if (P < 1 or Q < 1 or P > 65534 or technique not in (0, 1) or any(b < a for a, b in zip(row_seg, row_seg[1:]))
            or any(b < a for a, b in zip(col_seg, col_seg[1:])) or row_seg[0] < 0 or col_seg[0] < 0 or row_seg[-1] > m
            or col_seg[-1] > O.shape[1]):
        raise PdmkError(f"uce_delta: segments must ascend inside [0, {m}] x [0, {O.shape[1]}], technique 0 / 1")
    seg = torch.tensor(row_seg + col_seg, dtype=torch.int32).to(O.device)
    ws = torch.empty(2 * P * Q, device=O.device, dtype=torch.float64) if technique == 1 else None
    _chk(_lib.pdmk_uce_delta(_p(O), _p(N), _p(D), m, ld, _p(seg), P, _p(seg[P + 1:]), Q, int(technique), _p(ws), _st()),
         "pdmk_uce_delta")


DEBIAS_MAX_ATTR = 8


def uce_debias_delta(O, U, D, w, row_seg, col_seg):
    """D = sum_j c_j U[j] per (pair, projection) block with the debiasing recurrence's c_j (include/pdmk.h
    pdmk_uce_debias_delta): O, D fp32 [m, w] views of one row stride, U fp32 [A, m, w] with that row stride and attribute stride
    m * ld, w fp32 [P, A] on the device; row_seg / col_seg: host lists of P + 1 first rows / Q + 1 first columns.  Rows from
    row_seg[-1] on are zeroed."""
    m, ld = O.shape[0], O.stride(0)
    for t in (O, D):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != O.shape or t.stride() != O.stride() or t.stride(1) != 1:
            raise PdmkError("uce_debias_delta: O, D must be fp32 [m, w] views of one shape and row stride")
    A = U.shape[0] if U.dim() == 3 else 0
    if (U.dtype != torch.float32 or U.dim() != 3 or not 1 <= A <= DEBIAS_MAX_ATTR or tuple(U.shape[1:]) != tuple(O.shape)
            or U.stride() != (m * ld, ld, 1)):
        raise PdmkError(f"uce_debias_delta: U must be fp32 [A, m, w] with strides (m ld, ld, 1), 1 <= A <= {DEBIAS_MAX_ATTR}")
    row_seg, col_seg = [int(v) for v in row_seg], [int(v) for v in col_seg]
    P, Q = len(row_seg) - 1, len(col_seg) - 1
    if (P < 1 or Q < 1 or P > 65534 or any(b < a for a, b in zip(row_seg, row_seg[1:]))
            or any(b < a for a, b in zip(col_seg, col_seg[1:])) or row_seg[0] < 0 or col_seg[0] < 0 or row_seg[-1] > m
            or col_seg[-1] > O.shape[1]):
        raise PdmkError(f"uce_debias_delta: segments must ascend inside [0, {m}] x [0, {O.shape[1]}]")
    if w.dtype != torch.float32 or tuple(w.shape) != (P, A) or not w.is_contiguous() or w.device != O.device:
        raise PdmkError(f"uce_debias_delta: w must be contiguous fp32 [{P}, {A}] on the matrices' device")
    seg = torch.tensor(row_seg + col_seg, dtype=torch.int32).to(O.device)
    ws = torch.empty(P * Q * A, device=O.device, dtype=torch.float64)
    _chk(_lib.pdmk_uce_debias_delta(_p(O), _p(U), _p(D), m, ld, A, _p(w), _p(seg), P, _p(seg[P + 1:]), Q, _p(ws), ws.numel(),
                                    _st()), "pdmk_uce_debias_delta")


ZEROSHOT_MAX_CLASSES = 64


def zeroshot_head(img, txt, scale, probs=None, mask=None, group=None, hits=None):
    """CLIP zero-shot head (include/pdmk.h pdmk_zeroshot_head): img fp32 [B, D], txt fp32 [A, D] (unit column stride, a row
    stride >= D), scale the host's fp32 exp(logit_scale) -> (probs fp32 [B, A], mask int32 [B, A]).  hits int32 [G, A]
    (contiguous, accumulated into) and group int32 [B] on the device (None: every row counts in hits[0]) are optional."""
    def rows(t):
        return t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]
    if not rows(img) or not rows(txt) or img.shape[1] != txt.shape[1] or txt.device != img.device:
        raise PdmkError("zeroshot_head: img fp32 [B, D], txt fp32 [A, D], unit column stride, row stride >= D, one device")
    (B, D), A = img.shape, txt.shape[0]
    if not (1 <= B <= 65535 and 1 <= A <= ZEROSHOT_MAX_CLASSES and 1 <= D <= 4096):
        raise PdmkError(f"zeroshot_head: B = {B}, A = {A}, D = {D} outside 1 .. 65535, 1 .. {ZEROSHOT_MAX_CLASSES}, 1 .. 4096")
    probs = torch.empty((B, A), device=img.device, dtype=torch.float32) if probs is None else probs
    mask = torch.empty((B, A), device=img.device, dtype=torch.int32) if mask is None else mask
    if (probs.dtype != torch.float32 or mask.dtype != torch.int32 or tuple(probs.shape) != (B, A) or tuple(mask.shape) != (B, A)
            or not probs.is_contiguous() or not mask.is_contiguous()):
        raise PdmkError("zeroshot_head: probs fp32 [B, A], mask int32 [B, A], both contiguous")
    G = 0
    if hits is not None:
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != A or not hits.is_contiguous() or hits.shape[0] < 1:
            raise PdmkError(f"zeroshot_head: hits must be contiguous int32 [G, {A}]")
        G = hits.shape[0]
    if group is not None and (hits is None or group.dtype != torch.int32 or tuple(group.shape) != (B,) or not group.is_contiguous()
                              or group.device != img.device):
        raise PdmkError(f"zeroshot_head: group must be contiguous int32 [{B}] on the device, with hits")
    _chk(_lib.pdmk_zeroshot_head(_p(img), img.stride(0), _p(txt), txt.stride(0), B, A, D, float(scale), _p(probs), _p(mask),
                                 _p(group), _p(hits), G, _st()), "pdmk_zeroshot_head")
    return probs, mask
