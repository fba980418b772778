"""ctypes binding of libsaspa_hip.so (include/saspa_hip.h).  No fallback of any kind."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SASPA_HIP_LIB: load another build of the same ABI (the `make ABLATION=1` diagnostics library of tools/pp_clock.py ...)
LIB_PATH = os.environ.get("SASPA_HIP_LIB") or os.path.join(_HERE, "libsaspa_hip.so")
# the fp16 build of the 16-bit kernels (csrc/Makefile, -DSASPA_HALF_F16): opened only when an fp16 tensor reaches ops
F16_LIB_PATH = os.path.join(_HERE, "libsaspa_hip_f16.so")

SASPA_BF16, SASPA_F32, SASPA_F32X3 = 0, 1, 2
SASPA_F16 = 3                                              # libsaspa_hip_f16.so only
SASPA_EINVAL, SASPA_EALIGN, SASPA_ERANGE = -1, -2, -3      # include/saspa_hip.h
DECODE_MAX_D, DECODE_MAX_NK, DECODE_MAX_GROUP = 128, 1024, 8  # SASPA_DECODE_MAX_*
RMSNORM_MAX_C, RELBIAS_MAX_ROWS, SAMPLE_MAX_TOPK = 8192, 1024, 64   # SASPA_RMSNORM_MAX_C / SASPA_RELBIAS_MAX_ROWS / SASPA_SAMPLE_MAX_TOPK
LPIPS_MAX_C, LPIPS_MAX_BLOCKS = 512, 64                    # SASPA_LPIPS_MAX_C / SASPA_LPIPS_MAX_BLOCKS
CLASS_HEAD_MAX_D, CLASS_HEAD_MAX_C = 2048, 4096            # SASPA_CLASS_HEAD_MAX_D / SASPA_CLASS_HEAD_MAX_C
FILTER_RECORD_MAX_P, FILTER_RECORD_FIELDS = 64, 8          # SASPA_FILTER_RECORD_MAX_P; fp32 per record
ERRORS = {-1: "SASPA_EINVAL (null pointer / bad size)", -2: "SASPA_EALIGN (16-byte alignment / channel multiple)",
          -3: "SASPA_ERANGE (unsupported shape)"}


class GemmParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("a0", C.c_void_p), ("a1", C.c_void_p), ("c0", C.c_int), ("c1", C.c_int),
        ("lda0", C.c_int), ("lda1", C.c_int), ("batch", C.c_int), ("hin", C.c_int), ("win", C.c_int),
        ("hout", C.c_int), ("wout", C.c_int), ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int),
        ("pad", C.c_int), ("upsample", C.c_int), ("w", C.c_void_p), ("ldw", C.c_int), ("M", C.c_int),
        ("N", C.c_int), ("K", C.c_int), ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("ldrv", C.c_int),
        ("residual", C.c_void_p), ("ldr", C.c_int), ("alpha", C.c_float), ("act", C.c_int),
        ("out", C.c_void_p), ("ldo", C.c_int), ("nb1", C.c_int), ("nb2", C.c_int),
        ("sa1", C.c_longlong), ("sa2", C.c_longlong), ("sw1", C.c_longlong), ("sw2", C.c_longlong),
        ("so1", C.c_longlong), ("so2", C.c_longlong), ("ksplit", C.c_int), ("workspace", C.c_void_p),
        ("variant", C.c_int), ("korder", C.c_int), ("gn_stats", C.c_void_p), ("gn_unit", C.c_int),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("out_t", C.c_void_p), ("ldt", C.c_int),
        ("st", C.c_longlong), ("n_split", C.c_int), ("rows_per_batch", C.c_int), ("sharing", C.c_int), ("defer_reduce", C.c_int),
        ("w_split", C.c_int),                                                                     # ABI 20
    ]


class XattnBlockParams(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int), ("residual", C.c_void_p), ("ldr", C.c_int), ("M", C.c_longlong),
        ("rows_per_sample", C.c_int), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float),
        ("w", C.c_void_p), ("ldw", C.c_int), ("bias", C.c_void_p), ("kf", C.c_void_p), ("kf_stride", C.c_longlong),
        ("vf", C.c_void_p), ("vf_stride", C.c_longlong), ("nk", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
    ]


class AttnParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int), ("sqb", C.c_longlong),
        ("k", C.c_void_p), ("ldk", C.c_int), ("skb", C.c_longlong),
        ("vt", C.c_void_p), ("ldvt", C.c_int), ("svb", C.c_longlong),
        ("o", C.c_void_p), ("ldo", C.c_int), ("sob", C.c_longlong),
        ("batch", C.c_int), ("heads", C.c_int), ("D", C.c_int), ("nq", C.c_int), ("nk", C.c_int),
        ("scale", C.c_float), ("causal", C.c_int), ("flags", C.c_int),
    ]


class GroupNormParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("x0", C.c_void_p), ("x1", C.c_void_p), ("c0", C.c_int), ("c1", C.c_int),
        ("ldx0", C.c_int), ("ldx1", C.c_int), ("batch", C.c_int), ("hw", C.c_int), ("groups", C.c_int),
        ("eps", C.c_float), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("partial", C.c_void_p),
        ("nsplit", C.c_int), ("scale_shift", C.c_void_p), ("act", C.c_int), ("y", C.c_void_p), ("ldy", C.c_int),
        ("stats0", C.c_void_p), ("stats1", C.c_void_p), ("unit", C.c_int),
    ]


class ConvGnParams(C.Structure):
    _fields_ = [
        ("gamma_beta32", C.c_void_p), ("groups", C.c_int), ("eps", C.c_float), ("act", C.c_int),
        ("stats0", C.c_void_p), ("stats1", C.c_void_p), ("unit", C.c_int), ("partial", C.c_void_p), ("nsplit", C.c_int),
    ]


class GemmF8Params(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int), ("w", C.c_void_p), ("ldw", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("sa", C.c_void_p), ("sw", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int),
        ("act", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
        ("sa_broadcast", C.c_int), ("out_fp8", C.c_int), ("out_scale", C.c_void_p), ("amax", C.c_void_p),      # ABI 20
    ]


class ConvMxParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int), ("qs", C.c_void_p), ("ldqs", C.c_int),
        ("batch", C.c_int), ("h", C.c_int), ("w", C.c_int), ("C", C.c_int),
        ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("upsample", C.c_int),
        ("w8", C.c_void_p), ("ldw", C.c_int), ("N", C.c_int), ("Kp", C.c_int),
        ("sw", C.c_void_p), ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("ldrv", C.c_int),
        ("residual", C.c_void_p), ("ldr", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
        ("gn_stats", C.c_void_p), ("gn_unit", C.c_int),
    ]


class FfBlockParams(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int), ("residual", C.c_void_p), ("ldr", C.c_int), ("M", C.c_longlong), ("F", C.c_int),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("w1", C.c_void_p), ("ldw1", C.c_int),
        ("b1", C.c_void_p), ("w2f", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int),
    ]


class DecodeAttnParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("q", C.c_void_p), ("ldq", C.c_int), ("k", C.c_void_p), ("ldk", C.c_int), ("ske", C.c_longlong),
        ("v", C.c_void_p), ("ldv", C.c_int), ("sve", C.c_longlong), ("len", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int),
        ("rows", C.c_int), ("entries", C.c_int), ("heads", C.c_int), ("d", C.c_int), ("nk", C.c_int), ("group", C.c_int),
        ("scale", C.c_float),
    ]


class AttnRelbiasParams(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("q", C.c_void_p), ("ldq", C.c_int), ("k", C.c_void_p), ("ldk", C.c_int), ("ske", C.c_longlong),
        ("v", C.c_void_p), ("ldv", C.c_int), ("sve", C.c_longlong), ("len", C.c_void_p), ("pos", C.c_void_p),
        ("bias", C.c_void_p), ("ldb", C.c_int), ("ncol", C.c_int), ("center", C.c_int), ("out", C.c_void_p), ("ldo", C.c_int),
        ("rows", C.c_int), ("entries", C.c_int), ("heads", C.c_int), ("d", C.c_int), ("nk", C.c_int), ("rows_per_entry", C.c_int),
        ("scale", C.c_float),
    ]


class HedFuseParams(C.Structure):
    _fields_ = [
        ("nmaps", C.c_int), ("n", C.c_int), ("H", C.c_int), ("W", C.c_int),
        ("map", C.c_void_p * 5), ("mh", C.c_int * 5), ("mw", C.c_int * 5), ("ld", C.c_int * 5),
        ("xofs", C.c_void_p * 5), ("xw", C.c_void_p * 5), ("yofs", C.c_void_p * 5), ("yw", C.c_void_p * 5),
        ("dst", C.c_void_p),
    ]


# every symbol include/saspa_hip.h declares: (name, restype, argtypes)
_I, _LL, _F, _P = C.c_int, C.c_longlong, C.c_float, C.c_void_p
SYMBOLS = {
    "saspa_gemm": (_I, [C.POINTER(GemmParams), _P]),
    "saspa_gemm_suggest_ksplit": (_I, [C.POINTER(GemmParams)]),
    "saspa_gemm_as_eligible": (_I, [C.POINTER(GemmParams)]),
    "saspa_gemm_as_auto": (_I, [C.POINTER(GemmParams)]),
    "saspa_gemm_which": (_I, [C.POINTER(GemmParams)]),
    "saspa_ff_block": (_I, [C.POINTER(FfBlockParams), _P]),
    "saspa_ff_block_eligible": (_I, [C.POINTER(FfBlockParams)]),
    "saspa_flash_attn_bf16": (_I, [C.POINTER(AttnParams), _P]),
    "saspa_flash_attn_which": (_I, [C.POINTER(AttnParams)]),
    "saspa_flash_attn_f32x3": (_I, [C.POINTER(AttnParams), _P]),
    "saspa_softmax_rows": (_I, [_I, _P, _LL, _I, _I, _F, _I, _I, _P]),
    "saspa_attn_wide": (_I, [_I, _P, _I, _LL, _P, _I, _LL, _P, _I, _LL, _P, _I, _LL, _I, _I, _I, _I, _F, _P]),
    "saspa_attn_wide_f32x3": (_I, [_P, _I, _LL, _P, _I, _LL, _P, _I, _LL, _P, _I, _LL, _I, _I, _I, _I, _F, _P]),
    "saspa_groupnorm_stats": (_I, [C.POINTER(GroupNormParams), _P]),
    "saspa_groupnorm_apply": (_I, [C.POINTER(GroupNormParams), _P]),
    "saspa_layernorm": (_I, [_I, _P, _I, _P, _I, _LL, _I, _P, _P, _F, _P]),
    "saspa_geglu": (_I, [_I, _P, _I, _P, _I, _LL, _I, _P]),
    "saspa_activation": (_I, [_I, _I, _P, _I, _P, _I, _LL, _I, _P]),
    "saspa_embed_tokens": (_I, [_I, _P, _I, _I, _P, _P, _I, _P, _P]),
    "saspa_embed_tokens_ctx": (_I, [_I, _P, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P]),
    "saspa_cfg_plms_step": (_I, [_I, _P, _P, _P, _P, _I, _LL, _I, _I, _F, _I, _F, C.POINTER(C.c_float), _F, _F, _P]),
    "saspa_cfg_ddim_step": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _F, _F, _F, _P]),
    "saspa_ddim_step": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _F, _F, _P]),
    "saspa_gather_row_f32": (_I, [_P, _LL, _P, _P, _LL, _P]),
    "saspa_ddim_step_dev": (_I, [_I, _P, _P, _I, _LL, _I, _I, _I, _F, _P, _P, _P]),
    "saspa_index_add": (_I, [_P, _I, _P]),
    "saspa_cfg3_ddim_step": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _F, _F, _F, _F, _P]),
    "saspa_cfg3_ddim_step_dev": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _P, _P, _P]),
    "saspa_clock_probe": (_I, [_P, _I, _P]),
    "saspa_cfg_plms_step_dev": (_I, [_I, _P, _P, _P, _P, _I, _LL, _I, _I, _F, _P, _P, _P]),
    "saspa_scale": (_I, [_I, _P, _P, _LL, _F, _P]),
    "saspa_u8_to_act": (_I, [_I, _P, _P, _LL, _P]),
    "saspa_act_to_u8": (_I, [_I, _P, _I, _P, _LL, _P]),
    "saspa_canny": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "saspa_resample_u8": (_I, [_P, _P, _LL, _I, _I, _I, _P, _P, _I, _P]),
    "saspa_u8_to_act_norm": (_I, [_I, _P, _P, _LL, _F, _F, _F, _F, _F, _F, _P]),
    "saspa_u8_luma": (_I, [_P, _P, _LL, _P]),
    "saspa_safety_decide": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _I, C.c_double, _P, _LL, _P, _P]),
    "saspa_pool2d": (_I, [_I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "saspa_signsqrt_l2norm": (_I, [_P, _LL, _P, _LL, _I, _LL, _F, _F, _P]),
    "saspa_lpips_layer": (_I, [_I, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "saspa_class_head": (_I, [_P, _I, _P, _I, _P, _F, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "saspa_filter_record": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "saspa_resize_taps_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "saspa_hed_fuse": (_I, [C.POINTER(HedFuseParams), _P]),
    "saspa_gemm_fp8": (_I, [C.POINTER(GemmF8Params), _P]),
    "saspa_gemm_fp8_geglu_mx": (_I, [C.POINTER(GemmF8Params), _P, _I, _P]),
    "saspa_gemm_mxfp8": (_I, [C.POINTER(GemmF8Params), _P, _I, _P]),
    "saspa_layernorm_quant_fp8": (_I, [_P, _I, _P, _I, _P, _LL, _I, _P, _P, _F, _P]),
    "saspa_resize_area_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "saspa_vae_sample_noise": (_I, [_I, _P, _P, _P, _P, _LL, _F, _F, _F, _P]),
    "saspa_cfg_unipc_step": (_I, [_I, _P, _P, _P, _I, _LL, _I, _I, _F, C.POINTER(C.c_float), _P, _P, _P]),
    "saspa_unipc_step": (_I, [_I, _P, _P, _P, _I, _LL, _I, _I, C.POINTER(C.c_float), _P, _P, _P]),
    "saspa_cfg_ddim_step_v": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _F, _F, _F, _P]),
    "saspa_ddim_step_v": (_I, [_I, _P, _P, _I, _LL, _I, _I, _F, _F, _F, _F, _P]),
    "saspa_ddim_step_v_dev": (_I, [_I, _P, _P, _I, _LL, _I, _I, _I, _F, _P, _P, _P]),
    "saspa_cfg_unipc_step_v": (_I, [_I, _P, _P, _P, _I, _LL, _I, _I, _F, C.POINTER(C.c_float), _P, _P, _P]),
    "saspa_unipc_step_v": (_I, [_I, _P, _P, _P, _I, _LL, _I, _I, C.POINTER(C.c_float), _P, _P, _P]),
    "saspa_xattn_block": (_I, [C.POINTER(XattnBlockParams), _P]),
    "saspa_xattn_block_bcast": (_I, [C.POINTER(XattnBlockParams), _LL, _P]),
    "saspa_groupnorm_onepass_eligible": (_I, [C.POINTER(GroupNormParams)]),
    "saspa_groupnorm_onepass": (_I, [C.POINTER(GroupNormParams), _P]),
    "saspa_splitk_groupnorm_eligible": (_I, [C.POINTER(GemmParams), C.POINTER(GroupNormParams)]),
    "saspa_splitk_groupnorm": (_I, [C.POINTER(GemmParams), C.POINTER(GroupNormParams), _P]),
    "saspa_conv3x3_halo_eligible": (_I, [C.POINTER(GemmParams), C.POINTER(ConvGnParams)]),
    "saspa_conv3x3_halo_ksplit": (_I, [C.POINTER(GemmParams), _I]),
    "saspa_conv3x3_halo": (_I, [C.POINTER(GemmParams), C.POINTER(ConvGnParams), _P]),
    "saspa_groupnorm_quant_mxfp8": (_I, [C.POINTER(GroupNormParams), _P, _I, _P, _I, _P]),
    "saspa_conv3x3_mxfp8_eligible": (_I, [C.POINTER(ConvMxParams)]),
    "saspa_conv3x3_mxfp8": (_I, [C.POINTER(ConvMxParams), _P]),
    "saspa_png_capacity": (_LL, [_I, _I, _I]),
    "saspa_png_workspace": (_LL, [_I, _I, _I, _I]),
    "saspa_png_deflate": (_I, [_P, _I, _I, _I, _I, _P, _LL, _P, _P, _LL, _P]),
    "saspa_decode_attn": (_I, [C.POINTER(DecodeAttnParams), _P]),
    "saspa_logprob_topk": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _P, _P]),
    "saspa_rmsnorm": (_I, [_I, _P, _I, _P, _I, _I, _I, _P, C.c_float, _P]),
    "saspa_attn_relbias": (_I, [C.POINTER(AttnRelbiasParams), _P]),
    "saspa_sample_topk": (_I, [_P, _I, _I, _I, C.c_float, _I, C.c_float, _P, _P, _P, _P]),
    "saspa_abi_version": (_I, []),
    "saspa_half_type": (_I, []),
    "saspa_build_arch": (C.c_char_p, []),
}

# what libsaspa_hip_f16.so exports: the entry points of the translation units the fp16 mode needs (GEMM / conv, attention, norms,
# elementwise and scheduler steps, the fused transformer-block launches); fp8 / MX / halo convs, Canny, image, filter, resize, HED and
# PNG exist in the default library only
F16_SYMBOL_NAMES = (
    "saspa_gemm", "saspa_gemm_suggest_ksplit", "saspa_gemm_as_eligible", "saspa_gemm_as_auto", "saspa_gemm_which",
    "saspa_ff_block", "saspa_ff_block_eligible", "saspa_xattn_block", "saspa_xattn_block_bcast", "saspa_flash_attn_bf16",
    "saspa_flash_attn_which", "saspa_softmax_rows", "saspa_attn_wide",
    "saspa_groupnorm_stats", "saspa_groupnorm_apply", "saspa_groupnorm_onepass_eligible", "saspa_groupnorm_onepass",
    "saspa_splitk_groupnorm_eligible", "saspa_splitk_groupnorm", "saspa_layernorm", "saspa_geglu", "saspa_activation",
    "saspa_embed_tokens", "saspa_embed_tokens_ctx", "saspa_cfg_plms_step", "saspa_cfg_plms_step_dev", "saspa_cfg_ddim_step",
    "saspa_ddim_step", "saspa_ddim_step_dev", "saspa_cfg3_ddim_step", "saspa_cfg3_ddim_step_dev", "saspa_cfg_unipc_step", "saspa_unipc_step",
    "saspa_cfg_ddim_step_v", "saspa_ddim_step_v", "saspa_ddim_step_v_dev", "saspa_cfg_unipc_step_v", "saspa_unipc_step_v",
    "saspa_vae_sample_noise", "saspa_scale", "saspa_u8_to_act", "saspa_act_to_u8", "saspa_abi_version", "saspa_half_type",
    "saspa_build_arch",
)

_lib = None
_lib_f16 = None


def load():
    """Load the HIP library; raises (never falls back) when it is missing or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the gfx950 kernels are not built. Run "
            "`make -C saspa-aug_amd/csrc` (or __graft_entry__.build()). There is no CPU fallback.")
    # torch FIRST: libsaspa_hip.so needs libamdhip64 and must bind to the HIP runtime torch ships and initialises (torch/lib), the one
    # that owns the device pointers and streams every entry point is handed.  Loaded before torch, the dynamic loader resolves the
    # dependency to /opt/rocm's copy and torch then rides on THAT runtime: launches fail with hipErrorNoDevice (100) -- seen in round 6
    # with `python __graft_entry__.py smoke` (build() loaded the library, then smoke() imported torch).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    # SASPA_HIP_LIB_LENIENT=1 (only with SASPA_HIP_LIB): same-box A/B against an OLDER build that lacks newer symbols
    lenient = bool(os.environ.get("SASPA_HIP_LIB")) and os.environ.get("SASPA_HIP_LIB_LENIENT") == "1"
    for name, (res, args) in SYMBOLS.items():
        if lenient and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def load_f16():
    """Load the fp16 library (lazily: nothing of it is opened before an fp16 tensor reaches ops); raises, never falls back."""
    global _lib_f16
    if _lib_f16 is not None:
        return _lib_f16
    if not os.path.exists(F16_LIB_PATH):
        raise RuntimeError(
            f"{F16_LIB_PATH} not found: the fp16 build of the gfx950 kernels is missing. Run `make -C saspa-aug_amd/csrc` "
            "(or __graft_entry__.build()). fp16 tensors are never routed to the bf16 library.")
    import torch  # noqa: F401      (torch FIRST, as in load(): the library must bind to the HIP runtime torch ships)
    lib = C.CDLL(F16_LIB_PATH)
    for name in F16_SYMBOL_NAMES:
        fn = getattr(lib, name)  # AttributeError if the .so does not export a symbol of its subset
        fn.restype, fn.argtypes = SYMBOLS[name]
    if lib.saspa_abi_version() != load().saspa_abi_version() or lib.saspa_half_type() != SASPA_F16:
        raise RuntimeError(f"{F16_LIB_PATH}: ABI {lib.saspa_abi_version()} / 16-bit type {lib.saspa_half_type()} is not the fp16 "
                           "build of this tree's kernels; rebuild")
    _lib_f16 = lib
    return lib


def f16_loaded():
    return _lib_f16 is not None


def check(code, what):
    if code != 0:
        msg = ERRORS.get(code, f"hipError_t {code}" if code > 0 else f"error {code}")
        raise RuntimeError(f"{what}: {msg}")
