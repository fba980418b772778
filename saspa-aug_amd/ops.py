"""Tensor-level wrappers over the C ABI (include/saspa_hip.h).

PyTorch is used for device memory and the current HIP stream only; every function here
enqueues hand-written gfx950 kernels through ctypes and does no arithmetic of its own.
Activations are channels-last ``[B, H, W, C]`` (or ``[M, C]`` token matrices) whose last
dim is contiguous; the pixel pitch (``stride(-2)``) may exceed C (views into wider
buffers, e.g. the q/k slices of a fused projection)."""
import os
import collections
import ctypes as C

import torch

from . import _lib

ACT_NONE, ACT_SILU = 0, 1
ACT_QUICK_GELU = 2  # saspa_activation only
ACT_GELU = 4        # saspa_activation only: erf GELU (BERT / Q-Former)
ACT_GEGLU = 3       # saspa_gemm only: fused GEGLU epilogue (bf16, weights packed by weights.pack_geglu)
ACT_RELU = 5        # saspa_gemm / saspa_activation: ReLU (before the residual add)
ACT_ADD_RELU = 6    # saspa_gemm only: ReLU AFTER the residual add (ResNet bottleneck)
GEMM_AUTO, GEMM_TILED, GEMM_WIDE, GEMM_WS, GEMM_AS = 0, 1, 2, 3, 4   # SaspaGemmParams.variant


# Optional launch recorder (bench.py / profiling only): called as recorder(kind, flops, call)
# and must return call()'s result.  `flops` is the ALGORITHMIC work of the launch (2*M*N*K
# for the implicit GEMM, 4*nq*nk*D per head for attention), used for the roofline figures; `meta` of a GEMM launch is
# (M, N, K, kh, stride, upsample, concat, has_residual, output columns): kh = 0 linear, kh < 0 = -(batch count) of a raw
# batched GEMM.
_RECORDER = None


def set_recorder(rec):
    global _RECORDER
    _RECORDER = rec


_IN_LAUNCH = [False]


def _launch(kind, flops, call, meta=None):
    if _RECORDER is None:
        return call()
    _IN_LAUNCH[0] = True
    try:
        return _RECORDER(kind, flops, call, meta)
    finally:
        _IN_LAUNCH[0] = False


# library entry points that launch nothing (host-side queries), and the clock probe (a sleeping wave used as a gate / clock
# sample, not work of the path): never recorded
_HOST_ONLY = ("eligible", "suggest", "ksplit", "which", "as_auto", "abi_version", "build_arch", "clock_probe",
              "capacity", "workspace")


class _RecordingLib:
    """What `_L()` hands out while a launch recorder is installed: every kernel-launching entry point that is NOT already wrapped
    by `_launch` (norms, element-wise passes, scheduler updates ...) is timed too, under its own name with zero FLOPs -- so that the
    recorder's table covers the whole step (bench.py `timed_path_check`), not only the MFMA kernels."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("saspa_") or any(t in name for t in _HOST_ONLY):
            return fn

        def wrapped(*a):
            rec = _RECORDER
            if rec is None or _IN_LAUNCH[0]:
                return fn(*a)
            _IN_LAUNCH[0] = True
            try:
                return rec(name[len("saspa_"):], 0.0, lambda: fn(*a), None)
            finally:
                _IN_LAUNCH[0] = False
        return wrapped


def is_half(t):
    """The 16-bit compute type: bf16 (libsaspa_hip.so) or fp16 (libsaspa_hip_f16.so) -- the same kernels, layouts and fused paths."""
    return t.dtype == torch.bfloat16 or t.dtype == torch.float16


def _L(t=None):
    """The library that serves the activation tensor `t` (or the dtype code of a filled-in parameter struct): fp16 goes to the fp16
    build, everything else -- fp32 always -- to the default library."""
    f16 = t is not None and (t.dtype == torch.float16 if isinstance(t, torch.Tensor) else int(t) == _lib.SASPA_F16)
    lib = _lib.load_f16() if f16 else _lib.load()
    return lib if _RECORDER is None else _RecordingLib(lib)


GEMM_FAMILY_FP8 = 8                  # recorder meta only: launches of saspa_gemm_fp8 (not a SaspaGemmParams.variant)
GEMM_FAMILY_FF_BLOCK = 16                 # saspa_ff_block (not a saspa_gemm dispatch: the launch names its family itself)
GEMM_FAMILY_MXFP8_CONV = 32               # saspa_conv3x3_mxfp8 (block-scaled e4m3 3x3 conv; recorder meta only, like GEMM_FAMILY_FP8)
GEMM_FAMILY_NAMES = {1: "tiled_4wave", 2: "wide_8wave", 3: "wave_specialised", 4: "a_stationary", 8: "fp8_e4m3", 16: "ff_block",
                     32: "mxfp8_conv"}


def _meta_kernel(p, meta):
    """Recorder runs only: append (kernel family, K slices) of the launch `p` describes -- the library's own dispatch, executed dry
    (saspa_gemm_which) -- to the launch's meta tuple, so that per-launch timings can be grouped by the kernel that really ran."""
    if _RECORDER is None or meta is None:
        return meta
    w = int(_L(p.dtype).saspa_gemm_which(C.byref(p)))
    return tuple(meta) + ((w & 0xff, w >> 8) if w > 0 else (0, 1))


def _probe_launch(kind, flops, call, meta=None):
    """A launch that the library may REFUSE without launching anything (SASPA_ERANGE on a `defer_reduce` contract it cannot
    honour): goes to the recorder only when it really ran (rc == 0) -- a refused probe used to be logged as a 2*M*N*K-FLOP
    launch of ~zero duration and the fallback's real launch was logged again."""
    if _RECORDER is None:
        return call()
    box = []

    def run():
        box.append(call())
        return box[0]
    rec = _RECORDER
    _IN_LAUNCH[0] = True
    try:
        if hasattr(rec, "conditional"):
            return rec.conditional(kind, flops, run, meta, lambda rc: rc == 0)
        return call()                # a recorder without the hook: record nothing for the probe (under-counts one launch)
    finally:
        _IN_LAUNCH[0] = False


def _dt(t):
    if t.dtype == torch.bfloat16:
        return _lib.SASPA_BF16
    if t.dtype == torch.float16:
        return _lib.SASPA_F16
    if t.dtype == torch.float32:
        return _lib.SASPA_F32
    raise TypeError(f"unsupported activation dtype {t.dtype}")


_F32_GEMM_MODE = ["exact"]


class f32_gemm_mode:
    """Context: how fp32 GEMMs / convs issued inside run -- "exact" (fp32 MFMA, the parity path) or "x3" (SASPA_F32X3: three
    bf16 MFMAs per product, ~2^-17 relative; the upcast SDXL VAE).  Storage and every other kernel stay fp32."""

    def __init__(self, mode):
        if mode not in ("exact", "x3"):
            raise ValueError(mode)
        self.mode = mode

    def __enter__(self):
        self.prev = _F32_GEMM_MODE[0]
        _F32_GEMM_MODE[0] = self.mode

    def __exit__(self, *a):
        _F32_GEMM_MODE[0] = self.prev


def _gemm_dt(t):
    d = _dt(t)
    return _lib.SASPA_F32X3 if (d == _lib.SASPA_F32 and _F32_GEMM_MODE[0] == "x3") else d


_F32_ATTN_MODE = ["unfused"]


class f32_attn_mode:
    """Context: how fp32 attention with heads of at most 160 channels issued inside runs (models.attention_core) -- "unfused" (scores
    GEMM -> row softmax -> PV GEMM through a score matrix, the default) or "fused" (flash_attn_f32x3: one launch, x3 products, no
    score matrix).  16-bit attention and wider heads do not look at it."""

    def __init__(self, mode):
        if mode not in ("unfused", "fused"):
            raise ValueError(mode)
        self.mode = mode

    def __enter__(self):
        self.prev = _F32_ATTN_MODE[0]
        _F32_ATTN_MODE[0] = self.mode

    def __exit__(self, *a):
        _F32_ATTN_MODE[0] = self.prev


def f32_attn_fused():
    return _F32_ATTN_MODE[0] == "fused"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("saspa_aug_amd ops run on the GPU only (tensor is on %s)" % t.device)


def _same_dtype(what, x, **ts):
    """Operands of one launch share its element type: the library reads them all as `_dt(x)`, and with two 16-bit types a mismatch
    would no longer show as a size error."""
    for name, t in ts.items():
        if t is not None and t.dtype != x.dtype:
            raise ValueError(f"{what}: {name} is {t.dtype}, the activations are {x.dtype}")


_SIDE_STREAMS = {}


def side_stream(device):
    """THE second stream of a device: one per process and device, shared by every step graph's ControlNet branch (round 6) and
    by a twin launch recorder's paired region.  Each _StepGraph used to take its own stream out of torch's 32-stream
    pool; a long session that captured two-branch graphs for dozens of pipelines ended in a segmentation fault inside
    hipGraphLaunch (hip::Graph::UpdateStreams, profiles/r5_graph_replay_segv_backtrace.txt); with one shared stream the full GPU
    suite runs two-branch graphs everywhere (profiles/r6_forkall_tests.log).  SASPA_SIDE_STREAM=per_graph = the old behaviour."""
    if os.environ.get("SASPA_SIDE_STREAM", "shared") == "per_graph":
        return torch.cuda.Stream(device=device)
    key = torch.device(device).index
    if key is None:
        key = torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def sleep_wait(event, poll_s=0.001):
    """Wait for a recorded torch.cuda.Event WITHOUT spinning a host core: hipEventSynchronize busy-waits on this stack even for
    hipEventBlockingSync events (rocr::core::BusyWaitSignal::WaitRelaxed under hip::Event::synchronize -- rocgdb stack of the
    generation loop's launch thread, profiles/r6_host_thread_stacks.txt), so the host polls hipEventQuery and sleeps in between.
    1 ms granularity against 20-35 ms sampling steps / 1-2 s batches."""
    import time
    while not event.query():
        time.sleep(poll_s)


def h2d(t, device, dtype=None):
    """Host -> device copy that does NOT block the host: through pinned memory, asynchronous in the current stream (a
    pageable-memory copy would wait for everything queued before it -- e.g. the previous batch's whole launch sequence --
    and defeat the batch pipeline of run_aug).  Device tensors pass through."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.is_cuda:
        return t if dtype is None or t.dtype == dtype else t.to(dtype)
    d = t.contiguous().pin_memory().to(device, non_blocking=True)
    return d if dtype is None or d.dtype == dtype else d.to(dtype)


def _pitch4(x):
    """[B,H,W,C] channels-last view -> pixel pitch; validates regular pixel rows."""
    b, h, w, c = x.shape
    if c > 1 and x.stride(3) != 1:
        raise ValueError("last dim must be contiguous")
    ld = x.stride(2)
    if ld < c:
        raise ValueError("pixel pitch smaller than the channel count")
    if h > 1 and x.stride(1) != w * ld:
        raise ValueError("rows must be densely packed at the pixel pitch")
    if b > 1 and x.stride(0) != h * w * ld:
        raise ValueError("batch images must be densely packed at the pixel pitch")
    return ld


def round8(n):
    return (n + 7) // 8 * 8


_TWIN = [False]


class twin_branch:
    """Context: the launches issued inside run on ONE of two concurrent graph branches that walk the same layer shapes at the
    same time (UNet encoder || ControlNet encoder, pipeline._StepGraph).  The library sizes a launch for the whole chip; with
    a twin beside it half the chip is what it gets, so the launches carry SaspaGemmParams.sharing = 1 (ABI 15): tile choice
    and split-K are made for 128 CUs -- the convs / projections of the 32x32 level (128 wide tiles) run un-split next to
    their twin (no fp32 slabs, no reduce launch), the 16x16 level takes two K slices instead of four.  SASPA_TWIN_KS=0 turns
    the hint off (A/B knob).  Results differ from the single-branch dispatch only by the summation order of K."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _TWIN[0]
        _TWIN[0] = self.on and os.environ.get("SASPA_TWIN_KS", "1") != "0"

    def __exit__(self, *a):
        _TWIN[0] = self.prev


def _suggest_ksplit(p, t, force=None):
    """Split-K factor from the library's own heuristic (saspa_gemm_suggest_ksplit: every other field of p is already
    filled in, `sharing` from the twin context here) or the caller's override."""
    p.ksplit, p.workspace = 1, None
    p.sharing = 1 if _TWIN[0] else 0
    return _L(t).saspa_gemm_suggest_ksplit(C.byref(p)) if force is None else int(force)


def _alloc_slabs(p, ks, t):
    """Run p on ks K slices: allocates the ks * M * N fp32 slab workspace (None for one slice)."""
    p.ksplit, p.workspace = 1, None
    if ks > 1:
        ws = torch.empty((ks * p.M * p.N,), device=t.device, dtype=torch.float32)
        p.ksplit, p.workspace = ks, C.c_void_p(ws.data_ptr())
        return ws           # keep alive until the launch is enqueued
    return None


def _set_splitk(p, m, n, k, t, force=None):
    """Split-K factor (heuristic or override) and its slab workspace for the M x N x K problem p describes."""
    return _alloc_slabs(p, _suggest_ksplit(p, t, force), t)


def _as_over_stats():
    return os.environ.get("SASPA_GEMM_AS_OVER_STATS", "1") != "0"


def splitk_gn_enabled():
    """SASPA_SPLITK_GN=0: conv1 -> norm2 of the small levels runs as conv (+ reduce) and GroupNorm launches again (A/B knob)."""
    return os.environ.get("SASPA_SPLITK_GN", "1") != "0"


def gn_onepass_enabled():
    """SASPA_GN_ONEPASS=0: small-image GroupNorms run as statistics pass + apply pass again (A/B knob)."""
    return os.environ.get("SASPA_GN_ONEPASS", "1") != "0"


def gn_fusion_enabled():
    """SASPA_GN_FUSE=0: every GroupNorm runs its own statistics pass (A/B knob for the epilogue statistics)."""
    return os.environ.get("SASPA_GN_FUSE", "1") != "0"


def upconv_phase_enabled():
    """SASPA_UPCONV_PHASE=0: the Upsample2D convs keep their 3x3 weights and run as one nearest-x2 implicit GEMM over all nine
    taps again (A/B knob; read when a network is packed).  Default: the four 2x2 phase convs, 4/9 of the multiply-accumulates."""
    return os.environ.get("SASPA_UPCONV_PHASE", "1") != "0"


# What an epilogue hangs on its output tensor as `saspa_gn`: the statistics, their channel unit, and the buffer and tensor version
# they describe.  `_fresh_stats` re-checks the last two, so a tensor that was re-pointed or written in place through torch since the
# launch falls back to its own statistics pass.
GnStats = collections.namedtuple("GnStats", "stats unit data_ptr version")


def _gn_stats_for(p, out, gn_unit, b, hw, n):
    """Epilogue GroupNorm statistics (SaspaGemmParams.gn_stats): allocate the [rows / 128, N / unit, 2] fp32 buffer, hang it
    on the output tensor (`saspa_gn` = (stats, unit): `groupnorm` picks it up and skips its statistics pass) -- when the
    shape allows it: bf16, whole 128-row blocks per image, whole 160-column tiles, dense output rows."""
    if hasattr(out, "saspa_gn"):
        del out.saspa_gn                  # a reused `out=`: statistics of an earlier launch must not outlive this one
    if not gn_unit or not gn_fusion_enabled() or not is_half(out):
        return None
    if hw % 128 or n % 160 or 80 % gn_unit or gn_unit % 2 or gn_unit > 16 or out.shape[-1] != n or p.ldo % 8 or (p.residual and p.ldr % 8):
        return None
    stats = torch.empty((b * hw // 128, n // gn_unit, 2), device=out.device, dtype=torch.float32)
    p.gn_stats, p.gn_unit = _ptr(stats), int(gn_unit)
    out.saspa_gn = GnStats(stats, int(gn_unit), out.data_ptr(), out._version)
    return stats


def _fresh_stats(t):
    """The epilogue statistics hung on t (`saspa_gn`) as GnStats, when they still describe it -- the same buffer and tensor version,
    one statistics row per 128 pixels -- else None."""
    g = getattr(t, "saspa_gn", None) if t is not None else None
    if g is None:
        return None
    g = GnStats(*g)
    if g.data_ptr != t.data_ptr() or g.version != t._version or g.stats.shape[0] * 128 != t.shape[0] * t.shape[1] * t.shape[2]:
        return None
    return g


def _epilogue_stats(x, x2, groups):
    """(GnStats of x, GnStats of x2 or None) that the producers' epilogues hung on the tensors (`saspa_gn`, see _gn_stats_for), when
    they still describe the tensors and a GroupNorm of `groups` groups over cat(x, x2) can use them; else (None, None)."""
    b, h, w, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    g0, g1 = _fresh_stats(x), _fresh_stats(x2)
    fused = (g0 is not None and (x2 is None or g1 is not None) and gn_fusion_enabled() and (h * w) % 128 == 0
             and (x2 is None or g1.unit == g0.unit) and c0 % g0.unit == 0 and c1 % g0.unit == 0 and ((c0 + c1) // groups) % g0.unit == 0
             and g0.stats.shape[1] * g0.unit == c0 and (x2 is None or g1.stats.shape[1] * g1.unit == c1))
    return (g0, g1) if fused else (None, None)


def _gn_nsplit(batch, hw, c8):
    """Pixel splits of the statistics pass: about 1024 workgroups per channel slab (the apply pass re-reads
    nsplit * slabs * groups sums per workgroup, so no more than needed to fill the chip)."""
    want = max(1, int(os.environ.get("SASPA_GN_BLOCKS", "1024")) // max(1, batch))
    return max(1, min(want, 64, hw // 16 if hw >= 16 else 1))


def _gn_params(x, x2, gamma, beta, groups, eps, act, out, *, partial=None, nsplit=0, stats=(None, None)):
    """SaspaGroupNormParams of GroupNorm(+act) over cat(x, x2) into `out` (None: a launch that writes no y -- the statistics pass, the
    quantiser).  Where the statistics come from is the caller's: `partial` / `nsplit` of a statistics pass, or `stats` = the
    producers' (GnStats, GnStats or None) from `_epilogue_stats`; neither for the launches that take their own."""
    p = _lib.GroupNormParams()
    p.dtype = _dt(x)
    p.x0, p.x1, p.c0, p.c1 = _ptr(x), _ptr(x2), x.shape[3], 0 if x2 is None else x2.shape[3]
    p.ldx0, p.ldx1 = _pitch4(x), 0 if x2 is None else _pitch4(x2)
    p.batch, p.hw, p.groups, p.eps = x.shape[0], x.shape[1] * x.shape[2], int(groups), float(eps)
    p.gamma, p.beta = _ptr(gamma), _ptr(beta)
    p.partial, p.nsplit, p.scale_shift = _ptr(partial), nsplit, None
    p.act = int(act)
    if out is not None:
        p.y, p.ldy = _ptr(out), _pitch4(out)
    g0, g1 = stats
    if g0 is not None:
        p.stats0, p.stats1, p.unit = _ptr(g0.stats), _ptr(None if g1 is None else g1.stats), g0.unit
    return p


def _ldrv(rowvec):
    """Pitch of the per-image row vector: 0 = one vector for every image ([N] or [1, N])."""
    return 0 if (rowvec is None or rowvec.dim() == 1 or rowvec.shape[0] == 1) else rowvec.stride(0)


def _check_conv_operands(x, x2, w, taps, window, n, ho, wo, bias, rowvec, residual, out):
    """Operands of a conv of x (| x2) with `taps` weight columns per input channel into [B, ho, wo, >= n].
    Geometry is validated HERE: the kernel trusts it (a mismatched skip / residual would be read out of bounds)."""
    b, h, wd, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    if x2 is not None and (tuple(x2.shape[:3]) != (b, h, wd) or x2.dtype != x.dtype):
        raise ValueError(f"concat source {tuple(x2.shape)} does not match {tuple(x.shape)} (batch / height / width / dtype)")
    if w.shape[-1] < taps * (c0 + c1) or w.dtype != x.dtype:
        raise ValueError(f"weights {tuple(w.shape)} {w.dtype} do not fit a {window} window over {c0}+{c1} channels of {x.dtype}")
    if ho <= 0 or wo <= 0:
        raise ValueError("empty convolution output")
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (t.dim() != 4 or tuple(t.shape[:3]) != (b, ho, wo) or t.shape[3] < n or t.dtype != x.dtype):
            raise ValueError(f"{name} {tuple(t.shape)} {t.dtype} does not match the output [{b},{ho},{wo},>={n}] {x.dtype}")
    if bias is not None and bias.numel() < n:
        raise ValueError("bias shorter than N")
    if rowvec is not None and (rowvec.shape[-1] < n or (rowvec.dim() == 2 and rowvec.shape[0] not in (1, b))):
        raise ValueError(f"rowvec {tuple(rowvec.shape)} must be [N] or [batch, N]")


def _conv_out(x, ho, wo, n):
    """The output a conv allocates: [B, ho, wo, round8(N)], pad channels zero."""
    nc = round8(n)
    return (torch.zeros if nc != n else torch.empty)((x.shape[0], ho, wo, nc), device=x.device, dtype=x.dtype)


def _conv_gemm_params(x, x2, w, bias, rowvec, residual, alpha, act, kh, kw, stride, pad, upsample, ho, wo, n):
    """The implicit-GEMM fields of SaspaGemmParams for a conv of x (| x2) into [B, ho, wo, n]: sources and pitches, window, weights,
    M / N / K and the epilogue operands.  Output, K order, variant, statistics and split-K are the caller's."""
    b, h, wd, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    p = _lib.GemmParams()
    p.dtype = _gemm_dt(x)
    p.a0, p.a1, p.c0, p.c1 = _ptr(x), _ptr(x2), c0, c1
    p.lda0 = _pitch4(x)
    p.lda1 = 0 if x2 is None else _pitch4(x2)
    p.batch, p.hin, p.win, p.hout, p.wout = b, h, wd, ho, wo
    p.kh, p.kw, p.stride, p.pad, p.upsample = kh, kw, stride, pad, upsample
    p.w, p.ldw = _ptr(w), w.stride(-2)
    p.M, p.N, p.K = b * ho * wo, n, kh * kw * (c0 + c1)
    p.bias, p.rowvec, p.ldrv = _ptr(bias), _ptr(rowvec), _ldrv(rowvec)
    p.residual = _ptr(residual)
    p.ldr = 0 if residual is None else _pitch4(residual)
    p.alpha, p.act = float(alpha), int(act)
    p.nb1 = p.nb2 = 1
    return p


def _deferred_reduce_gn(p, lib, out, split, launch_conv, what, gn, flops, meta):
    """conv -> GroupNorm whose only reader is that GroupNorm, as the conv on K slices with the reduce left to saspa_splitk_groupnorm
    (sums the slabs, takes the statistics, normalises: the un-normalised output is never written).  p: the conv's filled
    SaspaGemmParams; split(): chooses its K slices (the heuristic WITHOUT epilogue statistics: nobody reads them); launch_conv():
    launches it and returns the library's code (`what` names it in an error); gn = (gamma, beta, groups, eps, act) of the GroupNorm
    over `out`; meta(): the recorder meta of the conv launch.  True: `out` holds the normalised tensor.  False: nothing was
    launched and p is back on one slice, not deferred -- the caller runs conv and groupnorm as usual."""
    if not (splitk_gn_enabled() and not p.residual and p.act == ACT_NONE and out.shape[-1] == p.N):
        return False
    _ws = split()  # noqa: F841
    gamma, beta, groups, eps, act = gn
    q = _gn_params(out, None, gamma, beta, groups, eps, act, out)
    if p.ksplit > 1 and lib.saspa_splitk_groupnorm_eligible(C.byref(p), C.byref(q)):
        p.defer_reduce = 1
        # SASPA_ERANGE: the dispatch would run this problem on ONE slice / a kernel without slabs (a variant pin, an A/B
        # knob): nothing was launched, fall back to conv + groupnorm
        rc = _probe_launch("gemm", flops, launch_conv, meta())
        if rc == 0:
            _launch("splitk_gn", 0.0, lambda: _lib.check(lib.saspa_splitk_groupnorm(C.byref(p), C.byref(q), _stream()), "saspa_splitk_groupnorm"))
            return True
        if rc != _lib.SASPA_ERANGE:
            _lib.check(rc, what)
    p.ksplit, p.workspace, p.defer_reduce = 1, None, 0
    return False


def conv(x, w, bias=None, *, kh=1, kw=1, stride=1, pad=0, upsample=False, x2=None, rowvec=None,
         residual=None, alpha=1.0, act=ACT_NONE, out=None, n_out=None, variant=0, korder=None, ksplit=None, out_hw=None,
         gn_unit=None, fuse_gn=None):
    """Implicit-GEMM conv of channels-last ``x`` (optionally channel-concatenated with
    ``x2``) with packed weights ``w`` [N, kh*kw*(C0+C1)].  Returns [B, Ho, Wo, round8(N)]
    (pad channels zero).  ``korder``: K order the weights were packed in (default: the tensor's
    ``saspa_korder`` attribute set by the packer, else tap-major).  ``gn_unit``: the output feeds a GroupNorm whose
    groups are multiples of this many channels -> the epilogue leaves its statistics (`_gn_stats_for`).
    ``w`` [4, N, 4*C0] (weights.pack_conv_up2x) with ``upsample=True, kh=kw=3, pad=1``: the same layer as four 2x2 phase convs over
    the low-res input in one launch (SaspaGemmParams.upsample = 2); no x2 / rowvec / residual / act there.
    ``fuse_gn`` = (gamma, beta, groups, eps, act): the conv's ONLY consumer is this GroupNorm (ResnetBlock2D.conv1 -> norm2 ->
    SiLU), so the call returns the NORMALISED tensor: where the conv runs on K slices and an image's group fits one workgroup
    (the 8x8 / 16x16 levels) the reduce launch, the statistics and the apply pass are one launch (saspa_splitk_groupnorm, ABI
    18: the un-normalised output is never written); otherwise the conv runs as usual and `groupnorm` follows."""
    _check_dev(x, w, bias, x2, rowvec, residual, out)
    lib = _L(x)
    b, h, wd, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    hv, wv = (2 * h, 2 * wd) if upsample else (h, wd)
    # phase weights of weights.pack_conv_up2x ([4, N, 4C]): the caller describes the layer (nearest x2, 3x3, pad 1), the launch is
    # SaspaGemmParams.upsample = 2 -- four 2x2 convs over the low-res input, one launch
    phase = w.dim() == 3
    if phase and not (upsample and kh == 3 and kw == 3 and stride == 1 and pad == 1 and w.shape[0] == 4 and is_half(x)
                      and x2 is None and rowvec is None and residual is None and act == ACT_NONE and out_hw is None
                      and fuse_gn is None and w.is_contiguous()):
        raise ValueError("phase weights serve the plain nearest-x2 3x3 / pad 1 conv of a 16-bit tensor only")
    ho = (hv + 2 * pad - kh) // stride + 1
    wo = (wv + 2 * pad - kw) // stride + 1
    if out_hw is not None:
        # asymmetric zero padding (Downsample2D(padding=0) of the VAE encoder pads right / bottom only): windows may hang
        # over the far edges, where the loaders' bounds masks read zeros; the C ABI checks the window origins
        ho, wo = out_hw
    n = w.shape[-2] if n_out is None else n_out
    _check_conv_operands(x, x2, w, 4 if phase else kh * kw, f"{kh}x{kw}", n, ho, wo, bias, rowvec, residual, out)
    if out is None:
        out = _conv_out(x, ho, wo, n)
    if phase:
        kh = kw = 2                   # what runs: a 2x2 window (K = 4C) over the low-res rows, SaspaGemmParams.upsample = 2
    p = _conv_gemm_params(x, x2, w, bias, rowvec, residual, alpha, act, kh, kw, stride, pad, 2 if phase else int(upsample), ho, wo, n)
    p.out, p.ldo = _ptr(out), _pitch4(out)
    p.variant = int(variant)
    p.korder = int(getattr(w, "saspa_korder", 0)) if korder is None else int(korder)
    if getattr(w, "saspa_wsplit", 0):
        # weights.presplit_x3 (ABI 20): [hi | lo] bf16 pairs per K-tile -- only the SASPA_F32X3 loop can read them
        if p.dtype != _lib.SASPA_F32X3:
            raise RuntimeError("pre-split (SASPA_F32X3) weights used outside ops.f32_gemm_mode('x3')")
        p.w_split = 1
    # a level-0 pointwise layer the A-stationary kernel takes on whole rounds (Transformer2DModel.proj_out): that kernel has no
    # statistics epilogue, and A-stationary + the consumer's own statistics pass (27 + 12 us) beats the tiled kernel with the
    # statistics in its epilogue (53 us); SASPA_GEMM_AS_OVER_STATS=0 keeps the statistics
    if gn_unit and kh == 1 and kw == 1 and c1 == 0 and is_half(x) and _as_over_stats() and \
            lib.saspa_gemm_as_auto(C.byref(p)) == 1:
        gn_unit = None
    # (phase mode reports what runs: K = 4C, a 2x2 window over M / 4 low-res rows, 2*M*N*4C FLOPs)
    meta = (p.M, p.N, p.K, kh, stride, int(upsample), c1 > 0, residual is not None, n // 2 if act == ACT_GEGLU else n)
    flops = 2.0 * p.M * p.N * p.K

    def launch():
        return lib.saspa_gemm(C.byref(p), _stream())
    if fuse_gn is not None and _deferred_reduce_gn(p, lib, out, lambda: _set_splitk(p, p.M, p.N, p.K, x, ksplit), launch,
                                                   "saspa_gemm(conv, deferred reduce)", fuse_gn, flops, lambda: _meta_kernel(p, meta)):
        return out
    _gs = _gn_stats_for(p, out, gn_unit, b, ho * wo, n)  # noqa: F841   (set BEFORE the split-K heuristic looks at p)
    _ws = _set_splitk(p, p.M, p.N, p.K, x, ksplit)  # noqa: F841   (ksplit: tuning override of the heuristic)
    _launch("gemm", flops, lambda: _lib.check(launch(), "saspa_gemm(conv)"), _meta_kernel(p, meta))
    return out if fuse_gn is None else groupnorm(out, *fuse_gn)


def conv_gn(x, gn, w32, bias=None, *, x2=None, rowvec=None, residual=None, alpha=1.0, out=None, ksplit=None, gn_unit=None,
            defer_to=None):
    """out = conv3x3(act(GroupNorm(cat(x, x2)))) in ONE launch (saspa_conv3x3_halo, ABI 19): the GroupNorm (+ SiLU) is applied
    to the conv's input tile in LDS -- ResnetBlock2D's norm -> SiLU -> conv.  gn = (gamma_beta32, groups, eps, act) or None
    (plain halo conv of an already normalised x); w32: weights packed SASPA_KORDER_CHUNK32 (weights.to_chunk32_major).
    Returns None when the launch is not eligible (the caller falls back to groupnorm + conv).  Statistics of x come from its
    producer's epilogue when it left them (`saspa_gn`), else from a statistics pass launched here.  defer_to = (gamma, beta,
    groups, eps, act): the conv's only consumer is that GroupNorm and the conv runs on K slices -> saspa_splitk_groupnorm sums the
    slabs and normalises (as ops.conv(fuse_gn=...))."""
    _check_dev(x, w32, bias, x2, rowvec, residual, out)
    if x.dtype != torch.bfloat16:
        return None
    lib = _L()
    b, h, wd, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    n = w32.shape[0]
    _check_conv_operands(x, x2, w32, 9, "3x3", n, h, wd, bias, rowvec, residual, out)
    p = _conv_gemm_params(x, x2, w32, bias, rowvec, residual, alpha, ACT_NONE, 3, 3, 1, 1, 0, h, wd, n)
    p.korder = 2
    q = None
    if gn is not None:
        gb32, groups, eps, gact = gn
        q = _lib.ConvGnParams()
        q.gamma_beta32, q.groups, q.eps, q.act = _ptr(gb32), int(groups), float(eps), int(gact)
        g0, g1 = _epilogue_stats(x, x2, groups)
        if g0 is not None:
            q.stats0, q.stats1, q.unit = _ptr(g0.stats), _ptr(None if g1 is None else g1.stats), g0.unit
    qq = C.byref(q) if q is not None else None
    own_stats = q is not None and not q.stats0
    # eligibility is decided BEFORE any allocation / statistics launch (out / ldo of a would-be output: dense rows of round8(N))
    p.out, p.ldo = _ptr(x), round8(n) if out is None else _pitch4(out)
    if own_stats:
        q.partial, q.nsplit = _ptr(x), 1            # placeholders for the eligibility check
    if not lib.saspa_conv3x3_halo_eligible(C.byref(p), qq):
        return None
    if own_stats:
        # no epilogue statistics on the input: the statistics pass of `groupnorm`, then the fused apply + conv
        ctot = c0 + c1
        nsplit = _gn_nsplit(b, h * wd, ctot // 8)
        partial = torch.empty((b * nsplit * ctot * 2,), device=x.device, dtype=torch.float32)
        g = _gn_params(x, x2, gb32, gb32, groups, eps, ACT_NONE, None, partial=partial, nsplit=nsplit)   # gamma / beta: not read by the pass
        _launch("gn_stats", 0.0, lambda: _lib.check(lib.saspa_groupnorm_stats(C.byref(g), _stream()), "saspa_groupnorm_stats"))
        q.partial, q.nsplit = _ptr(partial), nsplit
    if out is None:
        out = _conv_out(x, h, wd, n)
    p.out, p.ldo = _ptr(out), _pitch4(out)
    meta = (p.M, p.N, p.K, 3, 1, 0, c1 > 0, residual is not None, n)
    flops = 2.0 * p.M * p.N * p.K

    def _split(force):
        p.korder = 1                                  # the heuristic knows the im2col kernels' orders only; same K
        ks = _suggest_ksplit(p, x, force)
        p.korder = 2
        return _alloc_slabs(p, lib.saspa_conv3x3_halo_ksplit(C.byref(p), ks), x)

    def launch():
        return lib.saspa_conv3x3_halo(C.byref(p), qq, _stream())
    if defer_to is not None and _deferred_reduce_gn(p, lib, out, lambda: _split(ksplit), launch, "saspa_conv3x3_halo(deferred reduce)",
                                                    defer_to, flops, lambda: meta):
        return out
    _gs = _gn_stats_for(p, out, gn_unit, b, h * wd, n)  # noqa: F841
    _ws = _split(ksplit)  # noqa: F841
    _launch("gemm", flops, lambda: _lib.check(launch(), "saspa_conv3x3_halo"), meta)
    return out if defer_to is None else groupnorm(out, *defer_to)


def _linear_params(x2, w, bias, r2, o2, alpha, act, rowvec, variant, m, n, k):
    p = _lib.GemmParams()
    p.dtype = _gemm_dt(x2)
    p.a0, p.a1, p.c0, p.c1 = _ptr(x2), None, k, 0
    p.lda0, p.lda1 = (x2.stride(0) if m > 1 else max(k, x2.stride(0))), 0
    p.batch, p.hin, p.win, p.hout, p.wout = 1, m, 1, m, 1
    p.kh = p.kw = p.stride = 1
    p.pad = p.upsample = 0
    p.w, p.ldw = _ptr(w), w.stride(0)
    p.M, p.N, p.K = m, n, k
    p.bias, p.rowvec, p.ldrv = _ptr(bias), _ptr(rowvec), 0
    p.residual = _ptr(r2)
    p.ldr = 0 if r2 is None else (r2.stride(0) if m > 1 else max(n, r2.stride(0)))
    p.alpha, p.act = float(alpha), int(act)
    p.out = _ptr(o2)
    p.ldo = o2.stride(0) if m > 1 else max(o2.shape[-1], o2.stride(0))
    p.nb1 = p.nb2 = 1
    p.variant = int(variant)
    return p


def linear_ln_fusable(x, w, *, act=ACT_NONE, n_out=None):
    """Non-zero (2) if `linear(x, w, ..., ln=...)` / `out_t=` can run: the A-stationary kernel takes the problem
    (saspa_gemm_as_eligible: bf16, K = 320, N % 64 == 0, >= 192 blocks of 256 rows).  Use it as a boolean."""
    if not x.is_cuda or not is_half(x):
        return 0
    k = x.shape[-1]
    x2 = x.reshape(-1, k) if x.dim() != 2 else x
    m, n = x2.shape[0], w.shape[0]
    nc = (n // 2 if act == ACT_GEGLU else n) if n_out is None else n_out
    p = _linear_params(x2, w, None, None, x2, 1.0, act, None, 0, m, n, k)
    p.ldo = round8(nc)                    # the output a call would allocate (only its pitch / alignment are looked at)
    return int(_L(x).saspa_gemm_as_eligible(C.byref(p)))


def linear(x, w, bias=None, *, residual=None, alpha=1.0, act=ACT_NONE, out=None, rowvec=None, variant=0, ksplit=None,
           ln=None, out_t=None, n_split=None, rows_per_batch=None):
    """x: [..., K] (last dim contiguous, uniform row pitch) @ w[N, K]^T -> [..., round8(N)].
    ln = (gamma, beta, eps): LayerNorm over K applied to x inside the launch (SaspaGemmParams.ln_gamma: the A-stationary
    kernel only -- check `linear_ln_fusable` first; the library returns ERANGE otherwise).
    out_t [B, N - n_split, ld] with n_split, rows_per_batch: output columns >= n_split are written transposed per batch of
    rows_per_batch rows (the V^T operand of flash_attn next to Q | K); the returned tensor then has n_split columns."""
    _check_dev(x, w, bias, residual, out, out_t)
    _same_dtype("linear", x, w=w, residual=residual, out=out)
    lib = _L(x)
    k = x.shape[-1]
    x2 = x.reshape(-1, k) if x.dim() != 2 else x
    m = x2.shape[0]
    n = w.shape[0]
    if out is None:
        nc = round8(n // 2 if act == ACT_GEGLU else (n if out_t is None else n_split))
        out = (torch.zeros if (nc != n and act != ACT_GEGLU and out_t is None) else torch.empty)((m, nc), device=x.device, dtype=x.dtype)
    o2 = out.view(-1, out.shape[-1]) if out.dim() != 2 else out
    r2 = None if residual is None else (residual.reshape(-1, residual.shape[-1]) if residual.dim() != 2 else residual)
    p = _linear_params(x2, w, bias, r2, o2, alpha, act, rowvec, variant, m, n, k)
    if ln is not None:
        g, b_, eps = ln
        _check_dev(g, b_)
        if g.dtype != torch.float32 or b_.dtype != torch.float32 or g.numel() < k or b_.numel() < k:
            raise ValueError("LayerNorm gamma / beta must be fp32 vectors of K elements")
        p.ln_gamma, p.ln_beta, p.ln_eps = _ptr(g), _ptr(b_), float(eps)
    if out_t is not None:
        if out_t.dim() != 3 or out_t.stride(2) != 1 or out_t.dtype != x.dtype or n_split is None or not rows_per_batch:
            raise ValueError("out_t must be [batch, N - n_split, ld] in the input dtype, with n_split and rows_per_batch given")
        if out_t.shape[0] * rows_per_batch != m or out_t.shape[1] != n - n_split or out_t.shape[2] < rows_per_batch:
            raise ValueError(f"out_t {tuple(out_t.shape)} does not hold {n - n_split} transposed columns of {m} rows in batches of {rows_per_batch}")
        p.out_t, p.ldt, p.st = _ptr(out_t), out_t.stride(1), out_t.stride(0)
        p.n_split, p.rows_per_batch = int(n_split), int(rows_per_batch)
    _ws = _set_splitk(p, m, n, k, x, ksplit) if (act != ACT_GEGLU and ln is None and out_t is None) else None  # noqa: F841
    if act == ACT_GEGLU:
        p.ksplit, p.workspace = 1, None
    _launch("gemm", 2.0 * m * n * k, lambda: _lib.check(lib.saspa_gemm(C.byref(p), _stream()), "saspa_gemm(linear)"),
            _meta_kernel(p, (m, n, k, 0, 1, 0, False, residual is not None, n // 2 if act == ACT_GEGLU else n)))
    if x.dim() != 2 and out.dim() == 2:
        return out.reshape(*x.shape[:-1], out.shape[-1])
    return out


def dup_rows(x):
    """[B, ...] -> [2B, ...] = cat([x, x]) in ONE launch (a broadcast copy into a [2, B, ...] view): the point where a CFG-shared
    prefix becomes the two halves of the batch (models._Net.encode(cfg_pair=True))."""
    out = torch.empty((2,) + tuple(x.shape), device=x.device, dtype=x.dtype)
    out.copy_(x.unsqueeze(0).expand_as(out))
    return out.view((2 * x.shape[0],) + tuple(x.shape[1:]))


def xattn_block(x, ln, w, bias, kf, vf, nk, rows_per_sample, residual=None, out=None, x_rows=None):
    """The cross-attention half of a level-0 transformer block in one launch (saspa_xattn_block, include/saspa_hip.h):
    out = residual + to_out(softmax(to_q(LayerNorm(x)) K^T) V) + bias.  x [..., 320] bf16 (uniform row pitch), ln = (gamma, beta,
    eps), w / bias from weights.pack_xattn_w, kf / vf [B, ...] from weights.xattn_kv_fragments, residual defaults to x.
    x_rows (saspa_xattn_block_bcast): x / residual hold x_rows rows that every group of x_rows output rows reads again, the
    output has kf.shape[0] * rows_per_sample rows -- the two CFG halves of a shared prefix, each against its own keys."""
    _check_dev(x, w, bias, kf, vf, residual, out)
    _same_dtype("xattn_block", x, w=w, kf=kf, vf=vf, residual=residual, out=out)
    lib = _L(x)
    c = x.shape[-1]
    x2 = x.reshape(-1, c) if x.dim() != 2 else x
    m = x2.shape[0]
    if not is_half(x) or c != 320:
        raise ValueError("xattn_block: bf16 rows of 320 channels")
    r2 = x2 if residual is None else (residual.reshape(-1, c) if residual.dim() != 2 else residual)
    if x_rows is not None:
        if int(x_rows) != m or r2.shape[0] != m:
            raise ValueError(f"xattn_block: x_rows = {x_rows}, x holds {m} rows and the residual {r2.shape[0]}")
        m = kf.shape[0] * int(rows_per_sample)
    if out is None:
        out = torch.empty((m, c), device=x.device, dtype=x.dtype)
    o2 = out.view(-1, c) if out.dim() != 2 else out
    g, b_, eps = ln
    p = _lib.XattnBlockParams()
    p.x, p.ldx = _ptr(x2), x2.stride(0)
    p.residual, p.ldr = _ptr(r2), r2.stride(0)
    p.M, p.rows_per_sample = m, int(rows_per_sample)
    p.ln_gamma, p.ln_beta, p.ln_eps = _ptr(g), _ptr(b_), float(eps)
    p.w, p.ldw, p.bias = _ptr(w), w.stride(0), _ptr(bias)
    p.kf, p.kf_stride = _ptr(kf), kf.stride(0) * kf.element_size()
    p.vf, p.vf_stride = _ptr(vf), vf.stride(0) * vf.element_size()
    p.nk = int(nk)
    p.out, p.ldo = _ptr(o2), o2.stride(0)
    if kf.shape[0] * rows_per_sample != m or vf.shape[0] != kf.shape[0]:
        raise ValueError(f"xattn_block: {kf.shape[0]} samples of {rows_per_sample} rows do not make {m} rows")
    # algorithmic work: to_q + to_out (2 x 2 M C^2) and the two attention products over the nk keys (2 x 2 M nk C)
    flops = 4.0 * m * c * c + 4.0 * m * nk * c
    if x_rows is None:
        call = lambda: _lib.check(lib.saspa_xattn_block(C.byref(p), _stream()), "saspa_xattn_block")  # noqa: E731
    else:
        call = lambda: _lib.check(lib.saspa_xattn_block_bcast(C.byref(p), int(x_rows), _stream()), "saspa_xattn_block_bcast")  # noqa: E731
    _launch("gemm", flops, call, (m, 2 * c + 2 * nk, c, 0, 1, 0, False, True, c))
    if x_rows is None and x.dim() != 2 and out.dim() == 2:
        return out.reshape(*x.shape[:-1], c)
    return out


def gemm_batched(a, lda, sa, w, ldw, sw, out, ldo, so, m, n, k, nb1, nb2, alpha=1.0, residual=None, ldr=0, act=ACT_NONE):
    """Raw batched GEMM out[z] = act(alpha * a[z] @ w[z]^T) (+ residual[z], same batch strides as out); s* = (stride1,
    stride2) in elements.  ``a``/``w``/``out``/``residual`` are tensors whose data_ptr is the z=0 origin."""
    _check_dev(a, w, out, residual)
    _same_dtype("gemm_batched", a, w=w, out=out, residual=residual)
    lib = _L(a)
    p = _lib.GemmParams()
    p.dtype = _gemm_dt(a)
    p.a0, p.a1, p.c0, p.c1, p.lda0, p.lda1 = _ptr(a), None, k, 0, lda, 0
    p.batch, p.hin, p.win, p.hout, p.wout = 1, m, 1, m, 1
    p.kh = p.kw = p.stride = 1
    p.pad = p.upsample = 0
    p.w, p.ldw = _ptr(w), ldw
    p.M, p.N, p.K = m, n, k
    p.bias = p.rowvec = None
    p.residual, p.ldr = _ptr(residual), int(ldr)
    p.ldrv = 0
    p.alpha, p.act = float(alpha), int(act)
    p.out, p.ldo = _ptr(out), ldo
    p.nb1, p.nb2 = nb1, nb2
    p.sa1, p.sa2 = sa
    p.sw1, p.sw2 = sw
    p.so1, p.so2 = so
    p.ksplit, p.workspace = 1, None
    _launch("gemm", 2.0 * m * n * k * nb1 * nb2,
            lambda: _lib.check(lib.saspa_gemm(C.byref(p), _stream()), "saspa_gemm(batched)"),
            _meta_kernel(p, (m, n, k, -nb1 * nb2, 1, 0, False, residual is not None, n)))
    return out


def _ff_params(x, ln, w1p, b1p, w2f, b2, residual, out):
    c = x.shape[-1]
    x2 = x.reshape(-1, c) if x.dim() != 2 else x
    m = x2.shape[0]
    r2 = x2 if residual is None else (residual.reshape(-1, c) if residual.dim() != 2 else residual)
    p = _lib.FfBlockParams()
    p.x, p.ldx, p.residual, p.ldr, p.M, p.F = _ptr(x2), x2.stride(0), _ptr(r2), r2.stride(0), m, w2f.shape[0] * 32
    if ln is not None:
        p.ln_gamma, p.ln_beta, p.ln_eps = _ptr(ln[0]), _ptr(ln[1]), float(ln[2])
    p.w1, p.ldw1, p.b1, p.w2f, p.b2 = _ptr(w1p), w1p.stride(0), _ptr(b1p), _ptr(w2f), _ptr(b2)
    if out is not None:
        o2 = out.reshape(-1, c) if out.dim() != 2 else out
        p.out, p.ldo = _ptr(o2), o2.stride(0)
    return p, x2, r2, m, c


def ff_block_eligible(x, w1p, w2f):
    """Can `ff_block` take these tokens (bf16, 320 channels, rows % 128 == 0 ...)?  Host-side, launches nothing."""
    if not x.is_cuda or not is_half(x) or x.shape[-1] != 320 or w1p.dtype != x.dtype or w2f.dtype != x.dtype:
        return False
    p, x2, _, m, _ = _ff_params(x, None, w1p, w1p, w2f, w1p, None, None)
    p.out, p.ldo = p.x, p.ldx
    return bool(_L(x).saspa_ff_block_eligible(C.byref(p)))


def ff_block(x, ln, w1p, b1p, w2f, b2, residual=None, out=None):
    """The feed-forward half of a level-0 transformer block in one launch (saspa_ff_block, include/saspa_hip.h):
    out = residual + W2 (v * gelu(g)) + b2, [v ; g] = W1 LayerNorm(x) + b1.  x [..., 320] bf16 (uniform row pitch), ln = (gamma, beta,
    eps) or None, w1p / b1p / w2f / b2 from weights.pack_ff_block (bf16 / fp32 / bf16 / fp32), residual defaults to x."""
    _check_dev(x, w1p, b1p, w2f, b2, residual, out)
    if not is_half(x) or w1p.dtype != x.dtype or w2f.dtype != x.dtype:
        raise TypeError("ff_block: bf16 activations / weights")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    p, x2, r2, m, c = _ff_params(x, ln, w1p, b1p, w2f, b2, residual, out)
    f = p.F
    # algorithmic work: the two projections (2 M C 2F + 2 M F C)
    flops = 2.0 * m * c * 2 * f + 2.0 * m * f * c
    _launch("gemm", flops, lambda: _lib.check(_L(x).saspa_ff_block(C.byref(p), _stream()), "saspa_ff_block"),
            (m, 3 * f, c, 0, 1, 0, False, True, c) + ((GEMM_FAMILY_FF_BLOCK, 1) if _RECORDER is not None else ()))
    return out


def _attn_params(q, k, vt, out, heads, d, nq, nk, scale, causal, prescaled, v_rowmajor):
    p = _lib.AttnParams()
    p.q, p.ldq, p.sqb = _ptr(q), q.stride(1), q.stride(0)
    p.k, p.ldk, p.skb = _ptr(k), k.stride(1), k.stride(0)
    p.vt, p.ldvt, p.svb = _ptr(vt), vt.stride(1), vt.stride(0)
    p.o, p.ldo, p.sob = _ptr(out), out.stride(1), out.stride(0)
    p.batch, p.heads, p.D, p.nq, p.nk = q.shape[0], heads, d, nq, nk
    p.scale, p.causal, p.flags = float(scale), int(causal), (1 if prescaled else 0) | (2 if v_rowmajor else 0)
    return p


def flash_attn_which(q, k, vt, out, heads, d, nq, nk, causal=False, prescaled=False, v_rowmajor=False):
    """Which loop `flash_attn` would run these operands on, under the SASPA_ATTN_* knobs as they stand: saspa_flash_attn_which's packed
    plan (include/saspa_hip.h: loop 1 .. 4 in the low four bits, then the SASPA_ATTN_PLAN_* bits).  Host-side, launches nothing."""
    p = _attn_params(q, k, vt, out, heads, d, nq, nk, 1.0, causal, prescaled, v_rowmajor)
    w = int(_L(q).saspa_flash_attn_which(C.byref(p)))
    if w < 0:
        _lib.check(w, "saspa_flash_attn_which")
    return w


def flash_attn(q, k, vt, out, heads, d, nq, nk, scale, causal=False, prescaled=False, v_rowmajor=False):
    """q: [B, nq, >=heads*d] view, k: [B, nk, >=heads*d] view, vt: [B, heads*d, ldvt] (keys
    contiguous), out: [B, nq, >=heads*d] view.  bf16 only.  prescaled: q already carries scale * log2(e)
    (folded into the to_q weights, weights.ATTN_LOG2E) -> SASPA_ATTN_QPRESCALED, `scale` is ignored.
    v_rowmajor: `vt` is V itself, [B, nk, >=heads*d] like k (a view into a fused Q | K | V projection) ->
    SASPA_ATTN_V_ROWMAJOR: the kernel transposes between LDS and the MFMA, no V^T projection is needed."""
    _check_dev(q, k, vt, out)
    _same_dtype("flash_attn", q, k=k, v=vt, out=out)
    lib = _L(q)
    if not is_half(q):
        raise TypeError("flash_attn is the bf16 path; fp32 uses the unfused GEMM+softmax path")
    p = _attn_params(q, k, vt, out, heads, d, nq, nk, scale, causal, prescaled, v_rowmajor)
    _launch("flash_attn", 4.0 * q.shape[0] * heads * nq * nk * d,
            lambda: _lib.check(lib.saspa_flash_attn_bf16(C.byref(p), _stream()), "saspa_flash_attn_bf16"),
            (q.shape[0], heads, nq, nk, d))
    return out


def flash_attn_f32x3(q, k, vt, out, heads, d, nq, nk, scale, causal=False):
    """flash_attn's operands in fp32: q [B, nq, >=heads*d] view, k [B, nk, >=heads*d] view, vt [B, heads*d, ldvt >= nk] (keys
    contiguous), out [B, nq, >=heads*d] view.  One fused launch with x3 products (three bf16 MFMAs per product, counted as one
    product in the recorder's FLOPs), no score matrix; d a multiple of 8, at most 160.  Anything the library refuses raises with its
    SASPA_E* code, nothing is launched."""
    _check_dev(q, k, vt, out)
    _same_dtype("flash_attn_f32x3", q, k=k, v=vt, out=out)
    if q.dtype != torch.float32:
        raise TypeError("flash_attn_f32x3 is the fp32 path; 16-bit tensors use flash_attn")
    lib = _L(q)
    p = _attn_params(q, k, vt, out, heads, d, nq, nk, scale, causal, False, False)
    _launch("flash_attn_f32x3", 4.0 * q.shape[0] * heads * nq * nk * d,
            lambda: _lib.check(lib.saspa_flash_attn_f32x3(C.byref(p), _stream()), "saspa_flash_attn_f32x3"),
            (q.shape[0], heads, nq, nk, d))
    return out


def attn_wide(q, k, v, out, nq, nk, scale):
    """One wide head per batch entry (192 <= d <= 512, d % 64 == 0: the VAE's 512-channel mid-block attention) in one fused launch:
    q [B, nq, d], k / v [B, nk, d] and out [B, nq, d] views whose last dim is contiguous -- column slices of one fused Q | K | V
    buffer as they are; V row-major, no score matrix, no workspace.  bf16 tensors go to the default library, fp16 to the fp16 one;
    anything the library refuses (other dtypes, other widths, empty operands) raises with its SASPA_E* code, nothing is launched."""
    _check_dev(q, k, v, out)
    _same_dtype("attn_wide", q, k=k, v=v, out=out)
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"attn_wide: {name} must be [B, n, d] with a contiguous last dim, got {tuple(t.shape)} / {t.stride()}")
    b, d = q.shape[0], q.shape[2]
    lib = _L(q)
    _launch("attn_wide", 4.0 * b * nq * nk * d,
            lambda: _lib.check(lib.saspa_attn_wide(_dt(q), _ptr(q), q.stride(1), q.stride(0), _ptr(k), k.stride(1), k.stride(0),
                                                   _ptr(v), v.stride(1), v.stride(0), _ptr(out), out.stride(1), out.stride(0),
                                                   b, int(nq), int(nk), d, float(scale), _stream()), "saspa_attn_wide"),
            (b, 1, nq, nk, d))
    return out


def attn_wide_x3(q, k, v, out, nq, nk, scale):
    """attn_wide's operands in fp32 (192 <= d <= 512, d % 64 == 0): q [B, nq, d], k / v [B, nk, d] and out [B, nq, d] views whose last
    dim is contiguous -- column slices of one fused Q | K | V buffer as they are; V row-major.  One fused launch with x3 products
    (three bf16 MFMAs per product, counted as one product in the recorder's FLOPs), no score matrix, no workspace.  Anything the
    library refuses raises with its SASPA_E* code, nothing is launched."""
    _check_dev(q, k, v, out)
    _same_dtype("attn_wide_x3", q, k=k, v=v, out=out)
    if q.dtype != torch.float32:
        raise TypeError("attn_wide_x3 is the fp32 path; 16-bit tensors use attn_wide")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"attn_wide_x3: {name} must be [B, n, d] with a contiguous last dim, got {tuple(t.shape)} / {t.stride()}")
    b, d = q.shape[0], q.shape[2]
    lib = _L(q)
    _launch("attn_wide_x3", 4.0 * b * nq * nk * d,
            lambda: _lib.check(lib.saspa_attn_wide_f32x3(_ptr(q), q.stride(1), q.stride(0), _ptr(k), k.stride(1), k.stride(0),
                                                         _ptr(v), v.stride(1), v.stride(0), _ptr(out), out.stride(1), out.stride(0),
                                                         b, int(nq), int(nk), d, float(scale), _stream()), "saspa_attn_wide_f32x3"),
            (b, 1, nq, nk, d))
    return out


def _decode_attn_params(q, k, v, out, lens, heads, d, nk, group, scale):
    p = _lib.DecodeAttnParams()
    p.dtype = _dt(q)
    p.q, p.ldq = _ptr(q), q.stride(0)
    p.k, p.ldk, p.ske = _ptr(k), k.stride(1), k.stride(0)
    p.v, p.ldv, p.sve = _ptr(v), v.stride(1), v.stride(0)
    p.len = _ptr(lens)
    p.out, p.ldo = _ptr(out), out.stride(0)
    p.rows, p.entries, p.heads, p.d, p.nk, p.group = q.shape[0], k.shape[0], int(heads), int(d), int(nk), int(group)
    p.scale = float(scale)
    return p


def decode_attn(q, k, v, heads, nk, scale, *, group=1, lens=None, out=None):
    """One query per row against a key/value cache (saspa_decode_attn): q [rows, >= heads*d] view, k / v caches
    [entries, nk_max, >= heads*d] views (row-major, V not transposed), row r reads entry r // group and its keys < lens[r] (int32 on the
    device; None = all nk).  bf16 or fp32 storage, fp32 arithmetic, one rounding; -> out [rows, heads*d].  Anything the library refuses
    (d % 8, d > 128, nk > 1024, group > 8, alignment) raises with its SASPA_E* code, nothing is launched."""
    _check_dev(q, k, v, lens, out)
    _same_dtype("decode_attn", q, k=k, v=v, out=out)
    if q.dim() != 2 or k.dim() != 3 or v.dim() != 3 or q.stride(1) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("decode_attn: q must be [rows, C] and k / v [entries, nk_max, C] with a contiguous last dim")
    if k.shape[1] < nk or v.shape[1] < nk or v.shape[0] != k.shape[0]:
        raise ValueError(f"decode_attn: caches {tuple(k.shape)} / {tuple(v.shape)} do not hold {nk} keys per entry")
    if lens is not None and (lens.dtype != torch.int32 or lens.numel() < q.shape[0] or not lens.is_contiguous()):
        raise ValueError("decode_attn: lens must be a contiguous int32 tensor with one entry per row")
    c = k.shape[2]
    if c % heads or q.shape[1] < c:
        raise ValueError(f"decode_attn: {c} cache channels do not split into {heads} heads of the query's width {q.shape[1]}")
    d = c // heads
    if out is None:
        out = torch.empty((q.shape[0], c), device=q.device, dtype=q.dtype)
    p = _decode_attn_params(q, k, v, out, lens, heads, d, nk, group, scale)
    lib = _L(q)
    _launch("decode_attn", 4.0 * q.shape[0] * heads * nk * d,
            lambda: _lib.check(lib.saspa_decode_attn(C.byref(p), _stream()), "saspa_decode_attn"), (q.shape[0], heads, 1, nk, d))
    return out


def logprob_topk(logits, vocab, group, scores, ban_token=-1, ban_on=False):
    """One beam-search step's selection (saspa_logprob_topk): fp32 logits [images * group, ld >= vocab] (pad columns ignored), fp32
    running scores [images * group]; per image the 2 * group best of its group * vocab candidates log_softmax(row)[token] +
    scores[row] (ban_token at -inf while ban_on), descending, ties to the lowest row * vocab + token.
    -> (scores fp32 [images, 2*group], (row in group, token) int32 [images, 2*group, 2], buf): the first two are views of `buf`
    (int32 [3, images, 2*group]), so that the host fetches a step's selection with a single copy."""
    _check_dev(logits, scores)
    if logits.dtype != torch.float32 or scores.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logprob_topk takes fp32 logits [rows, ld] and fp32 scores")
    rows = logits.shape[0]
    if rows % group or scores.numel() != rows or not scores.is_contiguous():
        raise ValueError(f"logprob_topk: {rows} rows / {scores.numel()} scores are not whole images of {group} rows")
    if rows > group and logits.stride(0) != logits.shape[1]:
        raise ValueError("logprob_topk: the rows of the logits must be densely packed")
    images, k = rows // group, 2 * group
    buf = torch.empty((3, images, k), device=logits.device, dtype=torch.int32)
    out_score = buf[0].view(torch.float32)
    out_idx = buf[1:].view(images, k, 2)
    lib = _L()
    _launch("logprob_topk", 0.0,
            lambda: _lib.check(lib.saspa_logprob_topk(_ptr(logits), logits.stride(0) if rows > 1 else logits.shape[1], int(vocab), images,
                                                      int(group), _ptr(scores), int(ban_token), int(bool(ban_on)), _ptr(out_score),
                                                      _ptr(out_idx), _stream()), "saspa_logprob_topk"))
    return out_score, out_idx, buf


def _rmsnorm_args(x2, o2, gamma, eps):
    rows, c = x2.shape
    return (_dt(x2), _ptr(x2), x2.stride(0) if rows > 1 else max(c, x2.stride(0)), _ptr(o2),
            o2.stride(0) if rows > 1 else max(c, o2.stride(0)), rows, c, _ptr(gamma), float(eps), _stream())


def rmsnorm(x, gamma, eps=1e-6, out=None):
    """T5's RMS norm over the last dim (saspa_rmsnorm): x * rsqrt(mean(x^2) + eps) * gamma, no mean subtraction, no bias.  x [..., C]
    with a contiguous last dim and a uniform row pitch, bf16 or fp32; gamma fp32 [C].  C % 8 == 0, C <= 8192."""
    _check_dev(x, gamma, out)
    _same_dtype("rmsnorm", x, out=out)
    if gamma.dtype != torch.float32 or gamma.numel() < x.shape[-1] or not gamma.is_contiguous():
        raise ValueError("rmsnorm: gamma must be a contiguous fp32 vector of C elements")
    if x.stride(-1) != 1:
        raise ValueError("rmsnorm: the last dim must be contiguous")
    c = x.shape[-1]
    x2 = x.reshape(-1, c) if x.dim() != 2 else x
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    o2 = out.view(-1, c) if out.dim() != 2 else out
    lib = _L(_dt(x))
    _launch("rmsnorm", 0.0, lambda: _lib.check(lib.saspa_rmsnorm(*_rmsnorm_args(x2, o2, gamma, eps)), "saspa_rmsnorm"),
            (x2.shape[0], c))
    return out


def _attn_relbias_params(q, k, v, out, lens, pos, bias, center, heads, d, nk, rows_per_entry, scale):
    p = _lib.AttnRelbiasParams()
    p.dtype = _dt(q)
    p.q, p.ldq = _ptr(q), q.stride(0)
    p.k, p.ldk, p.ske = _ptr(k), k.stride(1), k.stride(0)
    p.v, p.ldv, p.sve = _ptr(v), v.stride(1), v.stride(0)
    p.len, p.pos = _ptr(lens), _ptr(pos)
    p.bias, p.ldb, p.ncol, p.center = _ptr(bias), bias.stride(0), bias.shape[1], int(center)
    p.out, p.ldo = _ptr(out), out.stride(0)
    p.rows, p.entries, p.heads, p.d, p.nk, p.rows_per_entry = q.shape[0], k.shape[0], int(heads), int(d), int(nk), int(rows_per_entry)
    p.scale = float(scale)
    return p


def attn_relbias(q, k, v, heads, nk, scale, pos, bias, center, *, rows_per_entry=1, lens=None, out=None):
    """Attention with an additive relative-position bias (saspa_attn_relbias): decode_attn's operands (q [rows, >= heads*d] view, k / v
    caches [entries, nk_max, >= heads*d] views, lens int32 per row or None) with row r reading entry r // rows_per_entry, pos int32
    [rows] on the device (the queries' positions) and bias fp32 [heads, ncol]: the logit of key j is
    scale * q.k_j + bias[head][clamp(pos[r] - j + center, 0, ncol - 1)].  -> out [rows, heads*d].  Anything the library refuses
    (d % 8, d > 128, nk > 1024, rows_per_entry > 1024, alignment) raises with its SASPA_E* code, nothing is launched."""
    _check_dev(q, k, v, lens, pos, bias, out)
    _same_dtype("attn_relbias", q, k=k, v=v, out=out)
    if q.dim() != 2 or k.dim() != 3 or v.dim() != 3 or q.stride(1) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("attn_relbias: q must be [rows, C] and k / v [entries, nk_max, C] with a contiguous last dim")
    if k.shape[1] < nk or v.shape[1] < nk or v.shape[0] != k.shape[0]:
        raise ValueError(f"attn_relbias: caches {tuple(k.shape)} / {tuple(v.shape)} do not hold {nk} keys per entry")
    for name, t in (("lens", lens), ("pos", pos)):
        if t is not None and (t.dtype != torch.int32 or t.numel() < q.shape[0] or not t.is_contiguous()):
            raise ValueError(f"attn_relbias: {name} must be a contiguous int32 tensor with one entry per row")
    if pos is None:
        raise ValueError("attn_relbias: pos (the queries' positions) is required")
    if bias.dtype != torch.float32 or bias.dim() != 2 or bias.shape[0] != heads or bias.stride(1) != 1:
        raise ValueError(f"attn_relbias: bias must be fp32 [heads = {heads}, ncol] with a contiguous last dim")
    c = k.shape[2]
    if c % heads or q.shape[1] < c:
        raise ValueError(f"attn_relbias: {c} cache channels do not split into {heads} heads of the query's width {q.shape[1]}")
    d = c // heads
    if out is None:
        out = torch.empty((q.shape[0], c), device=q.device, dtype=q.dtype)
    p = _attn_relbias_params(q, k, v, out, lens, pos, bias, center, heads, d, nk, rows_per_entry, scale)
    lib = _L(p.dtype)
    _launch("attn_relbias", 4.0 * q.shape[0] * heads * nk * d,
            lambda: _lib.check(lib.saspa_attn_relbias(C.byref(p), _stream()), "saspa_attn_relbias"), (q.shape[0], heads, 1, nk, d))
    return out


def _sample_topk_args(logits, vocab, temperature, top_k, top_p, u, tok, logp):
    rows = logits.shape[0]
    return (_ptr(logits), logits.stride(0) if rows > 1 else logits.shape[1], int(vocab), rows, float(temperature), int(top_k),
            float(top_p), _ptr(u), _ptr(tok), _ptr(logp), _stream())


def sample_topk(logits, vocab, u, *, temperature=1.0, top_k=50, top_p=1.0):
    """One sampling step (saspa_sample_topk): fp32 logits [rows, ld >= vocab] (pad columns ignored), u fp32 [rows] uniforms in [0, 1)
    on the device; temperature -> top-k (<= 64, clamped to vocab; ties to the lowest id) -> top-p -> inverse-CDF draw on u.
    -> (token int32 [rows], log-probability under the kept distribution fp32 [rows], buf): the first two are views of `buf` (int32
    [2, rows]), so that the host fetches a step's result with a single copy.  top_k = 1 is greedy."""
    _check_dev(logits, u)
    if logits.dtype != torch.float32 or u.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("sample_topk takes fp32 logits [rows, ld] and fp32 uniforms")
    rows = logits.shape[0]
    if u.numel() != rows or not u.is_contiguous():
        raise ValueError(f"sample_topk: {u.numel()} uniforms for {rows} rows")
    if logits.shape[1] < vocab:
        raise ValueError(f"sample_topk: rows of {logits.shape[1]} columns do not hold a vocabulary of {vocab}")
    buf = torch.empty((2, rows), device=logits.device, dtype=torch.int32)
    tok, logp = buf[0], buf[1].view(torch.float32)
    lib = _L()
    _launch("sample_topk", 0.0,
            lambda: _lib.check(lib.saspa_sample_topk(*_sample_topk_args(logits, vocab, temperature, top_k, top_p, u, tok, logp)),
                               "saspa_sample_topk"), (rows, int(vocab), int(top_k)))
    return tok, logp, buf


def softmax_rows(x, n, scale, causal=False, rows_per_mat=1):
    """In-place softmax(scale*x) over the first n columns of [rows, ld]; pad columns zeroed."""
    _check_dev(x)
    lib = _L(x)
    x2 = x.view(-1, x.shape[-1])
    _lib.check(lib.saspa_softmax_rows(_dt(x), _ptr(x2), x2.shape[0], n, x2.stride(0), float(scale), int(causal),
                                      int(rows_per_mat), _stream()), "saspa_softmax_rows")
    return x


def groupnorm(x, gamma, beta, groups, eps, act=ACT_NONE, x2=None, out=None):
    """GroupNorm(+SiLU) over channels-last x (optionally concatenated with x2) -> [B,H,W,C]."""
    _check_dev(x, gamma, beta, x2, out)
    lib = _L(x)
    b, h, w, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    ctot = c0 + c1
    if x2 is not None and (tuple(x2.shape[:3]) != (b, h, w) or x2.dtype != x.dtype):
        raise ValueError(f"concat source {tuple(x2.shape)} does not match {tuple(x.shape)}")
    if gamma.numel() < ctot or beta.numel() < ctot or ctot % groups:
        raise ValueError("GroupNorm parameters / groups do not match the channel count")
    if out is not None and (tuple(out.shape[:3]) != (b, h, w) or out.shape[3] < ctot or out.dtype != x.dtype):
        raise ValueError("GroupNorm output does not match the input geometry")
    if out is None:
        out = torch.empty((b, h, w, ctot), device=x.device, dtype=x.dtype)
    stats = _epilogue_stats(x, x2, groups)
    p = _gn_params(x, x2, gamma, beta, groups, eps, act, out, stats=stats)
    s = _stream()
    if stats[0] is not None:
        # statistics left by the producers' epilogues (conv(..., gn_unit=...)): no statistics pass
        _lib.check(lib.saspa_groupnorm_apply(C.byref(p), s), "saspa_groupnorm_apply(epilogue statistics)")
        return out
    # small images (the 8x8 level: no 128-row statistics blocks): statistics + apply in one launch
    if gn_onepass_enabled() and lib.saspa_groupnorm_onepass_eligible(C.byref(p)):
        _lib.check(lib.saspa_groupnorm_onepass(C.byref(p), s), "saspa_groupnorm_onepass")
        return out
    nsplit = _gn_nsplit(b, h * w, ctot // 8)
    partial = torch.empty((b * nsplit * ctot * 2,), device=x.device, dtype=torch.float32)
    p.partial, p.nsplit = _ptr(partial), nsplit
    _lib.check(lib.saspa_groupnorm_stats(C.byref(p), s), "saspa_groupnorm_stats")
    _lib.check(lib.saspa_groupnorm_apply(C.byref(p), s), "saspa_groupnorm_apply")
    return out


def groupnorm_quant_mxfp8(x, gamma, beta, groups, eps, act=ACT_NONE, x2=None):
    """GroupNorm(+SiLU) over channels-last bf16 x (optionally concatenated with x2), quantised to MX-fp8 for conv3x3_mxfp8 ->
    (q uint8 [B,H,W,C] e4m3 bytes, qs uint8 [B,H,W,C/32] E8M0 exponents of each pixel's 32-channel blocks):
    `saspa_groupnorm_quant_mxfp8`.  Statistics as `groupnorm` finds them (the producers' epilogues, else a statistics pass)."""
    _check_dev(x, gamma, beta, x2)
    lib = _L()
    b, h, w, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[3]
    ctot = c0 + c1
    if x.dtype != torch.bfloat16 or (x2 is not None and x2.dtype != x.dtype):
        raise TypeError("the MX-fp8 path takes bf16 activations")
    if x2 is not None and tuple(x2.shape[:3]) != (b, h, w):
        raise ValueError(f"concat source {tuple(x2.shape)} does not match {tuple(x.shape)}")
    if gamma.numel() < ctot or beta.numel() < ctot or ctot % groups:
        raise ValueError("GroupNorm parameters / groups do not match the channel count")
    q = torch.empty((b, h, w, ctot), device=x.device, dtype=torch.uint8)
    qs = torch.empty((b, h, w, ctot // 32), device=x.device, dtype=torch.uint8)
    stats = _epilogue_stats(x, x2, groups)
    p = _gn_params(x, x2, gamma, beta, groups, eps, act, None, stats=stats)
    s = _stream()
    if stats[0] is None:
        # pixel splits fixed per image (not _gn_nsplit's share of ~1024 workgroups over the batch): an image's statistics, and so its
        # bytes, do not depend on the batch it is quantised in
        nsplit = max(1, min(64, h * w // 16))
        partial = torch.empty((b * nsplit * ctot * 2,), device=x.device, dtype=torch.float32)
        p.partial, p.nsplit = _ptr(partial), nsplit
        _lib.check(lib.saspa_groupnorm_stats(C.byref(p), s), "saspa_groupnorm_stats")
    _lib.check(lib.saspa_groupnorm_quant_mxfp8(C.byref(p), _ptr(q), ctot, _ptr(qs), ctot // 32, s), "saspa_groupnorm_quant_mxfp8")
    return q, qs


def _conv_mx_params(q, qs, w8, sw, bias, rowvec, residual, out):
    b, h, w, c = q.shape
    p = _lib.ConvMxParams()
    p.q, p.ldq, p.qs, p.ldqs = _ptr(q), c, _ptr(qs), qs.shape[-1]
    p.batch, p.h, p.w, p.C = b, h, w, c
    p.kh, p.kw, p.stride, p.pad, p.upsample = 3, 3, 1, 1, 0
    p.w8, p.ldw, p.N, p.Kp = _ptr(w8), w8.shape[1], w8.shape[0], w8.shape[1]
    p.sw, p.bias = _ptr(sw), _ptr(bias)
    p.rowvec, p.ldrv = _ptr(rowvec), _ldrv(rowvec)
    n = w8.shape[0]
    p.residual, p.ldr = _ptr(residual), (0 if residual is None else _pitch4(residual))
    p.out, p.ldo = _ptr(out), n
    return p


def conv3x3_mxfp8_eligible(c, n, h=64, w=64, batch=1):
    """Shapes saspa_conv3x3_mxfp8 runs (3x3 / stride 1 / pad 1 of c channels into n): the library's own host-side answer."""
    p = _lib.ConvMxParams()
    p.batch, p.h, p.w, p.C, p.kh, p.kw, p.stride, p.pad = batch, h, w, c, 3, 3, 1, 1
    p.N, p.Kp = n, (9 * c + 127) // 128 * 128
    p.ldq, p.ldqs, p.ldw, p.ldo = c, c // 32, p.Kp, n
    return bool(_lib.load().saspa_conv3x3_mxfp8_eligible(C.byref(p)))


def conv3x3_mxfp8(q, qs, w8, sw, bias=None, rowvec=None, residual=None, gn_unit=None):
    """3x3 / stride 1 / pad 1 conv of MX-fp8 activations (groupnorm_quant_mxfp8's (q, qs)) with e4m3 weights
    (weights.pack_conv_mxfp8's (w8, sw)) -> bf16 [B,H,W,N]: `saspa_conv3x3_mxfp8`.  out = bf16(sw * sum + bias + rowvec[b])
    (+ residual); gn_unit: leave the GroupNorm statistics of the output for the next GroupNorm / quantiser (as `conv`)."""
    _check_dev(q, qs, w8, sw, bias, rowvec, residual)
    b, h, w, c = q.shape
    n, kp = w8.shape
    if kp != (9 * c + 127) // 128 * 128:
        raise ValueError(f"weights {tuple(w8.shape)} are not weights.pack_conv_mxfp8 of a 3x3 conv over {c} channels")
    if q.dtype != torch.uint8 or qs.dtype != torch.uint8 or w8.dtype != torch.uint8 or tuple(qs.shape) != (b, h, w, c // 32):
        raise TypeError("conv3x3_mxfp8 takes uint8 e4m3 bytes / E8M0 exponents")
    if not (q.is_contiguous() and qs.is_contiguous() and w8.is_contiguous()):
        raise ValueError("conv3x3_mxfp8 operands must be dense")
    if residual is not None and (tuple(residual.shape) != (b, h, w, n) or residual.dtype != torch.bfloat16):
        raise ValueError(f"residual {tuple(residual.shape)} does not match the output [{b},{h},{w},{n}]")
    out = torch.empty((b, h, w, n), device=q.device, dtype=torch.bfloat16)
    for name, t in (("sw", sw), ("bias", bias)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous()):
            raise ValueError(f"{name} must be a dense fp32 [{n}] vector (got {tuple(t.shape)} {t.dtype})")
    if rowvec is not None and (rowvec.dtype != torch.float32 or rowvec.dim() > 2 or rowvec.stride(-1) != 1 or rowvec.shape[-1] != n
                               or (rowvec.dim() == 2 and rowvec.shape[0] not in (1, b))):
        raise ValueError(f"rowvec {tuple(rowvec.shape)} {rowvec.dtype} is not fp32 [1 or {b}, {n}] with dense rows")
    p = _conv_mx_params(q, qs, w8, sw, bias, rowvec, residual, out)
    m = b * h * w
    _gn_stats_for(p, out, gn_unit, b, h * w, n)
    _launch("gemm", 2.0 * m * n * 9 * c, lambda: _lib.check(_L().saspa_conv3x3_mxfp8(C.byref(p), _stream()), "saspa_conv3x3_mxfp8"),
            (m, n, 9 * c, 3, 1, 0, False, residual is not None, n, GEMM_FAMILY_MXFP8_CONV, 1))
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _check_dev(x, gamma, beta, out)
    lib = _L(x)
    c = x.shape[-1]
    x2 = x.reshape(-1, c)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    o2 = out.view(-1, c)
    rows = x2.shape[0]
    _lib.check(lib.saspa_layernorm(_dt(x), _ptr(x2), x2.stride(0) if rows > 1 else c, _ptr(o2),
                                   o2.stride(0) if rows > 1 else c, rows, c, _ptr(gamma), _ptr(beta), float(eps),
                                   _stream()), "saspa_layernorm")
    return out


def layernorm_quant_fp8(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last dim of bf16 x, quantised per row to e4m3 -> (q uint8 [..., C], scale fp32 [rows])."""
    _check_dev(x, gamma, beta)
    if x.dtype != torch.bfloat16:
        raise TypeError("the fp8 path takes bf16 activations")
    c = x.shape[-1]
    x2 = x.reshape(-1, c)
    rows = x2.shape[0]
    q = torch.empty((rows, c), device=x.device, dtype=torch.uint8)
    scale = torch.empty((rows,), device=x.device, dtype=torch.float32)
    _lib.check(_L().saspa_layernorm_quant_fp8(_ptr(x2), x2.stride(0) if rows > 1 else c, _ptr(q), c, _ptr(scale), rows, c,
                                                     _ptr(gamma), _ptr(beta), float(eps), _stream()), "saspa_layernorm_quant_fp8")
    return q.view(*x.shape[:-1], c), scale


def _gemm_f8_params(x2, wq, wscale, bias, residual, act, out):
    """SaspaGemmF8Params of e4m3 rows x2 [M, K] @ wq [N, K]^T into the dense rows of `out`; the activation scales (per row, one
    value, or MX block exponents) are the caller's."""
    m, k = x2.shape
    r2 = None if residual is None else residual.reshape(-1, residual.shape[-1])
    p = _lib.GemmF8Params()
    p.a, p.lda, p.w, p.ldw = _ptr(x2), x2.stride(0) if m > 1 else k, _ptr(wq), wq.stride(0)
    p.M, p.N, p.K = m, wq.shape[0], k
    p.sw, p.bias = _ptr(wscale), _ptr(bias)
    p.residual, p.ldr = _ptr(r2), 0 if r2 is None else r2.stride(0)
    p.act, p.out, p.ldo = int(act), _ptr(out), out.shape[1]
    return p


def linear_fp8(xq, xscale, wq, wscale, bias=None, *, residual=None, act=ACT_NONE, out_fp8_scale=None, amax=None, out_mx=False):
    """e4m3 activations (uint8 [..., K] + per-row scale, or ONE scale for the whole tensor: a 1-element `xscale`) @ e4m3 weights
    (uint8 [N, K] + per-channel scale)^T -> bf16 [..., N] (N / 2 with the fused GEGLU): `saspa_gemm_fp8`.
    GEGLU only (ABI 20): `out_fp8_scale` (device fp32 scalar) makes the result e4m3 bytes under that tensor-wide scale -- uint8
    [..., N / 2], what the feed-forward output projection reads --, `amax` (device fp32 scalar) receives the atomic maximum of the
    gated values' magnitudes (calibration of that scale).
    GEGLU only, instead of those two: `out_mx=True` returns (q, qs), the gated values as MX e4m3 -- q uint8 [..., N / 2], qs uint8
    [rows, N / 64] E8M0 exponents, one per row and 32 columns -- for `linear_mxfp8`: `saspa_gemm_fp8_geglu_mx`, no calibrated scale."""
    _check_dev(xq, xscale, wq, wscale, bias, residual, out_fp8_scale, amax)
    k = xq.shape[-1]
    x2 = xq.reshape(-1, k)
    m, n = x2.shape[0], wq.shape[0]
    nout = n // 2 if act == ACT_GEGLU else n
    if (out_fp8_scale is not None or amax is not None) and act != ACT_GEGLU:
        raise ValueError("fp8 emission / amax exist in the GEGLU epilogue only")
    if out_mx and (act != ACT_GEGLU or out_fp8_scale is not None or amax is not None):
        raise ValueError("out_mx exists in the GEGLU epilogue only, and not together with out_fp8_scale / amax")
    out = torch.empty((m, nout), device=xq.device, dtype=torch.uint8 if (out_fp8_scale is not None or out_mx) else torch.bfloat16)
    p = _gemm_f8_params(x2, wq, wscale, bias, residual, act, out)
    p.sa = _ptr(xscale)
    if xscale.numel() == 1 and m > 1:
        p.sa_broadcast = 1
    elif xscale.numel() < m:
        raise ValueError(f"{xscale.numel()} activation scales for {m} rows")
    if out_fp8_scale is not None:
        if out_fp8_scale.dtype != torch.float32 or out_fp8_scale.numel() != 1:
            raise ValueError("out_fp8_scale is one fp32 value on the device")
        p.out_fp8, p.out_scale = 1, _ptr(out_fp8_scale)
    if amax is not None:
        if amax.dtype != torch.float32 or amax.numel() != 1:
            raise ValueError("amax is one fp32 value on the device")
        p.amax = _ptr(amax)
    if out_mx:
        ldqs = (n // 64 + 3) & ~3                  # a row's exponents start on a dword (the consumer's K-tile of 4 is one)
        qs = torch.empty((m, ldqs), device=xq.device, dtype=torch.uint8)[:, :n // 64]
        _launch("gemm", 2.0 * m * n * k,
                lambda: _lib.check(_L().saspa_gemm_fp8_geglu_mx(C.byref(p), _ptr(qs), ldqs, _stream()), "saspa_gemm_fp8_geglu_mx"),
                (m, n, k, 0, 1, 0, False, False, nout, GEMM_FAMILY_FP8, 1))
        return out.reshape(*xq.shape[:-1], nout), qs
    _launch("gemm", 2.0 * m * n * k, lambda: _lib.check(_L().saspa_gemm_fp8(C.byref(p), _stream()), "saspa_gemm_fp8"),
            (m, n, k, 0, 1, 0, False, residual is not None, nout, GEMM_FAMILY_FP8, 1))
    return out.reshape(*xq.shape[:-1], nout)


def linear_mxfp8(q, qs, wq, wscale, bias=None, *, residual=None):
    """MX e4m3 activations (`linear_fp8(..., out_mx=True)`'s (q uint8 [..., K], qs uint8 [rows, >= K / 32] E8M0 exponents, one per
    row and 32 columns)) @ e4m3 weights (uint8 [N, K] + per-channel scale)^T -> bf16 [..., N]: `saspa_gemm_mxfp8`, the exponents
    applied inside the scaled MFMA.  The feed-forward output projection of the calibration-free fp8 mode."""
    _check_dev(q, qs, wq, wscale, bias, residual)
    if q.dtype != torch.uint8 or qs.dtype != torch.uint8 or wq.dtype != torch.uint8:
        raise TypeError("linear_mxfp8 takes uint8 e4m3 bytes / E8M0 exponents")
    k = q.shape[-1]
    x2 = q.reshape(-1, k)
    m, n = x2.shape[0], wq.shape[0]
    if qs.dim() != 2 or qs.shape[0] != m or qs.shape[1] < k // 32 or qs.stride(1) != 1:
        raise ValueError(f"block exponents {tuple(qs.shape)} do not cover {m} rows of {k // 32} blocks")
    out = torch.empty((m, n), device=q.device, dtype=torch.bfloat16)
    p = _gemm_f8_params(x2, wq, wscale, bias, residual, ACT_NONE, out)
    ldqs = qs.stride(0) if m > 1 else (k // 32 + 3) & ~3      # one row: the pitch is never used
    _launch("gemm", 2.0 * m * n * k, lambda: _lib.check(_L().saspa_gemm_mxfp8(C.byref(p), _ptr(qs), ldqs, _stream()), "saspa_gemm_mxfp8"),
            (m, n, k, 0, 1, 0, False, residual is not None, n, GEMM_FAMILY_FP8, 1))
    return out.reshape(*q.shape[:-1], n)


def fp8_pow2_scale(amax, margin=16.0):
    """Tensor-wide e4m3 scale from a calibration maximum (device fp32 scalar -> device fp32 scalar, no host sync): the power of two
    >= margin * amax / 448.  e4m3 is a floating format: a power-of-two scale shifts exponents only, so the quantised values do not
    depend on the calibration batch as long as nothing overflows (the margin: 4 binades; the conversion saturates beyond) or
    underflows (values below scale * 2^-9 ~ 1e-4 of the calibration maximum flush to zero)."""
    a = amax.float().reshape(1)
    s = torch.exp2(torch.ceil(torch.log2((a * (margin / 448.0)).clamp_min(2.0 ** -60))))
    return torch.where(a > 0, s, torch.ones_like(s))


def geglu(x, out=None):
    """x: [..., 2F] -> [..., F] = x[..., :F] * gelu_erf(x[..., F:])"""
    _check_dev(x, out)
    lib = _L(x)
    f = x.shape[-1] // 2
    x2 = x.reshape(-1, 2 * f)
    if out is None:
        out = torch.empty((*x.shape[:-1], f), device=x.device, dtype=x.dtype)
    o2 = out.view(-1, f)
    _lib.check(lib.saspa_geglu(_dt(x), _ptr(x2), x2.stride(0), _ptr(o2), o2.stride(0), x2.shape[0], f, _stream()),
               "saspa_geglu")
    return out


def activation(x, act, out=None):
    _check_dev(x, out)
    lib = _L(x)
    c = x.shape[-1]
    x2 = x.reshape(-1, c)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    o2 = out.view(-1, c)
    rows = x2.shape[0]
    _lib.check(lib.saspa_activation(_dt(x), int(act), _ptr(x2), x2.stride(0) if rows > 1 else c, _ptr(o2),
                                    o2.stride(0) if rows > 1 else c, rows, c, _stream()), "saspa_activation")
    return out


def pool2d(x, k, stride=None, pad=0, mode="avg"):
    """nn.MaxPool2d(k, stride, pad) / nn.AvgPool2d(k) over channels-last x [B,H,W,C] -> [B,Ho,Wo,C]."""
    _check_dev(x)
    stride = k if stride is None else stride
    b, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.empty((b, ho, wo, c), device=x.device, dtype=x.dtype)
    _lib.check(_L().saspa_pool2d(_dt(x), 0 if mode == "max" else 1, _ptr(x), _pitch4(x), _ptr(out), c, b, h, w, c, int(k),
                                        int(stride), int(pad), _stream()), "saspa_pool2d")
    return out


def signsqrt_l2norm(x, eps, scale=1.0):
    """rows of fp32 [R, C]: scale * normalize(sign(x) * sqrt(|x| + eps)) (WSDAN bilinear attention pooling tail)."""
    _check_dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("signsqrt_l2norm expects an fp32 [rows, C] matrix")
    out = torch.empty((x.shape[0], x.shape[1]), device=x.device, dtype=torch.float32)
    _lib.check(_L().saspa_signsqrt_l2norm(_ptr(x), x.stride(0), _ptr(out), out.stride(0), x.shape[0], x.shape[1], float(eps),
                                                 float(scale), _stream()), "saspa_signsqrt_l2norm")
    return out


def lpips_layer(a, r, ref_index, w, dist=None, accumulate=False, workspace=None):
    """One LPIPS level (saspa_lpips_layer): a [n, ..., C] / r [m, ..., C] channels-last features of the same dtype and pixel count
    (the conv outputs as they are: any pixel pitch >= C), ref_index device int32 [n] (values in [0, m): the CALLER's guarantee, the
    kernel does not look), w fp32 [C] >= 0 -> fp32 [n]:  dist (+)= mean_p sum_c w_c (a_hat - r_hat[ref_index])^2."""
    _check_dev(a, r, ref_index, w, dist, workspace)
    if r.dim() != a.dim() or a.dtype != r.dtype or tuple(a.shape[1:]) != tuple(r.shape[1:]):
        raise ValueError(f"feature maps {tuple(a.shape)} {a.dtype} / {tuple(r.shape)} {r.dtype} do not pair up")
    n, m, c = a.shape[0], r.shape[0], a.shape[-1]
    if n <= 0 or m <= 0:
        raise ValueError("empty batch")

    def rows(t):
        if t.dim() not in (3, 4):
            raise ValueError("features must be [n, hw, C] or [n, h, w, C]")
        t4 = t.unsqueeze(1) if t.dim() == 3 else t
        return _pitch4(t4), t4.shape[1] * t4.shape[2]
    (lda, hw), (ldr, _) = rows(a), rows(r)
    if ref_index.dtype != torch.int32 or ref_index.dim() != 1 or ref_index.numel() != n or not ref_index.is_contiguous():
        raise ValueError("ref_index must be a contiguous int32 [n] device tensor")
    if w.dtype != torch.float32 or w.numel() != c or not w.is_contiguous():
        raise ValueError(f"w must be a contiguous fp32 [{c}] vector")
    if c % 8 or c > _lib.LPIPS_MAX_C:
        raise ValueError(f"C = {c}: the kernel takes multiples of 8 up to {_lib.LPIPS_MAX_C}")
    if dist is None:
        if accumulate:
            raise ValueError("accumulate needs the vector to add to")
        dist = torch.empty((n,), device=a.device, dtype=torch.float32)
    elif dist.dtype != torch.float32 or dist.numel() != n or not dist.is_contiguous():
        raise ValueError("dist must be a contiguous fp32 [n] vector")
    if workspace is None:
        workspace = torch.empty((n * _lib.LPIPS_MAX_BLOCKS,), device=a.device, dtype=torch.float32)
    elif workspace.dtype != torch.float32 or workspace.numel() < n * _lib.LPIPS_MAX_BLOCKS or not workspace.is_contiguous():
        raise ValueError(f"workspace must hold n * {_lib.LPIPS_MAX_BLOCKS} fp32")
    _lib.check(_L().saspa_lpips_layer(_dt(a), _ptr(a), lda, _ptr(r), ldr, _ptr(ref_index), _ptr(w), _ptr(dist), _ptr(workspace), n, hw,
                                      c, int(bool(accumulate)), _stream()), "saspa_lpips_layer")
    return dist


def class_head(feat, labels, cls=None, scale=1.0, normalize=True, width=None, want_logits=False):
    """The class head of a filter decision (saspa_class_head), one launch per batch.  Embedding mode (`cls` fp32 [C, D'] unit text rows):
    feat fp32 [n, D'] unnormalised embeddings, z = scale * unit(feat) @ cls^T over the first `width` (default: all) columns.  Logits mode
    (`cls` None): feat fp32 [n, C'] holds the logits, z = scale * feat[:, :width].  labels: device int32 [n], values in [0, C) -- the
    CALLER checks them; the kernel answers a label outside the range with NaN statistics and -1 indices.
    -> (stats fp32 [n, 4] = z_label, softmax(z)[label], max z, logsumexp z;  idx int32 [n, 2] = argmax (lowest index of equal logits),
    number of logits strictly greater than z_label;  logits fp32 [n, C] or None)."""
    _check_dev(feat, labels, cls)
    if feat.dtype != torch.float32 or feat.dim() != 2 or feat.stride(1) != 1:
        raise ValueError("class_head expects an fp32 [rows, width] matrix with a contiguous last dim")
    n = feat.shape[0]
    d = int(feat.shape[1] if width is None else width)
    if n < 1 or d < 1 or d > feat.shape[1]:
        raise ValueError(f"class_head: {n} rows of width {d} out of a [{n}, {feat.shape[1]}] matrix")
    if labels.dtype != torch.int32 or labels.dim() != 1 or labels.numel() != n or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int32 [rows] device tensor")
    ldc = 0
    if cls is not None:
        if cls.dtype != torch.float32 or cls.dim() != 2 or cls.stride(1) != 1 or cls.shape[1] < d:
            raise ValueError(f"cls must be an fp32 [C, >= {d}] matrix with a contiguous last dim")
        c = cls.shape[0]
        ldc = cls.stride(0) if c > 1 else (d + 3) // 4 * 4
    else:
        c = d
    if d > _lib.CLASS_HEAD_MAX_D or c > _lib.CLASS_HEAD_MAX_C:
        raise ValueError(f"class_head holds a row of at most {_lib.CLASS_HEAD_MAX_D} features and {_lib.CLASS_HEAD_MAX_C} classes in LDS, got {d} / {c}")
    stats = torch.empty((n, 4), device=feat.device, dtype=torch.float32)
    idx = torch.empty((n, 2), device=feat.device, dtype=torch.int32)
    ldl = (c + 3) // 4 * 4
    logits = torch.empty((n, ldl), device=feat.device, dtype=torch.float32) if want_logits else None
    ldf = feat.stride(0) if n > 1 else (d + 3) // 4 * 4                      # one row: its pitch is never used
    _lib.check(_L().saspa_class_head(_ptr(feat), ldf, _ptr(cls), ldc, _ptr(labels), float(scale),
                                     int(bool(normalize)), _ptr(stats), _ptr(idx), _ptr(logits), ldl, n, d, c, _stream()), "saspa_class_head")
    return stats, idx, (logits[:, :c] if want_logits else None)


def filter_record(table, slots, sem=None, conf=None, pc=None, bad=None, n_prompts=None):
    """One score record per image of a batch into rows `slots` of the run's table (saspa_filter_record; the fields are listed in
    include/saspa_hip.h).  table: device fp32 [n_rows, 8], contiguous.  slots: HOST ints, one per image -- checked here, before anything
    is uploaded: in [0, n_rows) and distinct (two images of a batch must never share a row).  sem: fp32 [n, >= P] semantic logits with a
    contiguous last dim (`n_prompts` = P, default: every column; P <= 64); conf / pc: the (stats, idx) pairs of the classifier's and of
    the per-class filter's `class_head` launch; bad: device bool [n], True = the image gets valid = 0.  Each of the three inputs may be
    None: that filter is off, its fields stay NaN.  Stream-ordered; nothing here waits for the GPU.  -> table."""
    import numpy as np
    _check_dev(table, sem, bad, *(conf or ()), *(pc or ()))
    f = _lib.FILTER_RECORD_FIELDS
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != f or not table.is_contiguous() or table.shape[0] < 1:
        raise ValueError(f"filter_record: the table is a contiguous fp32 [n_rows, {f}] device tensor")
    n_rows = table.shape[0]
    sl = np.asarray(slots)
    if sl.ndim != 1 or sl.size < 1 or sl.dtype.kind not in "iu":
        raise ValueError("filter_record: slots are a non-empty 1-D sequence of host integers")
    sl = sl.astype(np.int64)
    n = sl.size
    if sl.min() < 0 or sl.max() >= n_rows:
        raise ValueError(f"filter_record: slots must lie in [0, {n_rows}), got [{sl.min()}, {sl.max()}]")
    if np.unique(sl).size != n:
        raise ValueError("filter_record: two images of a batch share a slot")
    ld = p = 0
    if sem is not None:
        if sem.dtype != torch.float32 or sem.dim() != 2 or sem.shape[0] != n or sem.stride(1) != 1:
            raise ValueError(f"filter_record: sem is an fp32 [{n}, P] matrix with a contiguous last dim")
        p = int(sem.shape[1] if n_prompts is None else n_prompts)
        if p < 1 or p > sem.shape[1] or p > _lib.FILTER_RECORD_MAX_P:
            raise ValueError(f"filter_record: one lane per prompt, 1 <= P <= {min(_lib.FILTER_RECORD_MAX_P, sem.shape[1])}, got {p}")
        ld = sem.stride(0) if n > 1 else sem.shape[1]
    for name, pair in (("conf", conf), ("pc", pc)):
        if pair is None:
            continue
        st, ix = pair
        if st.dtype != torch.float32 or tuple(st.shape) != (n, 4) or not st.is_contiguous():
            raise ValueError(f"filter_record: {name} stats are the contiguous fp32 [{n}, 4] of class_head")
        if ix.dtype != torch.int32 or tuple(ix.shape) != (n, 2) or not ix.is_contiguous():
            raise ValueError(f"filter_record: {name} idx are the contiguous int32 [{n}, 2] of class_head")
    if bad is not None and (bad.dtype != torch.bool or tuple(bad.shape) != (n,) or not bad.is_contiguous()):
        raise ValueError(f"filter_record: bad is a contiguous bool [{n}] device tensor")
    slot_d = h2d(torch.from_numpy(sl.astype(np.int32)), table.device)
    cs, ci = conf if conf is not None else (None, None)
    ps, pi = pc if pc is not None else (None, None)
    _lib.check(_L().saspa_filter_record(_ptr(sem), ld, p, _ptr(cs), _ptr(ci), _ptr(ps), _ptr(pi), _ptr(bad), _ptr(slot_d), _ptr(table),
                                        n_rows, n, _stream()), "saspa_filter_record")
    return table


def u8_luma(img_u8):
    """PIL convert("L").convert("RGB") of a device u8 [..., 3] tensor (saspa_u8_luma; integer exact)."""
    _check_dev(img_u8)
    if img_u8.dtype != torch.uint8 or img_u8.dim() < 1 or img_u8.shape[-1] != 3 or not img_u8.is_contiguous() or img_u8.numel() == 0:
        raise ValueError("u8_luma expects a contiguous, non-empty u8 [..., 3] tensor")
    out = torch.empty_like(img_u8)
    _lib.check(_L().saspa_u8_luma(_ptr(img_u8), _ptr(out), img_u8.numel() // 3, _stream()), "saspa_u8_luma")
    return out


def png_deflate(images_u8):
    """Device u8 [n, H, W, C] (C = 3 or 1; [n, H, W] counts as C = 1) -> (streams u8 [n, capacity], sizes int32 [n]): per image the zlib
    stream of its PNG-filtered rows in streams[i, :sizes[i]] (saspa_png_deflate: adaptive row filters + Huffman-only deflate; pngenc.frame
    turns it into the file).  Stream-ordered, nothing here waits for the GPU; the bytes past sizes[i] are unspecified."""
    _check_dev(images_u8)
    if images_u8.dim() == 3:
        images_u8 = images_u8[..., None]
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or not images_u8.is_contiguous() or images_u8.numel() == 0:
        raise ValueError("png_deflate expects a contiguous, non-empty u8 [n, H, W, C] tensor")
    n, h, w, c = images_u8.shape
    lib = _L()
    cap, work = int(lib.saspa_png_capacity(h, w, c)), int(lib.saspa_png_workspace(n, h, w, c))
    _lib.check(min(cap, work, 0), f"saspa_png_capacity / saspa_png_workspace({n}, {h}, {w}, {c})")
    streams = torch.empty((n, cap), device=images_u8.device, dtype=torch.uint8)
    sizes = torch.empty((n,), device=images_u8.device, dtype=torch.int32)
    workspace = torch.empty((work,), device=images_u8.device, dtype=torch.uint8)
    _lib.check(lib.saspa_png_deflate(_ptr(images_u8), n, h, w, c, _ptr(streams), cap, _ptr(sizes), _ptr(workspace), work, _stream()),
               "saspa_png_deflate")
    return streams, sizes


def embed_tokens(ids, tok, pos, npos):
    _check_dev(ids, tok, pos)
    lib = _L(tok)
    n = ids.numel()
    c = tok.shape[1]
    out = torch.empty((n, c), device=tok.device, dtype=tok.dtype)
    ids32 = ids.reshape(-1).to(torch.int32)
    _lib.check(lib.saspa_embed_tokens(_dt(tok), _ptr(ids32), n, npos, _ptr(tok), _ptr(pos), c, _ptr(out), _stream()),
               "saspa_embed_tokens")
    return out


def embed_tokens_ctx(ids, ctx, ctx_begin, tok, pos):
    """ids [B, ntok] prompt tokens, ctx [B, nctx, C] (or None) spliced in at `ctx_begin`
    -> [B, ntok + nctx, C] = token embeddings + position embeddings (ContextCLIPTextEmbeddings)."""
    _check_dev(ids, ctx, tok, pos)
    lib = _L(tok)
    b, ntok = ids.shape
    c = tok.shape[1]
    nctx = 0 if ctx is None else ctx.shape[1]
    if ctx is not None:
        if ctx.shape[0] != b or ctx.shape[2] != c or ctx.dtype != tok.dtype:
            raise ValueError("ctx must be [B, nctx, C] in the embedding dtype")
        ctx = ctx.contiguous()
    if ntok + nctx > pos.shape[0]:
        raise ValueError("sequence longer than the position table")
    out = torch.empty((b, ntok + nctx, c), device=tok.device, dtype=tok.dtype)
    ids32 = ids.reshape(-1).to(torch.int32)
    _lib.check(lib.saspa_embed_tokens_ctx(_dt(tok), _ptr(ids32), b, ntok, _ptr(ctx), nctx, int(ctx_begin), _ptr(tok), _ptr(pos), c,
                                          _ptr(out), _stream()), "saspa_embed_tokens_ctx")
    return out


def cfg_plms_step(eps, x, hist, sample, nimg, hw, c, guidance, store_slot, w_cur, w_hist, coef_sample, coef_model):
    """eps, x: [2*nimg, hw, 8]; hist: [4, nimg, hw, 8] history of CFG-combined outputs; sample: [nimg, hw, 8] or None.
    One PNDM/PLMS update (see saspa_cfg_plms_step); updates x (both CFG halves) and hist[store_slot] in place."""
    _check_dev(eps, x, hist, sample)
    lib = _L(x)
    wh = (C.c_float * 4)(*[float(v) for v in w_hist])
    _lib.check(lib.saspa_cfg_plms_step(_dt(x), _ptr(eps), _ptr(x), _ptr(hist), _ptr(sample), nimg, hw, c, 8, float(guidance),
                                       int(store_slot), float(w_cur), wh, float(coef_sample), float(coef_model), _stream()),
               "saspa_cfg_plms_step")
    return x


def cfg_ddim_step(eps, x, nimg, hw, c, guidance, sa_t, s1m_t, sa_p, s1m_p):
    """eps, x: [2*nimg, hw, 8]; updates x (both CFG halves) in place."""
    _check_dev(eps, x)
    lib = _L(x)
    _lib.check(lib.saspa_cfg_ddim_step(_dt(x), _ptr(eps), _ptr(x), nimg, hw, c, 8, float(guidance), float(sa_t),
                                       float(s1m_t), float(sa_p), float(s1m_p), _stream()), "saspa_cfg_ddim_step")
    return x


def ddim_step(eps, x, nimg, hw, c, sa_t, s1m_t, sa_p, s1m_p):
    """eps, x: [nimg, hw, 8]; DDIM update without CFG (SDXL-Turbo, guidance off), x in place."""
    _check_dev(eps, x)
    lib = _L(x)
    _lib.check(lib.saspa_ddim_step(_dt(x), _ptr(eps), _ptr(x), nimg, hw, c, 8, float(sa_t), float(s1m_t), float(sa_p),
                                   float(s1m_p), _stream()), "saspa_ddim_step")
    return x


def gather_row(table, index, dst):
    """dst[:] = table[index[0]] for a [rows, ...] fp32 table and a device int32 index (hipGraph step state)."""
    _check_dev(table, index, dst)
    lib = _L()
    row = table[0].numel()
    if table.dtype != torch.float32 or dst.dtype != torch.float32 or index.dtype != torch.int32 or not table.is_contiguous() \
            or not dst.is_contiguous() or dst.numel() != row:
        raise ValueError("gather_row: fp32 contiguous table [rows, ...], dst of one row, int32 index")
    _lib.check(lib.saspa_gather_row_f32(_ptr(table), row, _ptr(index), _ptr(dst), row, _stream()), "saspa_gather_row_f32")
    return dst


def _check_table(what, name, table, rows, cols, index):
    """A step's device table: fp32 [rows, cols], dense, read at row index[0] of a device int32 index."""
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != cols or not table.is_contiguous() \
            or index is None or index.dtype != torch.int32:
        raise ValueError(f"{what}: {name} fp32 [{rows}, {cols}], int32 index")


def ddim_step_dev(eps, x, nimg, hw, c, guidance, coefs, index, cfg=True):
    """(CFG +) DDIM update with the coefficients of row index[0] of the device table coefs [steps, 4]."""
    _check_dev(eps, x, coefs, index)
    lib = _L(x)
    _check_table("ddim_step_dev", "coefs", coefs, "steps", 4, index)
    _lib.check(lib.saspa_ddim_step_dev(_dt(x), _ptr(eps), _ptr(x), nimg, hw, c, 8, int(bool(cfg)), float(guidance), _ptr(coefs),
                                       _ptr(index), _stream()), "saspa_ddim_step_dev")
    return x


def _cfg3_shapes(what, eps, x, nimg, hw):
    _same_dtype(what, x, eps=eps)
    if x.numel() != 3 * nimg * hw * 8 or eps.numel() != x.numel() or not x.is_contiguous() or not eps.is_contiguous():
        raise ValueError(f"{what}: eps, x contiguous [3 * nimg, hw, 8]")


def cfg3_ddim_step(eps, x, nimg, hw, c, guidance, image_guidance, sa_t, s1m_t, sa_p, s1m_p):
    """eps, x: [3*nimg, hw, 8] in the groups (uncond | image | text): three-branch guidance (InstructPix2Pix) + DDIM.  Channels < c of
    all three groups of x are updated in place; channels c..7 (the image latents) keep their bits."""
    _check_dev(eps, x)
    _cfg3_shapes("cfg3_ddim_step", eps, x, nimg, hw)
    lib = _L(x)
    _lib.check(lib.saspa_cfg3_ddim_step(_dt(x), _ptr(eps), _ptr(x), nimg, hw, c, 8, float(guidance), float(image_guidance), float(sa_t),
                                        float(s1m_t), float(sa_p), float(s1m_p), _stream()), "saspa_cfg3_ddim_step")
    return x


def cfg3_ddim_step_dev(eps, x, nimg, hw, c, guidance, image_guidance, coefs, index):
    """cfg3_ddim_step with the coefficients of row index[0] of the device table coefs [steps, 4]."""
    _check_dev(eps, x, coefs, index)
    _cfg3_shapes("cfg3_ddim_step_dev", eps, x, nimg, hw)
    lib = _L(x)
    _check_table("cfg3_ddim_step_dev", "coefs", coefs, "steps", 4, index)
    _lib.check(lib.saspa_cfg3_ddim_step_dev(_dt(x), _ptr(eps), _ptr(x), nimg, hw, c, 8, float(guidance), float(image_guidance),
                                            _ptr(coefs), _ptr(index), _stream()), "saspa_cfg3_ddim_step_dev")
    return x


def cfg_plms_step_dev(eps, x, hist, saved, nimg, hw, c, guidance, table, index):
    """PLMS update with the evaluation's parameters read from row index[0] of the device table [evaluations, 10]."""
    _check_dev(eps, x, hist, saved, table, index)
    _check_table("cfg_plms_step_dev", "table", table, "evaluations", 10, index)
    _lib.check(_L(x).saspa_cfg_plms_step_dev(_dt(x), _ptr(eps), _ptr(x), _ptr(hist), _ptr(saved), nimg, hw, c, 8, float(guidance),
                                                   _ptr(table), _ptr(index), _stream()), "saspa_cfg_plms_step_dev")
    return x


def cfg_unipc_step(eps, x, state, nimg, hw, c, guidance, row=None, table=None, index=None):
    """CFG + one UniPC step; state [3, nimg, hw, 8] (last | m0 | m1).  `row`: 12 host floats, or (`table` fp32 [steps, 12],
    `index` int32 [1]) on the device."""
    _check_dev(eps, x, state, table, index)
    if table is not None:
        _check_table("cfg_unipc_step", "table", table, "steps", 12, index)
    r = None if row is None else (C.c_float * 12)(*[float(v) for v in row])
    _lib.check(_L(x).saspa_cfg_unipc_step(_dt(x), _ptr(eps), _ptr(x), _ptr(state), nimg, hw, c, 8, float(guidance), r,
                                                _ptr(table), _ptr(index), _stream()), "saspa_cfg_unipc_step")
    return x


def unipc_step(eps, x, state, nimg, hw, c, row=None, table=None, index=None):
    """One UniPC step WITHOUT classifier-free guidance (sd_xl-turbo): eps / x [nimg, hw, 8]; state [3, nimg, hw, 8]."""
    _check_dev(eps, x, state, table, index)
    if table is not None:
        _check_table("unipc_step", "table", table, "steps", 12, index)
    r = None if row is None else (C.c_float * 12)(*[float(v) for v in row])
    _lib.check(_L(x).saspa_unipc_step(_dt(x), _ptr(eps), _ptr(x), _ptr(state), nimg, hw, c, 8, r, _ptr(table), _ptr(index),
                                            _stream()), "saspa_unipc_step")
    return x


def _vstep_shapes(what, v, x, nimg, hw, groups, state=None):
    """Operands of a v-prediction step: v, x contiguous [groups * nimg, hw, 8] of one element type (state: [3, nimg, hw, 8])."""
    _same_dtype(what, x, v=v, state=state)
    n = groups * nimg * hw * 8
    if nimg < 1 or hw < 1 or x.numel() != n or v.numel() != n or not x.is_contiguous() or not v.is_contiguous():
        raise ValueError(f"{what}: v, x contiguous [{groups} * nimg, hw, 8]")
    if state is not None and (state.numel() != 3 * nimg * hw * 8 or not state.is_contiguous()):
        raise ValueError(f"{what}: state contiguous [3, nimg, hw, 8]")


def cfg_ddim_step_v(v, x, nimg, hw, c, guidance, sa_t, s1m_t, sa_p, s1m_p):
    """cfg_ddim_step for a v-prediction network (saspa_cfg_ddim_step_v): v, x [2*nimg, hw, 8]; x in place, both CFG halves."""
    _check_dev(v, x)
    _vstep_shapes("cfg_ddim_step_v", v, x, nimg, hw, 2)
    _lib.check(_L(x).saspa_cfg_ddim_step_v(_dt(x), _ptr(v), _ptr(x), nimg, hw, c, 8, float(guidance), float(sa_t), float(s1m_t),
                                           float(sa_p), float(s1m_p), _stream()), "saspa_cfg_ddim_step_v")
    return x


def ddim_step_v(v, x, nimg, hw, c, sa_t, s1m_t, sa_p, s1m_p):
    """ddim_step for a v-prediction network (no CFG): v, x [nimg, hw, 8]; x in place."""
    _check_dev(v, x)
    _vstep_shapes("ddim_step_v", v, x, nimg, hw, 1)
    _lib.check(_L(x).saspa_ddim_step_v(_dt(x), _ptr(v), _ptr(x), nimg, hw, c, 8, float(sa_t), float(s1m_t), float(sa_p),
                                       float(s1m_p), _stream()), "saspa_ddim_step_v")
    return x


def ddim_step_v_dev(v, x, nimg, hw, c, guidance, coefs, index, cfg=True):
    """ddim_step_dev for a v-prediction network: the coefficients of row index[0] of the device table coefs [steps, 4]."""
    _check_dev(v, x, coefs, index)
    _vstep_shapes("ddim_step_v_dev", v, x, nimg, hw, 2 if cfg else 1)
    _check_table("ddim_step_v_dev", "coefs", coefs, "steps", 4, index)
    _lib.check(_L(x).saspa_ddim_step_v_dev(_dt(x), _ptr(v), _ptr(x), nimg, hw, c, 8, int(bool(cfg)), float(guidance), _ptr(coefs),
                                           _ptr(index), _stream()), "saspa_ddim_step_v_dev")
    return x


def cfg_unipc_step_v(v, x, state, nimg, hw, c, guidance, row=None, table=None, index=None):
    """cfg_unipc_step for a v-prediction network; the 12-float row carries alpha_t in slot 10 (UniPCMultistepScheduler.plan)."""
    _check_dev(v, x, state, table, index)
    _vstep_shapes("cfg_unipc_step_v", v, x, nimg, hw, 2, state)
    if table is not None:
        _check_table("cfg_unipc_step_v", "table", table, "steps", 12, index)
    r = None if row is None else (C.c_float * 12)(*[float(t) for t in row])
    _lib.check(_L(x).saspa_cfg_unipc_step_v(_dt(x), _ptr(v), _ptr(x), _ptr(state), nimg, hw, c, 8, float(guidance), r,
                                            _ptr(table), _ptr(index), _stream()), "saspa_cfg_unipc_step_v")
    return x


def unipc_step_v(v, x, state, nimg, hw, c, row=None, table=None, index=None):
    """unipc_step (no CFG) for a v-prediction network: v, x [nimg, hw, 8]; state [3, nimg, hw, 8]."""
    _check_dev(v, x, state, table, index)
    _vstep_shapes("unipc_step_v", v, x, nimg, hw, 1, state)
    if table is not None:
        _check_table("unipc_step_v", "table", table, "steps", 12, index)
    r = None if row is None else (C.c_float * 12)(*[float(t) for t in row])
    _lib.check(_L(x).saspa_unipc_step_v(_dt(x), _ptr(v), _ptr(x), _ptr(state), nimg, hw, c, 8, r, _ptr(table), _ptr(index),
                                        _stream()), "saspa_unipc_step_v")
    return x


def index_add(index, delta=1):
    _check_dev(index)
    _lib.check(_L().saspa_index_add(_ptr(index), int(delta), _stream()), "saspa_index_add")
    return index


def clock_probe(out2, iters=250):
    """out2: int64 device tensor [2] <- (shader clocks, 100 MHz ticks) of a window of iters x s_sleep 127 (~1 ms at 250),
    measured by one sleeping wave on the current stream (bench.py: a side stream, while the hot path runs)."""
    _check_dev(out2)
    if out2.dtype != torch.int64 or out2.numel() < 2 or not out2.is_contiguous():
        raise ValueError("clock_probe wants a contiguous int64 tensor of >= 2 elements")
    _lib.check(_L().saspa_clock_probe(_ptr(out2), int(iters), _stream()), "saspa_clock_probe")
    return out2


def vae_sample_noise(moments, e1, e2, scaling, sa, s1m):
    """moments [B,h,w,8] (mean | logvar), e1 / e2 [B,h,w,8] noise draws -> noised start latents [B,h,w,8] (img2img)."""
    _check_dev(moments, e1, e2)
    out = torch.empty_like(moments)
    npix = moments.numel() // 8
    _lib.check(_L(moments).saspa_vae_sample_noise(_dt(moments), _ptr(moments.contiguous()), _ptr(e1.contiguous()), _ptr(e2.contiguous()),
                                                  _ptr(out), npix, float(scaling), float(sa), float(s1m), _stream()),
               "saspa_vae_sample_noise")
    return out


def scale(x, s, out=None):
    _check_dev(x, out)
    lib = _L(x)
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.saspa_scale(_dt(x), _ptr(x), _ptr(out), x.numel(), float(s), _stream()), "saspa_scale")
    return out


def u8_to_act(img_u8, dtype):
    """u8 [n,H,W,3] -> [n,H,W,8] in [0,1]"""
    _check_dev(img_u8)
    n, h, w, _ = img_u8.shape
    out = torch.empty((n, h, w, 8), device=img_u8.device, dtype=dtype)
    lib = _L(out)
    _lib.check(lib.saspa_u8_to_act(_dt(out), _ptr(img_u8), _ptr(out), n * h * w, _stream()), "saspa_u8_to_act")
    return out


def act_to_u8(x):
    """[n,H,W,>=4] (3 live channels) -> u8 [n,H,W,3]"""
    _check_dev(x)
    lib = _L(x)
    n, h, w, _ = x.shape
    out = torch.empty((n, h, w, 3), device=x.device, dtype=torch.uint8)
    _lib.check(lib.saspa_act_to_u8(_dt(x), _ptr(x), _pitch4(x), _ptr(out), n * h * w, _stream()), "saspa_act_to_u8")
    return out


def canny(img_u8, low, high):
    """u8 [n,H,W,3] (device) -> u8 [n,H,W,3] in {0,255}"""
    _check_dev(img_u8)
    lib = _L()
    n, h, w, c = img_u8.shape
    if c != 3 or img_u8.dtype != torch.uint8 or not img_u8.is_contiguous():
        raise ValueError("canny expects a contiguous u8 [n,H,W,3] tensor")
    out = torch.empty_like(img_u8)
    work = torch.empty((8 * n * h * w,), device=img_u8.device, dtype=torch.uint8)
    _lib.check(lib.saspa_canny(_ptr(img_u8), _ptr(out), _ptr(work), n, h, w, int(low), int(high), _stream()),
               "saspa_canny")
    return out
