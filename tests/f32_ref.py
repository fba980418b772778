"""TEST INFRASTRUCTURE ONLY -- operands, float64 references, fp32 emulations and mutants of the exact-fp32 kernels: saspa_gemm with
SASPA_F32 operands (linear, conv, batched; every epilogue form), saspa_pool2d's average form and saspa_signsqrt_l2norm, plus the
fp32 forms of the softmax / norm / elementwise kernels.  CPU only; the CPU proof (tests/test_errbudget.py) and the GPU tests
(tests/test_f32_errbudget_gpu.py) both import it.  Every tensor is float64 holding fp32-representable values (f32v) -- the operands
the kernel gets -- so the reference is exact arithmetic on the kernel's own inputs and the error in units of 2^-24 (UNIT_F32) of the
per-output term magnitude is O(1) for any right kernel, whatever order it sums in.

The arithmetic being emulated (csrc/):
- Mma<float> (saspa_gemm.hip:39-52) is v_mfma_f32_16x16x4_f32: one step adds FOUR products to an fp32 accumulator; K tiles of 32
  are walked in ascending order.  The hardware's rounding inside a step is not documented, so both ends are legitimate: every
  product rounded into the accumulator on its own (`chain1`: the most roundings) and the four summed exactly, rounded once
  (`chain4`: the fewest).  torch's own matmul, K reversed and K slices are further orders.
- the fp32 epilogue is the un-staged per-lane one (gemm_epilogue's generic path, saspa_gemm.hip:242-285): v = acc + bias, + rowvec,
  act_pre(v * alpha), + residual, act_post, all fp32, float4 stores with a scalar tail for the last n < N columns when N % 4 != 0;
  act_pre is SiLU (x / (1 + expf(-x)), common.h:167) or ReLU, act_post the ReLU of ADD_RELU (common.h:173-176).
- K slices: fp32 slabs summed in slab order by splitk_reduce_kernel<float> (:906-935), then the same epilogue arithmetic.
- pool2d_kernel (saspa_filter.hip:31-64): the window's taps added in (ty, tx) order into an fp32 accumulator, times fp32 1 / k^2,
  stored in the storage type.
- signsqrt_l2norm_kernel (saspa_filter.hip:66-90): per-lane fp32 sums of |x| + eps over the lane's elements tid + 256 i -- over the
  NON-ZERO elements only, as sign(0) = 0 adds nothing to the reference's norm --, a wave sum, the four waves in fp64; inv = scale /
  max(sqrt(total), 1e-12) in fp32; y = sign(x) sqrtf(|x| + eps) inv.
"""
import math

import torch
import torch.nn.functional as F

from tests.errbudget import UNIT_BF16, UNIT_F32, _floor, gemm_scale

BF = torch.bfloat16                    # (fixed: this module's families do not follow tests/fp16_budget.py's re-run)


def f32(x):
    return x.float()


def f32v(x):
    """float64 holding fp32-representable values."""
    return x.float().double()


def through_bf16(x):
    return x.float().to(BF).double()


def tf32(x):
    """fp32 with the low 13 mantissa bits cleared (what an MFMA fed tf32 operands would see)."""
    return (x.float().contiguous().view(torch.int32) & -8192).view(torch.float32).double()


def split_hi_lo(a):
    hi = a.float().to(BF).float()
    return hi, (a.float() - hi).to(BF).float()


# ------------------------------------------------------------------ family f32_gemm
# epilogue forms: out = act_post(act_pre(alpha (acc + bias + rowvec)) + residual)
FORMS = {
    "bias": dict(act="none", alpha=1.0, bias=True, rowvec=False, res=False),
    "relu_res": dict(act="relu", alpha=1.0, bias=True, rowvec=False, res=True),
    "add_relu_res": dict(act="add_relu", alpha=1.0, bias=True, rowvec=False, res=True),
    "silu_full": dict(act="silu", alpha=0.75, bias=True, rowvec=True, res=True),
    "plain": dict(act="none", alpha=1.0, bias=False, rowvec=False, res=False),
}


def f32_scalar(v):
    """A host double as the fp32 the launch struct carries (SaspaGemmParams.alpha is a float): the reference uses THAT value."""
    return torch.tensor(v, dtype=torch.float32).item()


def bap_form(hw):
    """feature_matrix = att^T feat / HW (filters.py:356): alpha = 1 / HW as an fp32, nothing else."""
    return dict(act="none", alpha=f32_scalar(1.0 / hw), bias=False, rowvec=False, res=False)


def gemm_operands(rand, m, k, n, seed, kind="plain"):
    """The operands of one GEMM, out = A W^T (+ ...), all fp32-representable:
    - "plain": A ~ N(0, 1), W ~ N(0, 1 / K);
    - "relu": A = relu(z + 0.3), post-ReLU activations (non-negative, 38 % exact zeros, mean 0.57) against weight rows with their
      mean removed, so that the large common part cancels and |ref| << s as in test_errbudget._gemm_cases;
    - "bap": the bilinear-attention-pooling product of WSDANCAL.forward (filters.py:352-356): both operands post-ReLU, the last 4 of
      the K columns zero (HW = K - 4 real columns padded to a multiple of 8).  Nothing cancels: s = |ref|.
    bias, rowvec [N] and residual [M, N] ~ N(0, 1); a form uses what it names."""
    if kind == "plain":
        x = rand(m, k, seed=seed)
        w = rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k))
    elif kind == "relu":
        x = torch.relu(rand(m, k, seed=seed) + 0.3)
        w = rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k))
        w = w - w.mean(1, keepdim=True)
    elif kind == "bap":
        x = torch.relu(rand(m, k, seed=seed) + 0.3)
        w = torch.relu(rand(n, k, seed=seed + 1))
        x[:, k - 4:] = 0.0
        w[:, k - 4:] = 0.0
    else:
        raise ValueError(kind)
    return dict(x=f32v(x), w=f32v(w), b=f32v(rand(n, seed=seed + 2)), rv=f32v(rand(n, seed=seed + 3)),
                res=f32v(rand(m, n, seed=seed + 4)))


def _act_pre(act, z):
    return F.silu(z) if act == "silu" else (torch.relu(z) if act == "relu" else z)


def epilogue_ref(acc, op, form):
    """The documented epilogue in the dtype of acc (float64: the reference)."""
    f = FORMS[form] if isinstance(form, str) else form
    z = acc
    if f["bias"]:
        z = z + op["b"].to(acc.dtype)
    if f["rowvec"]:
        z = z + op["rv"].to(acc.dtype)
    z = _act_pre(f["act"], z * f["alpha"])
    if f["res"]:
        z = z + op["res"].to(acc.dtype)
    return torch.relu(z) if f["act"] == "add_relu" else z


def gemm_ref(op, form):
    """(float64 reference, magnitude s) of one GEMM in the given epilogue form."""
    f = FORMS[form] if isinstance(form, str) else form
    ref = epilogue_ref(op["x"] @ op["w"].t(), op, f)
    s = gemm_scale(op["x"], op["w"], op["b"] if f["bias"] else None, alpha=f["alpha"], residual=op["res"] if f["res"] else None,
                   rowvec=op["rv"] if f["rowvec"] else None)
    return ref, s


def acc_f32(x, w, order="matmul", ks=1):
    """A W^T accumulated in fp32: "matmul" torch's own order; "rev" K descending; "chain1" ONE accumulator, every product added
    with one rounding (an fma chain); "chain4" one accumulator, four products summed exactly per step and rounded once (the least an
    MFMA 16x16x4 step can round); ks > 1: K in ks contiguous slices, each summed by torch, the slabs added in slab order."""
    k = x.shape[1]
    if order == "rev":
        return f32(x.flip(1)) @ f32(w.flip(1)).t()
    if order in ("chain1", "chain4"):
        step = 1 if order == "chain1" else 4
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
        for k0 in range(0, k, step):
            # (fp32 x fp32 products are exact in float64; the sum is rounded to fp32 once)
            acc = (acc.double() + x[:, k0:k0 + step] @ w[:, k0:k0 + step].t()).float()
        return acc
    bounds = [round(i * k / ks) for i in range(ks + 1)]
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for a, b in zip(bounds[:-1], bounds[1:]):
        acc = acc + f32(x[:, a:b]) @ f32(w[:, a:b]).t()
    return acc


def gemm_emul(op, form, order="matmul", ks=1, *, x3=False, operands_tf32=False, bias_bf16=False, res_bf16=False, out_bf16=False,
              kdrop=0, bias_cols=None, alpha_first=False, tail_row=False, act=None, tail_bias0=False):
    """The kernel's arithmetic in fp32 (order / ks: the summation order); every further option is ONE slip (the mutants)."""
    f = dict(FORMS[form] if isinstance(form, str) else form)
    x, w = op["x"], op["w"]
    if kdrop:
        x, w = x[:, :-kdrop], w[:, :-kdrop]
    if operands_tf32:
        x, w = tf32(x), tf32(w)
    if x3:
        (xh, xl), (wh, wl) = split_hi_lo(x), split_hi_lo(w)
        acc = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    else:
        acc = acc_f32(x, w, order, ks)
    o = dict(op)
    if bias_bf16:
        o["b"] = through_bf16(op["b"])
    if res_bf16:
        o["res"] = through_bf16(op["res"])
    if bias_cols is not None:
        o["b"] = op["b"].clone()
        o["b"][bias_cols:] = 0.0
    if tail_bias0:                                     # the scalar tail indexes the bias by r instead of n + r
        o["b"] = op["b"].clone()
        o["b"][1:] = op["b"][0]
    if act is not None:
        f["act"] = act
    if alpha_first:
        z = acc * f["alpha"] + f32(o["b"]) + (f32(o["rv"]) if f["rowvec"] else 0.0)
        z = _act_pre(f["act"], z) + (f32(o["res"]) if f["res"] else 0.0)
        got = torch.relu(z) if f["act"] == "add_relu" else z
    else:
        got = epilogue_ref(acc, o, f)
    if tail_row:
        got = got.clone()
        got[-1] = got[-2]
    return through_bf16(got) if out_bf16 else got.double()


def conv_operands(rand, b, h, w, cin, cout, kh, stride, pad, seed, kind="plain", creal=None):
    """A convolution as its implicit GEMM: channels-last input [B, H, W, cin] (channels >= creal zero: a padded stem), weights [cout,
    cin, kh, kh]; "x" / "w" are the [M, taps * cin] / [N, taps * cin] operands in the kernel's K order (tap-major), rows in (b, oy,
    ox) order, so gemm_ref / gemm_emul serve it as they serve a linear.  kind as gemm_operands."""
    creal = cin if creal is None else creal
    x = rand(b, h, w, cin, seed=seed)
    wt = rand(cout, cin, kh, kh, seed=seed + 1, scale=1 / math.sqrt(creal * kh * kh))
    if kind == "relu":
        x = torch.relu(x + 0.3)
        wt = wt - wt[:, :creal].mean((1, 2, 3), keepdim=True)
    x[..., creal:] = 0.0
    wt[:, creal:] = 0.0
    x, wt = f32v(x), f32v(wt)
    u = F.unfold(x.permute(0, 3, 1, 2), kh, padding=pad, stride=stride)                    # [B, cin * taps, L]
    a = u.reshape(b, cin, kh * kh, -1).permute(0, 3, 2, 1).reshape(-1, kh * kh * cin)
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
    return dict(x=a, w=wt.permute(0, 2, 3, 1).reshape(cout, -1), b=f32v(rand(cout, seed=seed + 2)), rv=f32v(rand(cout, seed=seed + 3)),
                res=f32v(rand(a.shape[0], cout, seed=seed + 4)), x_nhwc=x, w_nchw=wt, out_hw=(ho, wo))


# (tag, M, K, N, operand kind, epilogue form, seed): the CPU proof's cases.  The GPU file launches its own shapes (one per kernel
# instantiation) with the same generators; the arithmetic per output depends on K, the operands and the form, not on M and N.
GEMM_CASES = [("300x64x96", 300, 64, 96, "plain", "silu_full", 1), ("129x40x40", 129, 40, 40, "relu", "bias", 5),
              ("260x320x4", 260, 320, 4, "plain", "relu_res", 9), ("260x320x3", 260, 320, 3, "relu", "add_relu_res", 13),
              ("192x576x96", 192, 576, 96, "relu", "silu_full", 17), ("192x2048x96", 192, 2048, 96, "plain", "add_relu_res", 21),
              ("64x4608x128", 64, 4608, 128, "relu", "relu_res", 25), ("300x64x96", 300, 64, 96, "plain", "bias", 27)]
# non-negative against non-negative operands (family f32_gemm_pos): every partial sum is as large as the result, so ONE fp32
# accumulator walking K errs by ~0.13 sqrt(K) units -- a budget of its own, see LIMITS
GEMM_POS_CASES = [("bap 32x200x64", 32, 200, 64, "bap", 196, 29), ("bap 32x56x64", 32, 56, 64, "bap", 52, 33)]
X3_KMAX = 576                          # beyond it the x3 arithmetic sinks into the accumulation error (see LIMITS["f32_gemm"])


def gemm_cases(rand, cases=None):
    """(name, got, ref64, s, legit?) rows of the f32_gemm family (cases = GEMM_POS_CASES: of f32_gemm_pos)."""
    out = []
    for tag, m, k, n, kind, form, seed in (GEMM_CASES if cases is None else cases):
        op = gemm_operands(rand, m, k, n, seed, kind)
        if kind == "bap":
            form, fname = bap_form(form), f"alpha = 1 / {form}"
        else:
            fname = form
        ref, s = gemm_ref(op, form)
        f = FORMS[form] if isinstance(form, str) else form
        tag = f"f32 {tag} {kind} {fname}"
        for order in ("matmul", "rev", "chain1", "chain4"):
            out.append((f"legit fp32 {order} {tag}", gemm_emul(op, form, order), ref, s, True))
        for ks in (2, 5, 8):
            if k >= 32 * ks:
                out.append((f"legit K in {ks} slices {tag}", gemm_emul(op, form, ks=ks), ref, s, True))
        if k <= X3_KMAX:
            out.append((f"mutant bf16x3 split operands {tag}", gemm_emul(op, form, x3=True), ref, s, False))
        out.append((f"mutant operands truncated to tf32 {tag}", gemm_emul(op, form, operands_tf32=True), ref, s, False))
        out.append((f"mutant output through bf16 {tag}", gemm_emul(op, form, out_bf16=True), ref, s, False))
        if f["bias"]:
            out.append((f"mutant bias rounded to bf16 {tag}", gemm_emul(op, form, bias_bf16=True), ref, s, False))
        if f["res"]:
            out.append((f"mutant residual rounded to bf16 {tag}", gemm_emul(op, form, res_bf16=True), ref, s, False))
        if kind != "bap":                              # (its last 4 K columns are the zero padding)
            out.append((f"mutant last 4 of K dropped {tag}", gemm_emul(op, form, kdrop=4), ref, s, False))
        out.append((f"mutant last 32 of K dropped {tag}", gemm_emul(op, form, kdrop=32), ref, s, False))
        if f["bias"] and n % 4 == 0 and n >= 8:
            out.append((f"mutant bias missing on the last 4 columns {tag}", gemm_emul(op, form, bias_cols=n - 4), ref, s, False))
        if f["bias"] and f["alpha"] != 1.0:
            out.append((f"mutant alpha applied before the bias {tag}", gemm_emul(op, form, alpha_first=True), ref, s, False))
        out.append((f"mutant ragged tail row copies its neighbour {tag}", gemm_emul(op, form, tail_row=True), ref, s, False))
        if f["act"] == "add_relu":
            out.append((f"mutant ReLU before the residual where ADD_RELU was asked {tag}", gemm_emul(op, form, act="relu"), ref, s,
                        False))
        if f["act"] == "relu":
            out.append((f"mutant ReLU after the residual where RELU was asked {tag}", gemm_emul(op, form, act="add_relu"), ref, s,
                        False))
        if n == 3:
            out.append((f"mutant scalar-tail columns take column 0's bias {tag}", gemm_emul(op, form, tail_bias0=True), ref, s,
                        False))
    return out


# ------------------------------------------------------------------ family f32_pool (average pooling, fp32 and bf16 storage)
def pool_input(rand, b, h, w, c, seed, kind, storage):
    """Channels-last [B, H, W, C] values of the storage type: "randn" N(0, 1), "relu" post-ReLU (non-negative, half zeros)."""
    x = rand(b, h, w, c, seed=seed)
    x = torch.relu(x) if kind == "relu" else x
    return x.to(storage).double()


def pool_windows(x, k, stride):
    """[B, H, W, C] -> [B, Ho, Wo, C, k * k], a window's taps in the kernel's (ty, tx) order (no padding: the average form)."""
    u = x.permute(0, 3, 1, 2).unfold(2, k, stride).unfold(3, k, stride)
    return u.permute(0, 2, 3, 1, 4, 5).reshape(*u.shape[:1], u.shape[2], u.shape[3], u.shape[1], k * k)


def avgpool_ref(x, k, stride):
    """(float64 window mean, s = window mean of |x|)."""
    win = pool_windows(x, k, stride)
    return win.mean(-1), _floor(win.abs().mean(-1))


def avgpool_emul(x, k, stride, storage, *, order="taps", denom=None, drop_last_row=False, acc_bf16=False):
    win = pool_windows(x, k, stride).float()
    taps = k * k - (k if drop_last_row else 0)
    inv = torch.tensor(1.0 / (denom or k * k), dtype=torch.float32)
    if order == "torch":
        got = F.avg_pool2d(x.float().permute(0, 3, 1, 2), k, stride).permute(0, 2, 3, 1)
    else:
        acc = torch.zeros(win.shape[:-1], dtype=torch.float32)
        for t in range(taps):
            acc = acc + win[..., t]
            if acc_bf16:
                acc = acc.to(BF).float()
        got = acc / float(denom or k * k) if order == "divide" else acc * inv
    return got.to(storage).double()


# (B, H, W, C, k, stride, input kind, seed); every case in both storage types
POOL_CASES = [(3, 23, 19, 8, 2, 2, "randn", 51), (3, 23, 19, 8, 7, 7, "randn", 53), (2, 14, 14, 24, 2, 2, "relu", 55),
              (2, 14, 14, 24, 7, 7, "relu", 57), (2, 14, 14, 24, 14, 14, "relu", 59), (3, 23, 19, 8, 19, 19, "randn", 61)]


def pool_unit(storage):
    """The unit of an average-pooling case is that of its storage type (families f32_pool / f32_pool_bf16)."""
    return UNIT_F32 if storage == torch.float32 else UNIT_BF16


def pool_cases(rand, storage=torch.float32):
    """Not every mutant is separable on every case, and the list says which: with bf16 storage the output rounding (2^-9 |out|)
    hides a slip that is small against it --
    - 1 / (k*k - 1) is 2^-8 / (k*k - 1) |out| / s units: on zero-mean inputs with 49 taps or more |out| << s and a few hundred
      outputs cannot show it; it is named for the non-negative inputs (|out| = s) and the 2x2 windows;
    - a bf16 accumulator adds ~0.1 sqrt(taps) units to an output rounding of ~0.4: it is named for the 196-tap whole-image window
      of the non-negative input, the only case where it doubles the rms."""
    out = []
    for b, h, w, c, k, stride, kind, seed in POOL_CASES:
        x = pool_input(rand, b, h, w, c, seed, kind, storage)
        ref, s = avgpool_ref(x, k, stride)
        tag = f"avgpool {b}x{h}x{w}x{c} k={k} {kind} {'fp32' if storage == torch.float32 else 'bf16'} storage"
        for order in ("taps", "torch", "divide"):
            out.append((f"legit fp32 sum, order {order} {tag}", avgpool_emul(x, k, stride, storage, order=order), ref, s, True))
        if storage == torch.float32 or kind == "relu" or k == 2:
            out.append((f"mutant 1 / (k*k - 1) {tag}", avgpool_emul(x, k, stride, storage, denom=k * k - 1), ref, s, False))
        out.append((f"mutant last tap row left out {tag}", avgpool_emul(x, k, stride, storage, drop_last_row=True), ref, s, False))
        if storage == BF and kind == "relu" and k == 14:
            out.append((f"mutant accumulation in bf16 {tag}", avgpool_emul(x, k, stride, storage, acc_bf16=True), ref, s, False))
    return out


# ------------------------------------------------------------------ family f32_tail (signsqrt_l2norm)
TAIL_EPS, TAIL_SCALE = 1e-6, 100.0


def tail_rows(rand, rows, c, kind, seed):
    """fp32 feature rows as the bilinear attention pooling leaves them (ReLU features under ReLU attention maps, ~0.05): "dense" no
    zeros (|z| * 0.05), "block" the same with C / 32 of the row zero in one block (a dead attention map), "heavy" relu(z - 0.25) *
    0.05: 60 % exact zeros, and its last row ALL zero; "signed": N(0, 1) of both signs with 7 zeros at the head of row 0 (the rows
    of test_filters_gpu.test_signsqrt_l2norm)."""
    z = rand(rows, c, seed=seed)
    if kind == "signed":
        x = z.clone()
        x[0, :7] = 0.0
    elif kind == "heavy":
        x = torch.relu(z - 0.25) * 0.05
        x[-1] = 0.0
    else:
        x = z.abs().clamp_min(1e-4) * 0.05
        if kind == "block":
            x[:, c // 3: c // 3 + c // 32] = 0.0
    return f32v(x)


def tail_ref(x, eps=TAIL_EPS, scale=TAIL_SCALE):
    """(float64 of the reference's formula: sign(x) sqrt(|x| + eps), F.normalize (1e-12 floor), * scale; s = |ref| floored)."""
    y = torch.sign(x) * torch.sqrt(x.abs() + eps)
    ref = scale * y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return ref, _floor(ref.abs())


def tail_emul(x, eps=TAIL_EPS, scale=TAIL_SCALE, *, order="kernel", count_zero_eps=False, norm_first=False):
    """fp32: "kernel" the kernel's sums (per lane tid + 256 i in fp32, 64 lanes per wave in fp32, the waves in fp64), "torch" the
    reference's own expression evaluated in fp32, "wave" ONE wave's 64 lanes with an fp32 combine (the coarsest order a kernel of
    this design could take; ONE fp32 accumulator over the whole row -- what the fp64 combine exists to avoid -- errs by 5 .. 13 rms
    units at 4096 positive elements and is deliberately NOT in the budget).  count_zero_eps: eps joins the squared
    norm for exact zeros too (sum (|x| + eps) over every element); norm_first: the row normalised before the sign-sqrt."""
    xf = f32(x)
    if norm_first:
        xf = F.normalize(xf, dim=-1)
    e = torch.tensor(eps, dtype=torch.float32)
    t = xf.abs() + e
    y = torch.sign(xf) * torch.sqrt(t)
    if order == "torch" and not count_zero_eps:
        return (F.normalize(y, dim=-1) * scale).double()
    tt = t if count_zero_eps else torch.where(xf != 0, t, torch.zeros(()))
    r, c = tt.shape
    if order == "wave":
        lanes = F.pad(tt, (0, -c % 64)).reshape(r, -1, 64)
        acc = torch.zeros(r, 64)
        for i in range(lanes.shape[1]):
            acc = acc + lanes[:, i]
        tot = acc.sum(-1).double()
    else:
        lanes = F.pad(tt, (0, -c % 256)).reshape(r, -1, 256)
        acc = torch.zeros(r, 256)
        for i in range(lanes.shape[1]):
            acc = acc + lanes[:, i]
        tot = acc.reshape(r, 4, 64).sum(-1).double().sum(-1)
    inv = torch.tensor(scale, dtype=torch.float32) / torch.sqrt(tot).float().clamp_min(1e-12)
    return (y * inv[:, None]).double()


TAIL_CASES = [(4, 4096, "dense", 71), (4, 4096, "block", 73), (5, 4096, "heavy", 75), (4, 1000, "dense", 77), (4, 1000, "block", 79),
              (5, 1000, "heavy", 81), (5, 4096, "signed", 83)]


def tail_cases(rand):
    out = []
    for rows, c, kind, seed in TAIL_CASES:
        x = tail_rows(rand, rows, c, kind, seed)
        ref, s = tail_ref(x)
        tag = f"signsqrt_l2norm {rows}x{c} {kind}"
        for order in ("kernel", "torch", "wave"):
            out.append((f"legit fp32 {order} sums {tag}", tail_emul(x, order=order), ref, s, True))
        if kind in ("block", "heavy"):                 # (without zeros the two formulas are the same; 7 zeros in 4096: 0.01 units)
            out.append((f"mutant eps counted for exact zeros {tag}", tail_emul(x, count_zero_eps=True), ref, s, False))
        out.append((f"mutant eps = 1e-12 {tag}", tail_emul(x, eps=1e-12), ref, s, False))
        out.append((f"mutant norm taken before the sign-sqrt {tag}", tail_emul(x, norm_first=True), ref, s, False))
    return out


# ------------------------------------------------------------------ second tier: the fp32 forms of kernels with bf16 budgets
# Operand generators and case lists are those of tests/test_errbudget.py (the values stay bf16-representable, stored as fp32: the
# GroupNorm reference restates the kernels' fp32 partial sums, which is exact only while v * v is); what changes is that nothing
# is rounded to bf16 on the way out, so the error is measured in units of 2^-24.
def _T():
    from tests import test_errbudget as T
    return T


def ident(x):
    """The fp32 store: the `rnd` of the bf16 emulations with the rounding removed."""
    return x.float().double()


def _tree(a):
    """Sum over the last dim (a power of two) as an xor-butterfly adds it."""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def ln_emul_lanes(x, g, b, eps, *, onepass=False):
    """layernorm_kernel<float> (saspa_norm.hip:372-435): LPR lanes per row, lane `sub` owns the 8-channel chunks sub + LPR i and
    adds their values in order, the lanes by butterfly; mean = sum / C; the squared deviations the same way; rstd = 1 / sqrtf(var +
    eps); y = (x - mean) rstd gamma + beta, all fp32.  onepass (NOT the kernel; a mutant on mean-offset rows): var = E[x^2] -
    mean^2 from fp32 sums."""
    xf = f32(x)
    rows, c = xf.shape
    lpr = 16 if c <= 384 else (32 if c <= 768 else 64)
    nch = -(-(c // 8) // lpr)
    v = F.pad(xf, (0, nch * lpr * 8 - c)).reshape(rows, nch, lpr, 8)
    live = F.pad(torch.ones(c), (0, nch * lpr * 8 - c)).reshape(nch, lpr, 8)

    def lanes(t):
        acc = torch.zeros(rows, lpr)
        for i in range(nch):
            for j in range(8):
                acc = acc + t[:, i, :, j]
        return _tree(acc)
    mean = (lanes(v) / c)[:, None]
    if onepass:
        var = (lanes(v * v) / c)[:, None] - mean * mean
    else:
        d = (v - mean[:, None, None]) * live
        var = (lanes(d * d) / c)[:, None]
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return ((xf - mean) * rstd * f32(g) + f32(b)).double()


def norm_cases(rand):
    """Family f32_norm: layernorm and groupnorm (statistics + apply) on fp32 storage."""
    from tests.errbudget import norm_scale
    T = _T()
    out = []
    for (rows, c, kind, eps, seed) in [(1024, 320, "normal", 1e-5, 1), (77, 768, "lowvar", 1e-5, 5), (77, 768, "lowvar", 1e-6, 7),
                                        (300, 320, "offset", 1e-5, 9)]:
        x = T._norm_inputs(kind, (rows, c), seed)
        g, b = f32v(1 + 0.1 * rand(c, seed=seed + 1)), f32v(0.1 * rand(c, seed=seed + 2))
        ref, xhat = T._ln_ref(x, g, b, eps)
        s = norm_scale(xhat, g, b, T.mu_rstd(x, eps), cancel=1.0)
        tag = f"f32 layernorm {rows}x{c} {kind} eps={eps:g}"
        out.append((f"legit two-pass, torch's sums {tag}", T._ln_emul(x, g, b, eps, rnd=ident), ref, s, True))
        out.append((f"legit two-pass, the kernel's lanes {tag}", ln_emul_lanes(x, g, b, eps), ref, s, True))
        out.append((f"mutant output through bf16 {tag}", through_bf16(ln_emul_lanes(x, g, b, eps)), ref, s, False))
        out.append((f"mutant gamma rounded to bf16 {tag}", ln_emul_lanes(x, through_bf16(g), b, eps), ref, s, False))
        if kind == "normal":
            out.append((f"mutant eps 1e-3 {tag}", T._ln_emul(x, g, b, eps, eps_used=1e-3, rnd=ident), ref, s, False))
            out.append((f"mutant n-1 variance {tag}", T._ln_emul(x, g, b, eps, unbiased=True, rnd=ident), ref, s, False))
        if kind == "lowvar":
            out.append((f"mutant eps swapped {tag}", T._ln_emul(x, g, b, eps, eps_used=1e-6 if eps == 1e-5 else 1e-5, rnd=ident), ref, s,
                        False))
            out.append((f"mutant eps x 10 {tag}", T._ln_emul(x, g, b, eps, eps_used=eps * 10, rnd=ident), ref, s, False))
        if kind == "offset":
            out.append((f"mutant one-pass fp32 statistics {tag}", ln_emul_lanes(x, g, b, eps, onepass=True), ref, s, False))
    for (bsz, hw, c, groups, kind, eps, seed) in [(8, 256, 320, 32, "normal", 1e-5, 11), (2, 64, 1280, 32, "lowvar", 1e-5, 13),
                                                  (2, 64, 1280, 32, "lowvar", 1e-6, 15), (2, 256, 320, 32, "offset", 1e-5, 587),
                                                  (2, 64, 1280, 32, "offset", 1e-5, 1355)]:
        x = T._norm_inputs(kind, (bsz, hw, c), seed)
        g, b = f32v(1 + 0.1 * rand(c, seed=12 + c)), f32v(0.1 * rand(c, seed=13 + c))
        cpg = c // groups
        for op in [False] + ([True] if cpg % 8 == 0 and hw * cpg <= 8192 else []):
            ref, xhat, mr = T.gn_kernel_ref(x, g, b, groups, eps, onepass=op)
            s = norm_scale(xhat, g, b, mr, cancel=1.0)
            mean, rstd = T.gn_kernel_stats(x, groups, eps, onepass=op)
            tag = f"f32 groupnorm {bsz}x{hw}x{c}/{groups} {kind} eps={eps:g} {'one-pass' if op else 'two-pass'}"
            apply = lambda r, rnd=ident: T.gn_kernel_apply(x, g, b, mean, r, groups, rnd=rnd)  # noqa: E731
            out.append((f"legit kernel statistics, fp32 scale / shift {tag}", apply(rstd), ref, s, True))
            out.append((f"legit kernel statistics, fp32 (x - mean) rstd gamma + beta {tag}",
                        ((f32(x) - mean.float().repeat_interleave(cpg, 1)[:, None]) * rstd.float().repeat_interleave(cpg, 1)[:, None]
                         * f32(g) + f32(b)).double(), ref, s, True))
            out.append((f"mutant output through bf16 {tag}", apply(rstd, through_bf16), ref, s, False))
            if kind == "normal":
                n = hw * cpg
                out.append((f"mutant n-1 variance {tag}", apply((rstd ** -2 * n / (n - 1)) ** -0.5), ref, s, False))
            if kind == "lowvar":
                for e2, nm in [(1e-6 if eps == 1e-5 else 1e-5, "eps swapped"), (eps * 10, "eps x 10")]:
                    out.append((f"mutant {nm} {tag}", apply((rstd ** -2 - eps + e2) ** -0.5), ref, s, False))
    return out


def softmax_ref(x, scale, causal):
    """(float64 softmax(x * scale) over the last dim of [..., n, n], s).  scale: the fp32 the launch carries.  A logit l = x * scale
    and its distance to the row's level are rounded to fp32 before the exponential, which turns 2^-24 (|l| + |l - m|) into a
    relative error of p: s = p (1 + |l| + |l - m|)."""
    l = x * scale
    if causal:
        l = l + torch.full(l.shape[-2:], float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax(l, -1)
    lv = torch.where(torch.isfinite(l), l, torch.zeros((), dtype=torch.float64))
    return p, _floor(p * (1 + lv.abs() + (lv - l.amax(-1, keepdim=True)).abs()))


def softmax_emul(x, scale, causal, *, order="kernel", shift=0, scale_mul=1.0):
    """softmax_rows_kernel<float> (saspa_attn.hip:1549-1573): l = x * scale, the level by max, expf(l - m) summed per lane over the
    columns lane + 64 i and by butterfly, times 1 / sum; "torch": torch's own fp32 softmax."""
    n = x.shape[-1]
    l = f32(x) * torch.tensor(scale * scale_mul, dtype=torch.float32)
    if causal:
        l = l + torch.full((n, n), float("-inf")).triu_(1 + shift)
    if order == "torch":
        return torch.softmax(l, -1).double()
    e = torch.exp(l - l.amax(-1, keepdim=True))
    lanes = F.pad(e, (0, -n % 64)).reshape(*e.shape[:-1], -1, 64)
    acc = torch.zeros(*e.shape[:-1], 64)
    for i in range(lanes.shape[-2]):
        acc = acc + lanes[..., i, :]
    return (e * (1.0 / _tree(acc))[..., None]).double()


SOFTMAX_SCALE = 0.3


def softmax_cases(rand):
    out = []
    sc = f32_scalar(SOFTMAX_SCALE)
    for causal in (False, True):
        x = f32v(rand(6, 77, 77, seed=27, scale=3.0))
        ref, s = softmax_ref(x, sc, causal)
        tag = f"f32 softmax_rows 6x77x77 {'causal' if causal else 'plain'}"
        for order in ("kernel", "torch"):
            out.append((f"legit fp32 {order} order {tag}", softmax_emul(x, sc, causal, order=order), ref, s, True))
        out.append((f"mutant output through bf16 {tag}", through_bf16(softmax_emul(x, sc, causal)), ref, s, False))
        out.append((f"mutant logits through bf16 {tag}", softmax_emul(through_bf16(x), sc, causal), ref, s, False))
        out.append((f"mutant scale x (1 + 2^-12) {tag}", softmax_emul(x, sc, causal, scale_mul=1 + 2.0 ** -12), ref, s, False))
        if causal:
            out.append((f"mutant causal mask shifted by one {tag}", softmax_emul(x, sc, causal, shift=1), ref, s, False))
    return out


QUICK = 1.702


def elem_refs(x):
    """{name: (float64 reference, s)} of geglu (x = [a | gate]), SiLU and quick-GELU.  0.5 g (1 + erf) is a difference of two
    terms of size 0.5 |g| and 0.5 |g erf| that cancel in the negative tail: both are in the magnitude.  quick-GELU rounds z = 1.702 x
    before the exponential: 2^-24 |z| there is a relative error of |z| (1 - sigmoid(z)) 2^-24 of the result, which joins its s."""
    f = x.shape[-1] // 2
    a, g = x[:, :f], x[:, f:]
    erf = torch.erf(g / math.sqrt(2.0))
    q = f32_scalar(QUICK)
    return {"geglu": (a * 0.5 * g * (1 + erf), _floor(a.abs() * 0.5 * g.abs() * (1 + erf.abs()))),
            "silu": (F.silu(x), _floor(F.silu(x).abs())),
            "quick-gelu": (x * torch.sigmoid(q * x),
                           _floor((x * torch.sigmoid(q * x)).abs() * (1 + (q * x).abs() * (1 - torch.sigmoid(q * x)))))}


def elem_cases(rand):
    out = []
    x = f32v(rand(123, 2 * 96, seed=38) * 2)
    xf = f32(x)
    a, g = xf[:, :96], xf[:, 96:]
    refs = elem_refs(x)
    q = torch.tensor(QUICK, dtype=torch.float32)
    kern = "the kernel's expression"
    emul = {"geglu": [("torch gelu", a * F.gelu(g)), (kern, a * (0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))))],
            "silu": [("torch silu", F.silu(xf)), (kern, xf / (1.0 + torch.exp(-xf)))],
            "quick-gelu": [("x sigmoid(1.702 x)", xf * torch.sigmoid(q * xf)), (kern, xf / (1.0 + torch.exp(-q * xf)))]}
    other = {"geglu": ("tanh-gelu", a * F.gelu(g, approximate="tanh")), "silu": ("swapped for quick-gelu", emul["quick-gelu"][1][1]),
             "quick-gelu": ("swapped for silu", emul["silu"][1][1])}
    for name, (ref, s) in refs.items():
        for how, got in emul[name]:
            out.append((f"legit f32 {name}, {how}", got.double(), ref, s, True))
        out.append((f"mutant f32 {name} output through bf16", through_bf16(emul[name][1][1]), ref, s, False))
        out.append((f"mutant f32 {name} {other[name][0]}", other[name][1].double(), ref, s, False))
    return out
