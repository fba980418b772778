"""Host call trace of ``saspa_aug_amd.pipeline``: run the pipelines' batch entry points on CPU tensors and record, in order, what
they ask of the layers below -- every `ops.*` call, every network method, every stream operation -- without launching anything.
`pipeline.ops` is a recording stand-in, the networks are fakes that return CPU tensors of plausible shapes, the streams are fakes.
tests/test_pipeline_trace_host.py pins the traces of a fixed corpus of cases.

Tensors are logged by name: what a fake returned (`unet.mid`, `h2d#1`: the second tensor `ops.h2d` returned) or, for a tensor the
pipeline made itself, `[shape]dtype#ordinal` in order of first appearance; a view of a named buffer as `name+offset[shape]`."""
import contextlib
import inspect
import os

import numpy as np
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import imageproc
from saspa_aug_amd import ops as real_ops
from saspa_aug_amd import pipeline as P

_DT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.uint8: "u8", torch.int32: "i32", torch.int64: "i64",
       torch.float64: "f64", torch.float8_e4m3fn: "e4m3", torch.bool: "bool"}       # (the last three: tests/models_trace.py)
_LOG = [None]                       # the Log of the case that is running (what _T.record_stream writes to)


class _T(torch.Tensor):
    """What the fakes return: a CPU tensor whose `record_stream` is logged (the real one refuses a CPU tensor)."""

    def record_stream(self, stream):
        _LOG[0].add("record_stream", self, stream)


class Stream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_stream(self, other):
        self.log.add("wait_stream", self, other)


class Log:
    def __init__(self):
        self.lines, self.bufs, self.counts = [], [], {}
        self.main, self.side = Stream(self, "main"), Stream(self, "side")

    def name(self, t, name):
        """Register what a fake returns under `name` (`name#n` from the second of that name on); returns it as a _T."""
        if isinstance(t, (tuple, list)):
            return type(t)(self.name(e, name) for e in t)
        if not torch.is_tensor(t):
            return t
        n = self.counts.get(name, 0)
        self.counts[name] = n + 1
        t = t.as_subclass(_T)
        self.bufs.append((name if n == 0 else f"{name}#{n}", t))      # (kept alive: a freed buffer's address could come back)
        return t

    def tensor(self, t):
        base = t.untyped_storage().data_ptr()
        for name, b in self.bufs:
            if b.untyped_storage().data_ptr() == base:
                off = t.storage_offset() - b.storage_offset()
                whole = off == 0 and t.shape == b.shape and t.dtype == b.dtype
                return name if whole else f"{name}+{off}{list(t.shape)}" + ("" if t.dtype == b.dtype else _DT[t.dtype])
        whole = t if t._base is None else t._base         # (first seen as a slice: the buffer is what it was cut from)
        key = f"{list(whole.shape)}{_DT[whole.dtype]}"
        n = self.counts.get(key, 0)
        self.counts[key] = n + 1
        self.bufs.append((f"{key}#{n}", whole))
        return self.tensor(t)

    def value(self, v):
        if torch.is_tensor(v):
            return self.tensor(v)
        if isinstance(v, Stream):
            return v.name
        if isinstance(v, np.ndarray):
            return [self.value(e) for e in v.tolist()] if v.ndim == 1 and v.size <= 16 else f"np{list(v.shape)}{v.dtype}"
        if isinstance(v, (bool, type(None), str)):
            return v
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(f"{float(v):.6g}")               # (scheduler coefficients: not to the last bit of the host's libm)
        if isinstance(v, (list, tuple, torch.Size)):
            return [self.value(e) for e in v]
        if isinstance(v, dict):
            return {str(k): self.value(e) for k, e in v.items()}
        if isinstance(v, torch.dtype):
            return _DT[v]
        if isinstance(v, torch.device):
            return str(v)
        return type(v).__name__

    def add(self, what, *args):
        self.lines.append([what] + [self.value(a) for a in args])

    @contextlib.contextmanager
    def region(self, what, *args):
        self.add(what + " enter", *args)
        try:
            yield
        finally:
            self.add(what + " exit")


def _z(shape, dtype):
    return torch.zeros(tuple(shape), dtype=dtype)


_OPS_RESULTS = {
    "h2d": lambda t, device, dtype=None: torch.as_tensor(t).to(dtype or torch.as_tensor(t).dtype).clone(),
    "u8_to_act": lambda img, dtype: _z(tuple(img.shape[:3]) + (8,), dtype),
    "act_to_u8": lambda x: _z(tuple(x.shape[:3]) + (3,), torch.uint8),
    "scale": lambda x, s, out=None: torch.zeros_like(x),
    "dup_rows": lambda x: _z((2 * x.shape[0],) + tuple(x.shape[1:]), x.dtype),
    "vae_sample_noise": lambda moments, *a: torch.zeros_like(moments),
}


class FakeOps:
    """`pipeline.ops` during a case: every call is logged with its arguments bound to the real function's parameter names (a
    keyword passed positionally is the same call); the few results the pipeline goes on to use are CPU tensors of the real shape."""

    def __init__(self, log):
        self._log, self._RECORDER = log, None

    def set_recorder(self, rec):
        self._RECORDER = rec

    def side_stream(self, device):
        return self._log.side

    def twin_branch(self, on=True):
        return self._log.region("ops.twin_branch", bool(on))

    def f32_gemm_mode(self, mode):
        return self._log.region("ops.f32_gemm_mode", mode)

    def __getattr__(self, name):
        real = getattr(real_ops, name)                     # (AttributeError for what ops does not have)
        if not callable(real):
            return real

        def call(*a, **k):
            bound = inspect.signature(real).bind(*a, **k)
            bound.apply_defaults()
            self._log.add("ops." + name, dict(bound.arguments))
            make = _OPS_RESULTS.get(name)
            return None if make is None else self._log.name(make(*a, **k), name)
        return call


class FakeNet:
    """UNet / ControlNet: logs the methods the pipeline calls.  Under cfg_pair the encoders take B rows and hand back B rows at
    the first skip and 2B below it, as models._Net.encode does."""

    def __init__(self, log, name, dtype):
        self.log, self.name, self.dtype = log, name, dtype
        self.temb_all = self.ctx_kv = None

    def prepare_context(self, ctx):
        self.log.add(self.name + ".prepare_context", ctx)
        k, vt = self.log.name((_z((ctx.shape[0], 77, 16), self.dtype), _z((ctx.shape[0], 16, 80), self.dtype)), self.name + ".kv")
        self.ctx_kv = {"blk": (k, vt, int(ctx.shape[1]))}

    def prepare_timesteps(self, timesteps, added=None):
        self.log.add(self.name + ".prepare_timesteps", timesteps, added)
        shape = (len(timesteps), 24) if added is None else (len(timesteps), added[0].shape[0], 24)
        self.temb_all = self.log.name(_z(shape, torch.float32), self.name + ".temb_all")

    def bind_step_state(self, cur):
        self.log.add(self.name + ".bind_step_state", cur)

    def _levels(self, sample, cfg_pair):
        n, h, w, _ = sample.shape
        n2 = 2 * n if cfg_pair else n
        return _z((n2, h // 2, w // 2, 16), self.dtype), [_z((n, h, w, 16), self.dtype), _z((n2, h // 2, w // 2, 16), self.dtype)]

    def encode(self, sample, step, conv_in_residual=None, cfg_pair=False):
        self.log.add(self.name + ".encode", sample, step, conv_in_residual, cfg_pair)
        mid, skips = self._levels(sample, cfg_pair)
        return self.log.name(mid, self.name + ".mid"), self.log.name(skips, self.name + ".skip")

    def decode(self, mid, skips, step, out=None):
        self.log.add(self.name + ".decode", mid, skips, step, out)
        return out

    def cond_embedding(self, cond):
        self.log.add(self.name + ".cond_embedding", cond)
        return self.log.name(_z((cond.shape[0], cond.shape[1] // 8, cond.shape[2] // 8, 16), self.dtype), self.name + ".cemb")

    def _added(self, what, sample, cfg_pair):
        n = sample.shape[0] * (2 if cfg_pair else 1)
        mid, skips = self._levels(sample[:1].expand(n, -1, -1, -1), False)
        return self.log.name(skips, what + ".skip"), self.log.name(mid, what + ".mid")

    def zero_convs(self, mid, feats, scale, unet_skips=None, unet_mid=None, cfg_pair=False):
        self.log.add(self.name + ".zero_convs", mid, feats, scale, unet_skips, unet_mid, cfg_pair)
        return self._added("zc", feats[0], cfg_pair)

    def forward(self, sample, step, cond_emb, scale, unet_skips=None, unet_mid=None, cfg_pair=False):
        self.log.add(self.name + ".forward", sample, step, cond_emb, scale, unet_skips, unet_mid, cfg_pair)
        return self._added("fwd", sample, cfg_pair)


class FakeVAE:
    f32_gemm = "exact"

    def __init__(self, log, dtype):
        self.log, self.dtype = log, dtype

    def decode(self, z):
        self.log.add("vae.decode", z)
        return self.log.name(_z((z.shape[0], 8 * z.shape[1], 8 * z.shape[2], 8), z.dtype), "vae.img")

    def encode(self, x):
        self.log.add("vae_encoder.encode", x)
        return self.log.name(_z((x.shape[0], x.shape[1] // 8, x.shape[2] // 8, 8), x.dtype), "vae.moments")


class FakeText:
    def __init__(self, log, name, width, dtype):
        self.log, self.name, self.width, self.dtype = log, name, width, dtype

    def forward(self, ids, ctx=None, ctx_begin=2, penultimate=False):
        self.log.add(self.name + ".forward", ids, ctx, ctx_begin, penultimate)
        tokens = ids.shape[1] + (0 if ctx is None else ctx.shape[1])        # (BLIP: the subject tokens are spliced in)
        h = self.log.name(_z((ids.shape[0], tokens, self.width), self.dtype), self.name + ".h")
        return (h, self.log.name(_z((ids.shape[0], self.width), self.dtype), self.name + ".pooled")) if penultimate else h


class FakeSafety:
    def __init__(self, log):
        self.log = log

    def forward(self, images_u8):
        self.log.add("safety.forward", images_u8)
        return self.log.name((torch.zeros_like(images_u8), _z((images_u8.shape[0],), torch.int32)), "safety.out")


class TwinRecorder:
    """bench.Recorder(twin=True) as far as the pipeline sees it."""
    twin = True

    def __init__(self, log):
        self.log = log

    def __call__(self, kind, flops, call, meta=None):
        return call()

    def begin_twin(self):
        self.log.add("rec.begin_twin")

    def end_twin(self):
        self.log.add("rec.end_twin")


def place(pipe, log, dtype=torch.bfloat16, vae_dtype=None):
    """What `.to()` leaves behind, with fakes for the networks and the CPU for the device."""
    pipe.device, pipe.dtype, pipe.noise_dtype = torch.device("cpu"), dtype, torch.float16
    pipe._need_device = lambda: None
    pipe._vae_dtype = vae_dtype or dtype
    pipe.unet = FakeNet(log, "unet", dtype)
    pipe.controlnet = FakeNet(log, "cn", dtype) if pipe.HAS_CONTROLNET else None
    pipe.vae = FakeVAE(log, vae_dtype or dtype)
    pipe.vae_encoder = FakeVAE(log, vae_dtype or dtype)
    pipe.text_encoder = FakeText(log, "text", pipe.cfgs["text"]["width"], dtype)
    if "text2" in pipe.cfgs:
        pipe.text_encoder_2 = FakeText(log, "text2", pipe.cfgs["text2"]["width"], dtype)
    if "safety" in pipe.cfgs and not hasattr(pipe, "qformer"):
        pipe.safety_checker = FakeSafety(log)
    return pipe


class _StepDone(Exception):
    """Ends a captured case once the step body has run (there is no graph to replay)."""


def run_case(fn, env=None, recorder=None, captured=False):
    """Run `fn(log)` (which builds a pipeline with `place` and calls a batch entry point) under the stand-ins and return the
    case's record.  captured: the step graph's `run` is the step body once, and the case ends there with the graph's cache key."""
    log = Log()
    fake = FakeOps(log)
    if recorder == "plain":
        fake.set_recorder(lambda kind, flops, call, meta=None: call())
    elif recorder == "twin":
        fake.set_recorder(TwinRecorder(log))
    pipes = []

    def run_once(graph):
        graph._step()
        raise _StepDone

    saved = (P.ops, P.side_stream, P._StepGraph.run, imageproc.normalize_u8, torch.cuda.current_stream, torch.cuda.stream)
    saved_env = dict(os.environ)
    for k in [k for k in os.environ if k.startswith("SASPA_")]:
        del os.environ[k]
    os.environ.update(dict(env or {}, SASPA_GRAPH="1" if captured else "0"))
    P.ops, P.side_stream, P._StepGraph.run = fake, fake.side_stream, run_once
    imageproc.normalize_u8 = lambda x, dtype, mean, std: (log.add("imageproc.normalize_u8", x, dtype, mean, std),
                                                          log.name(_z(tuple(x.shape[:3]) + (8,), dtype), "px"))[1]
    torch.cuda.current_stream = lambda *a: log.main
    torch.cuda.stream = lambda s: log.region("stream", s)
    _LOG[0] = log
    rec = {}
    try:
        out = fn(log, pipes)
        rec["ret"] = log.value(out)
    except _StepDone:
        rec["graph_keys"] = [log.value(k) for p in pipes for k in p._graphs]
    except Exception as e:                              # noqa: BLE001   (the cases that are meant to raise)
        rec["exc"] = [type(e).__name__, str(e)]
    finally:
        P.ops, P.side_stream, P._StepGraph.run, imageproc.normalize_u8, torch.cuda.current_stream, torch.cuda.stream = saved
        os.environ.clear()
        os.environ.update(saved_env)
        _LOG[0] = None
    rec["calls"] = log.lines
    return rec
