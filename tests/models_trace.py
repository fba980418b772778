"""Host call trace of ``saspa_aug_amd.models`` / ``blip`` (and the one method of ``filters`` that runs `attention_core`): build the
networks on the CPU from `weights.synth_state_dict`, run their methods on CPU tensors and record, in order, every `ops.*` call they
make -- arguments bound to the real function's parameter names, tensors by name -- without launching anything.
tests/test_models_trace_host.py pins the traces of a fixed corpus of cases.

Results: the stand-in logs the call and then runs the REAL ops wrapper under tests/ops_trace.py's patched library (every launch is
answered with 0), so the wrappers' own allocation code decides the result shapes.  Three exceptions: `h2d` (pinned memory needs a
device: a CPU copy), and the two predicates that are gated on `x.is_cuda`, `linear_ln_fusable` and `ff_block_eligible`, which answer
what the case scripts.  `torch.cuda.is_current_stream_capturing` answers what the case scripts as well.

Tensor names (pipeline_trace.Log): the entries of `net.p` under their keys (registered in sorted key order, so a view of a shared
buffer is `first key+offset[shape]`), the case's inputs under the names the case gives them, everything else `[shape]dtype#n` in
order of first appearance."""
import contextlib
import copy
import hashlib
import inspect
import json
import os

import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import blip, filters, models
from saspa_aug_amd import ops as real_ops
from saspa_aug_amd import weights as W
import ops_trace
from pipeline_trace import _DT, Log

CPU = torch.device("cpu")
PREDICATES = ("linear_ln_fusable", "ff_block_eligible")
ROUTING = ("blocks", "tr_info", "fp8_blocks", "fp8_qkv", "fp8_ffout", "fp8_ff_mx", "xattn_blocks", "ff_blocks", "fused_geglu",
           "qscaled", "temb_off", "n_skips")
CLASSES = {"unet": models.UNet, "controlnet": models.ControlNet, "vae": models.VAEDecoder, "vae_encoder": models.VAEEncoder,
           "text": models.CLIPText, "text2": models.CLIPText, "safety": models.SafetyChecker, "qformer": blip.Blip2QFormer,
           "clip_rn50": filters.ClipRN50Visual}
PACK_ENV = ("SASPA_FF_BLOCK", "SASPA_FP8_BREADTH", "SASPA_ATTN_VROW", "SASPA_UPCONV_PHASE", "SASPA_X3_PRESPLIT")  # read while packing


class _Launches:
    """What ops_trace's library proxy writes to: nothing is kept of a launch but the tensors ops allocated (alive, so that no
    address comes back under another name)."""

    def __init__(self):
        self.allocs, self.calls, self.rc = [], _Sink(), {}

    def snap(self, a):
        return None


class _Sink:
    def append(self, x):
        pass


class FakeOps:
    """`models.ops` / `blip.ops` / `filters.ops` during a case."""

    def __init__(self, log, pred):
        self._log, self._pred = log, pred

    @contextlib.contextmanager
    def f32_gemm_mode(self, mode):
        with self._log.region("ops.f32_gemm_mode", mode), real_ops.f32_gemm_mode(mode):
            yield

    def __getattr__(self, name):
        real = getattr(real_ops, name)                     # (AttributeError for what ops does not have)
        if not callable(real):
            return real
        sig = inspect.signature(real)

        def call(*a, **k):
            bound = sig.bind(*a, **k)
            # an argument left at (or passed as) its default is not stored: the same call, and a third of the fixture's size
            args = {n: v for n, v in bound.arguments.items()
                    if sig.parameters[n].default is inspect.Parameter.empty or not _same(v, sig.parameters[n].default)}
            self._log.add("ops." + name, args)
            if name in PREDICATES:
                return self._pred
            if name == "h2d":
                t = torch.as_tensor(a[0])
                return t.to(bound.arguments.get("dtype") or t.dtype).clone()
            return real(*a, **k)
        return call


def _same(v, default):
    return v is default or (isinstance(v, (bool, int, float, str)) and type(v) is type(default) and v == default) or \
        (isinstance(v, (int, float)) and isinstance(default, (int, float)) and not isinstance(v, bool) and v == default)


# ---- networks --------------------------------------------------------------------------------------------------------------------
_SD, _NETS, MANIFESTS, HOST_SUM_ERRORS = {}, {}, {}, {}


def host_sums(sd, p):
    """{key: (float64 recomputation from the state dict, bound)} of the entries of `p` that packing forms by a host matmul or
    normalisation: a v bias folded through the out projection, the safety checker's unit rows, CLIP RN50's position table through a
    projection.  Their last bits follow the host's BLAS and thread count, so the manifest pins shape and dtype and
    test_host_sums_by_value pins the values: bound = (K + 2) 2^-24 sum |terms|, what fp32 accumulation of K terms in ANY order
    can be off by (and one rounding of the result)."""
    def fold(bias, w, v):
        bias, w, v = sd[bias].double(), sd[w].double(), v.double()
        return bias + w @ v, (w.shape[1] + 2) * 2.0 ** -24 * (bias.abs() + w.abs() @ v.abs())
    out = {}
    for k in p:
        a = k[:-len(".o.b")]
        if k.endswith(".o.b"):
            for o, v in ((".out_proj", ".v_proj.bias"), (".to_out.0", ".to_v.bias"), (".output.dense", ".attention.value.bias")):
                if a + v in sd:
                    out[k] = fold(a + o + ".bias", a + o + ".weight", sd[a + v])
            if a + ".qkv.bias" in sd:
                out[k] = fold(a + ".projection.bias", a + ".projection.weight", sd[a + ".qkv.bias"][-sd[a + ".projection.weight"].shape[1]:])
        elif k == "embeds_n":
            e = torch.cat([sd["special_care_embeds"], sd["concept_embeds"]], 0).double()
            out[k] = torch.nn.functional.normalize(e), (e.shape[1] + 4) * 2.0 ** -24 * torch.nn.functional.normalize(e).abs()
        elif k.endswith(".r") and "visual.attnpool.positional_embedding" in sd:
            n = "visual.attnpool." + k[:-2] + "_proj"
            pos = sd["visual.attnpool.positional_embedding"].double()
            ref = pos @ sd[n + ".weight"].double().t() + sd[n + ".bias"].double()
            out[k] = ref, 2.0 ** -23 * (pos.abs() @ sd[n + ".weight"].double().abs().t() + sd[n + ".bias"].double().abs())
    return out


def _sha(obj, n):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:n]


def describe_params(p, by_value=()):
    """{key: what the manifest pins of it} for every entry of a network's `p`, in sorted key order; by_value: host_sums' keys."""
    shared = {}
    for k in sorted(p):
        if torch.is_tensor(p[k]):
            shared.setdefault(p[k].untyped_storage().data_ptr(), []).append(k)
    out = {}
    for k in sorted(p):
        t = p[k]
        if not torch.is_tensor(t):
            out[k] = repr(t)
            continue
        d = {"shape": list(t.shape), "dtype": _DT[t.dtype]}
        if k in by_value:
            d["host_sum"] = True
        else:
            d["sha256"] = hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
        for a in ("saspa_korder", "saspa_cin", "saspa_wsplit"):
            if hasattr(t, a):
                d[a] = int(getattr(t, a))
        peers = shared[t.untyped_storage().data_ptr()]
        if len(peers) > 1:
            d["shares_storage"] = [t.storage_offset(), list(t.stride())] + [q for q in peers if q != k]
        out[k] = d
    return out


def routing(net):
    out = {}
    for a in ROUTING:
        if hasattr(net, a):
            v = getattr(net, a)
            out[a] = sorted(v) if isinstance(v, set) else ({k: v[k] for k in sorted(v)} if isinstance(v, dict) else v)
    return json.loads(json.dumps(out))


def manifest(net, by_value=()):
    """The fixture's record of a freshly built network: the key count and a digest of the key list, one hex digit of a digest per key
    of `p` (sorted key order: which key changed) under a digest of them all, and four hex digits of a digest per routing attribute
    in ROUTING's order (`----`: the network has none)."""
    d, r = describe_params(net.p, by_value), routing(net)
    return {"keys": [len(d), _sha(sorted(d), 8)], "params": "".join(_sha([k, v], 1) for k, v in d.items()), "sha256": _sha(d, 16),
            "routing": "".join(_sha(r[a], 4) if a in r else "----" for a in ROUTING)}


def state_dict(kind, cfg):
    key = (kind, repr(cfg))
    if key not in _SD:
        _SD[key] = W.synth_state_dict({"vae_encoder": "vae_enc"}.get(kind, kind), cfg, seed=0)
    return _SD[key]


def _clone(net):
    """A network the case may change (time tables, contexts, calibration state) next to the cached one: the same tensors."""
    n2 = copy.copy(net)
    for a, v in vars(net).items():
        if isinstance(v, (dict, set, list)):
            setattr(n2, a, copy.copy(v))
    if hasattr(net, "pk"):
        n2.pk = copy.copy(net.pk)
        n2.pk.p = n2.p
    return n2


def build(log, name, kind, cfg, dtype, sd_edit=None, **kw):
    """Build (or take from the cache: packing is the slow part) a network under the case's environment and register its `p` with the
    log.  `name` is the manifest's name; sd_edit(sd) -> the state dict to build from instead.  Mutable fp8 state: never cached."""
    env = tuple((k, os.environ[k]) for k in PACK_ENV if k in os.environ)
    key = (name, kind, repr(cfg), dtype, repr(sorted(kw.items())), env)
    if key not in _NETS:
        sd = state_dict(kind, cfg)
        if sd_edit is not None:
            sd = sd_edit(dict(sd))
        mark = len(log.lines)
        try:
            with torch.no_grad():
                net = CLASSES[kind](sd, cfg, CPU, dtype, **kw)
        finally:
            del log.lines[mark:]                # (what packing asks of ops -- knobs, eligibility -- shows in the manifest)
        sums = host_sums(sd, net.p)
        MANIFESTS.setdefault(name, manifest(net, sums))
        HOST_SUM_ERRORS.setdefault(name, {k: float(((net.p[k].double() - ref).abs() / tol.clamp_min(1e-300)).max()) for k, (ref, tol) in sums.items()})
        if kw.get("fp8"):
            return _register(log, net)
        _NETS[key] = net
    return _register(log, _clone(_NETS[key]))


def _register(log, net):
    for holder in (net, getattr(net, "c", None)):           # (ClipRN50Visual keeps its convs in `c.p`)
        if holder is not None:
            for k in sorted(holder.p):
                if torch.is_tensor(holder.p[k]):
                    log.name(holder.p[k], k)
    return net


# ---- one case ----------------------------------------------------------------------------------------------------------------------
def run_case(fn, env=None, pred=False, capturing=False):
    """Run `fn(log)` (which builds networks with `build` and calls their methods) under the stand-ins; returns the case's record."""
    log = Log()
    fake = FakeOps(log, pred)
    saved = (models.ops, blip.ops, filters.ops, torch.cuda.is_current_stream_capturing)
    rec = {}
    with ops_trace._patched(_Launches(), env), torch.no_grad():
        models.ops = blip.ops = filters.ops = fake
        torch.cuda.is_current_stream_capturing = lambda: capturing
        try:
            rec["ret"] = log.value(fn(log))
        except Exception as e:                              # noqa: BLE001   (the cases that are meant to raise)
            rec["exc"] = [type(e).__name__, str(e)]
        finally:
            models.ops, blip.ops, filters.ops, torch.cuda.is_current_stream_capturing = saved
    rec["calls"] = log.lines
    return rec


def chain(calls):
    """Whole-network cases in the fixture: one hex digit per call of a running SHA-256 over the calls so far (a changed call changes
    every later digit as well: the first digit that differs is at the changed call, or seldom just behind it), and the final digest."""
    h, out = hashlib.sha256(), []
    for c in calls:
        h.update(json.dumps(c, separators=(",", ":")).encode())
        out.append(h.hexdigest()[0])
    return {"n": len(calls), "digits": "".join(out), "sha256": h.hexdigest()[:16]}
