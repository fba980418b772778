"""Host launch trace of ``saspa_aug_amd.ops``: run ops functions on CPU tensors and record, in order, every library call that would
launch a kernel -- the parameter structs as ops filled them, with pointers replaced by labels -- without launching anything.  The
library's host-side queries (the `ops._HOST_ONLY` name rule: dispatch, eligibility, split-K suggestions) are answered by the real
library, which needs no device for them.  tests/test_ops_trace_host.py pins the traces of a fixed corpus of cases."""
import contextlib
import ctypes as C
import os

import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops

_DT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.uint8: "u8", torch.int32: "i32", torch.int64: "i64"}


class Names:
    """The tensors a case passes in, by attribute name: `n.x = ...` registers `x` for the pointer labels."""

    def __init__(self):
        object.__setattr__(self, "tensors", {})

    def __setattr__(self, name, t):
        self.tensors[name] = t
        object.__setattr__(self, name, t)


class _TorchShim:
    """`ops.torch` during a case: forwards to torch; `empty` / `zeros` (and `empty_like`) are forced onto the CPU, logged and kept
    alive (a freed temporary's address could be handed out again and mislabel a later pointer)."""

    def __init__(self, allocs):
        self._allocs = allocs

    def __getattr__(self, name):
        return getattr(torch, name)

    def _make(self, kind, shape, kw):
        kw["device"] = "cpu"
        t = getattr(torch, kind)(shape, **kw)
        self._allocs.append((kind, t))
        return t

    def empty(self, shape, **kw):
        return self._make("empty", shape, kw)

    def zeros(self, shape, **kw):
        return self._make("zeros", shape, kw)

    def empty_like(self, t, **kw):
        return self._make("empty", tuple(t.shape), dict(kw, dtype=kw.get("dtype", t.dtype)))


class _Proxy:
    """Stands in for a loaded library: host-only entry points go to the real one, every other `saspa_*` call is snapshot and
    answered with 0 (or the next scripted return code of that entry point)."""

    def __init__(self, real, trace, tag):
        self._real, self._trace, self._tag = real, trace, tag

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("saspa_") or any(t in name for t in ops._HOST_ONLY):
            return fn
        tr = self._trace

        def record(*args):
            tr.calls.append([self._tag + name] + [tr.snap(a) for a in args])
            scripted = tr.rc.get(name)
            return scripted.pop(0) if scripted else 0
        return record


class Trace:
    def __init__(self, names, rc):
        self.names, self.allocs, self.calls, self.recorded = names, [], [], []
        self.rc = {k: list(v) for k, v in (rc or {}).items()}

    @staticmethod
    def _holds(t, v):
        base = t.data_ptr()
        return base <= v < base + max(1, t.untyped_storage().nbytes() - t.storage_offset() * t.element_size())

    def label(self, v):
        """A pointer as `<argument name>+<byte offset>` or `<empty|zeros><shape><dtype>#<ordinal among the case's allocations of
        the same kind, shape and dtype>+<offset>`: independent of where the allocator put things and of the order in which
        differently shaped temporaries were made."""
        if not v:
            return None
        for name, t in self.names.tensors.items():
            if t is not None and self._holds(t, v):
                return f"{name}+{v - t.data_ptr()}"
        seen = {}
        for kind, t in self.allocs:
            key = f"{kind}{list(t.shape)}{_DT[t.dtype]}"
            seen[key] = seen.get(key, -1) + 1
            if self._holds(t, v):
                return f"{key}#{seen[key]}+{v - t.data_ptr()}"
        return "?"

    def snap(self, a):
        obj = getattr(a, "_obj", None)                     # byref(struct)
        if isinstance(obj, C.Structure):
            fields = {}
            for f, ty in obj._fields_:
                v = getattr(obj, f)
                if ty is C.c_void_p:
                    v = self.label(v)
                if v:
                    fields[f] = v
            return [type(obj).__name__, fields]
        if isinstance(a, C.c_void_p):
            return self.label(a.value)
        if isinstance(a, C.Array):
            return list(a)
        return a

    def tensor(self, t):
        if t is None or not torch.is_tensor(t):
            return t
        d = {"shape": list(t.shape), "strides": list(t.stride()), "dtype": _DT[t.dtype], "ptr": self.label(t.data_ptr())}
        g = getattr(t, "saspa_gn", None)
        if g is not None:
            d["saspa_gn"] = [int(g[1]), self.label(g[0].data_ptr())]
        return d

    def recorder(self):
        """A launch recorder with the `conditional` hook, as bench.py's: logs (kind, flops, meta) of what it is handed."""
        log = self.recorded

        class Rec:
            def __call__(self, kind, flops, call, meta=None):
                log.append([kind, flops, None if meta is None else list(meta)])
                return call()

            def conditional(self, kind, flops, call, meta, keep):
                rc = call()
                if keep(rc):
                    log.append([kind, flops, None if meta is None else list(meta)])
                return rc
        return Rec()


@contextlib.contextmanager
def _patched(tr, env):
    real, real_f16 = _lib.load, _lib.load_f16
    saved = (ops._check_dev, ops._stream, ops.torch, ops._RECORDER)
    saved_env = dict(os.environ)
    for k in [k for k in os.environ if k.startswith("SASPA_")]:
        del os.environ[k]                                   # the A/B knobs a case does not set are at their defaults
    os.environ.update(env or {})
    ops._check_dev = lambda *ts: None
    ops._stream = lambda: None
    ops.torch = _TorchShim(tr.allocs)
    _lib.load = lambda: _Proxy(real(), tr, "")
    _lib.load_f16 = lambda: _Proxy(real_f16(), tr, "f16:")
    try:
        yield
    finally:
        _lib.load, _lib.load_f16 = real, real_f16
        ops._check_dev, ops._stream, ops.torch, ops._RECORDER = saved
        os.environ.clear()
        os.environ.update(saved_env)


def run_case(fn, rc=None, env=None, recorder=False):
    """Run `fn(names)` (which registers its tensors on `names` and calls ops) and return the case's normalised record."""
    names = Names()
    tr = Trace(names, rc)
    rec = {}
    with _patched(tr, env):
        if recorder:
            ops.set_recorder(tr.recorder())
        try:
            out = fn(names)
            rec["ret"] = [tr.tensor(t) for t in out] if isinstance(out, (tuple, list)) else tr.tensor(out)
        except Exception as e:                              # noqa: BLE001   (the cases that are meant to raise)
            rec["exc"] = [type(e).__name__, str(e)]
    allocs = {}
    for kind, t in tr.allocs:
        key = f"{kind}{list(t.shape)}{_DT[t.dtype]}"
        allocs[key] = allocs.get(key, 0) + 1
    rec["allocs"] = dict(sorted(allocs.items()))
    rec["calls"] = tr.calls
    if recorder:
        rec["recorded"] = tr.recorded
    return rec
