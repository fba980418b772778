"""What `pipeline.py` asks of the layers below it, call for call, against a recorded trace (no GPU: tests/pipeline_trace.py runs the
batch entry points on CPU tensors with recording stand-ins for `ops`, the networks and the streams).  The eager loop and the
captured step of every pipeline family, scheduler and A/B knob are pinned: which rows the encoders take, where the twin hint is
on, which stream the ControlNet encoder runs on, which update closes the step and with what coefficients.
`python tests/test_pipeline_trace_host.py --write-golden` records tests/golden/pipeline_call_trace.json; `--write-golden CASE...`
re-records the named cases only."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import pipeline as P  # noqa: E402
from saspa_aug_amd.scheduler import DDIMScheduler, PNDMScheduler, UniPCMultistepScheduler  # noqa: E402
from pipeline_trace import place, run_case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_call_trace.json")
# The fixture was recorded from the pipeline as it was when a sampling step was still written three times (the captured step, the
# eager loop, SDXL's own eager loop), except the cases these rules name: they changed when the three became one, are recorded from
# that code, and carry the reason in the fixture.  Same calls with the same arguments in each; what moved is their order.


def note(name):
    if name.startswith("captured") and name.endswith("fork=0"):
        return ("recorded from the single network evaluation: the captured step with SASPA_FORK=0 ran UNet-encode, then "
                "ControlNet.forward; now ControlNet-encode, UNet-encode, zero_convs with the twin hint off, as the eager loop always did")
    if name.startswith("eager sdxl"):
        return ("recorded from the single eager loop: SDXL's own loop prepared context and time tables net by net; now both contexts, "
                "then both time tables, as the SD-1.5 loop always did (independent host-side preparation, same calls)")
    if name == "eager refused: img2img on UniPC":
        return "recorded from the single schedule: the eager loop refused after prepare_context; now before it, as the captured form did"
    return None
TINY, TINY_XL, TINY_IP2P = CFG.tiny(), CFG.tiny_xl(), CFG.tiny_ip2p()
B, HH, STEPS = 2, 64, 2
TOK = object()                      # (the batch entry points take token ids: no tokenizer is built)
CASES = []


def _ids(n=B, tokens=77):
    return np.arange(n * tokens, dtype=np.int64).reshape(n, tokens) % 500


def _u8(n=B, side=HH):
    return np.zeros((n, side, side, 3), np.uint8)


def _lat(log, name="latents", c=4, side=HH):
    return log.name(torch.zeros((B, c, side // 8, side // 8), dtype=torch.float16), name)


def case(name, **opts):
    def reg(fn):
        CASES.append((name, fn, opts))
        return fn
    return reg


def both_forms(name, fn, forks=(None,), **opts):
    """The eager loop and the captured step of one call; `forks`: the SASPA_FORK settings of the captured form."""
    CASES.append(("eager " + name, fn, opts))
    for f in forks:
        env = dict(opts.get("env", {}), **({} if f is None else {"SASPA_FORK": f}))
        CASES.append((f"captured {name}" + ("" if f is None else f" fork={f}"), fn, dict(opts, env=env, captured=True)))


def sd15(sched=None, **kw):
    def fn(log, pipes):
        pipe = place(P.StableDiffusionControlNetPipeline({}, TINY, TOK, sched and sched()), log)
        pipes.append(pipe)
        return pipe.generate_batch(_ids(), _ids(1), _u8(), _lat(log), STEPS, return_latents=True, **kw)
    return fn


def img2img(cls, sched=None, strength=0.5, steps=4, **kw):
    def fn(log, pipes):
        pipe = place(cls({}, TINY, TOK, sched and sched()), log)
        pipes.append(pipe)
        images = (_u8(),) if cls is P.StableDiffusionImg2ImgPipeline else (_u8(), _u8())
        return pipe.generate_batch_img2img(_ids(), _ids(1), *images, _lat(log, "sample_noise"), _lat(log, "noise"), steps, strength,
                                           return_latents=True, **kw)
    return fn


def ip2p(sched=None, **kw):
    def fn(log, pipes):
        pipe = place(P.StableDiffusionInstructPix2PixPipeline({}, TINY_IP2P, TOK, sched and sched()), log)
        pipes.append(pipe)
        return pipe.generate_batch_ip2p(_ids(), _ids(1), _u8(), _lat(log), STEPS, return_latents=True, **kw)
    return fn


def blip(**kw):
    def fn(log, pipes):
        pipe = place(P.BlipDiffusionControlNetPipeline({}, TINY, TOK, None, TOK), log)
        pipes.append(pipe)
        q = log.name(torch.zeros((B, 16, 64), dtype=torch.bfloat16), "query_embeds")
        return pipe.generate_batch(_ids(tokens=pipe.prompt_token_count()), _ids(1), _u8(), _lat(log), STEPS, 7.5, 1.0,
                                   return_latents=True, query_embeds=q, **kw)
    return fn


def sdxl(sched=None, guidance=0.0, neg=None, **kw):
    def fn(log, pipes):
        pipe = place(P.StableDiffusionXLControlNetPipeline({}, TINY_XL, TOK, sched and sched(), TOK), log, vae_dtype=torch.float32)
        pipes.append(pipe)
        return pipe.generate_batch(_ids(), neg, _u8(), _lat(log), STEPS, guidance, return_latents=True, **kw)
    return fn


# ---- SD-1.5 ControlNet: scheduler x CFG prefix x fork x recorder ----------------------------------------------------------------
for _s, _sched in (("ddim", None), ("unipc", UniPCMultistepScheduler)):
    for _p in ("1", "0"):
        for _f in ("1", "0"):
            _env = {"SASPA_CFG_PREFIX": _p, "SASPA_FORK": _f}
            _n = f"sd15 {_s} prefix={_p} fork={_f}"
            CASES.append(("eager " + _n, sd15(_sched), {"env": _env}))
            CASES.append(("eager " + _n + " plain recorder", sd15(_sched), {"env": _env, "recorder": "plain"}))
            CASES.append(("eager " + _n + " twin recorder", sd15(_sched), {"env": _env, "recorder": "twin"}))
            CASES.append(("captured " + _n, sd15(_sched), {"env": _env, "captured": True}))
# ---- the other families -----------------------------------------------------------------------------------------------------------
both_forms("controlnet img2img t_start=2", img2img(P.StableDiffusionControlNetImg2ImgPipeline), forks=("1", "0"))
both_forms("img2img without controlnet, pair prefix", img2img(P.StableDiffusionImg2ImgPipeline))
both_forms("img2img without controlnet, prefix=0", img2img(P.StableDiffusionImg2ImgPipeline), env={"SASPA_CFG_PREFIX": "0"})
both_forms("ip2p three branches", ip2p())
both_forms("blip plms", blip(), forks=("1", "0"))
both_forms("sdxl no cfg ddim", sdxl(), forks=("1", "0"))
both_forms("sdxl no cfg unipc", sdxl(UniPCMultistepScheduler), forks=("1", "0"))
both_forms("sdxl cfg negative None", sdxl(guidance=5.0), forks=("1", "0"))
both_forms("sdxl cfg negative given", sdxl(guidance=5.0, neg=_ids(1)), forks=("1", "0"))
both_forms("sdxl cfg unipc", sdxl(UniPCMultistepScheduler, guidance=5.0, neg=_ids(1)), forks=("1",))
# ---- refusals: each in the eager and in the captured form -----------------------------------------------------------------------
both_forms("refused: img2img on PNDM", img2img(P.StableDiffusionControlNetImg2ImgPipeline, PNDMScheduler))
both_forms("refused: img2img on UniPC", img2img(P.StableDiffusionControlNetImg2ImgPipeline, UniPCMultistepScheduler))
both_forms("refused: three branches on PNDM", ip2p(PNDMScheduler))
both_forms("refused: three branches on UniPC", ip2p(UniPCMultistepScheduler))
both_forms("img2img on UniPC, strength 1 (t_start 0) runs", img2img(P.StableDiffusionControlNetImg2ImgPipeline, UniPCMultistepScheduler, 1.0, 2))
REFUSED = {
    "refused: img2img on PNDM": ("NotImplementedError", "img2img runs on DDIM / UniPC (the reference switches non-BLIP pipelines away from PNDM)"),
    "refused: img2img on UniPC": ("NotImplementedError", "img2img with UniPC: the multistep history would have to start mid-schedule"),
    "refused: three branches on PNDM": ("NotImplementedError", "three guidance branches (InstructPix2Pix) run on DDIM only"),
    "refused: three branches on UniPC": ("NotImplementedError", "three guidance branches (InstructPix2Pix) run on DDIM only"),
}


# ---- refusals of the batch entry points (the shared prologue) ----------------------------------------------------------------------
def entry_refusal(name, call, exc):
    def fn(log, pipes):
        return call(log)
    CASES.append(("entry refused: " + name, fn, {}))
    REFUSED["entry refused: " + name] = exc


def _sd15_pipe(log):
    return place(P.StableDiffusionControlNetPipeline({}, TINY, TOK), log)


def _i2i_pipe(log, cls=P.StableDiffusionControlNetImg2ImgPipeline):
    return place(cls({}, TINY, TOK), log)


entry_refusal("sd15 guidance <= 1", lambda log: _sd15_pipe(log).generate_batch(_ids(), _ids(1), _u8(), _lat(log), STEPS, 1.0),
              ("NotImplementedError", "guidance_scale <= 1 (no CFG) belongs to the SDXL-Turbo branch (SURVEY a9)"))
entry_refusal("sd15 control image side", lambda log: _sd15_pipe(log).generate_batch(_ids(), _ids(1), _u8(side=96), _lat(log, side=96), STEPS),
              ("ValueError", "control image sides must be multiples of 64 (got 96x96)"))
entry_refusal("sd15 latents shape", lambda log: _sd15_pipe(log).generate_batch(_ids(), _ids(1), _u8(), _lat(log, side=128), STEPS),
              ("ValueError", "latents shape (2, 4, 16, 16) does not match the control image 64x64"))
entry_refusal("sd15 latents shape on device",
              lambda log: _sd15_pipe(log).generate_batch(_ids(), _ids(1), _u8(), _lat(log), STEPS, latents_on_device=True),
              ("ValueError", "latents shape (2, 4, 8, 8) does not match the control image 64x64"))
entry_refusal("blip negative token count",
              lambda log: place(P.BlipDiffusionControlNetPipeline({}, TINY, TOK, None, TOK), log).generate_batch(
                  _ids(tokens=61), _ids(1, 61), _u8(), _lat(log), STEPS, 7.5, 1.0, query_embeds=torch.zeros((B, 16, 64), dtype=torch.bfloat16)),
              ("ValueError", "negative context has 61 tokens, positive 77"))
entry_refusal("img2img image side",
              lambda log: _i2i_pipe(log).generate_batch_img2img(_ids(), _ids(1), _u8(side=96), _u8(side=96), _lat(log, side=96), _lat(log, side=96), 4, 0.5),
              ("ValueError", "image sides must be multiples of 64 (got 96x96)"))
entry_refusal("img2img source and control sizes",
              lambda log: _i2i_pipe(log).generate_batch_img2img(_ids(), _ids(1), _u8(), _u8(side=128), _lat(log), _lat(log), 4, 0.5),
              ("ValueError", "source and control images must have the same size"))
entry_refusal("img2img control image refused without controlnet",
              lambda log: P.StableDiffusionControlNetImg2ImgPipeline.generate_batch_img2img(
                  _i2i_pipe(log, P.StableDiffusionImg2ImgPipeline), _ids(), _ids(1), _u8(), _u8(), _lat(log), _lat(log), 4, 0.5),
              ("ValueError", "a control image is required by the ControlNet pipelines and refused by the ControlNet-free one"))
entry_refusal("ip2p image side",
              lambda log: place(P.StableDiffusionInstructPix2PixPipeline({}, TINY_IP2P, TOK), log).generate_batch_ip2p(
                  _ids(), _ids(1), _u8(side=96), _lat(log, side=96), STEPS),
              ("ValueError", "image sides must be multiples of 64 (got 96x96)"))
entry_refusal("ip2p latents shape",
              lambda log: place(P.StableDiffusionInstructPix2PixPipeline({}, TINY_IP2P, TOK), log).generate_batch_ip2p(
                  _ids(), _ids(1), _u8(), _lat(log, side=128), STEPS),
              ("ValueError", "latents shape (2, 4, 16, 16) does not match the source image 64x64"))
entry_refusal("sdxl control image side",
              lambda log: place(P.StableDiffusionXLControlNetPipeline({}, TINY_XL, TOK, None, TOK), log).generate_batch(
                  _ids(), None, _u8(side=80), _lat(log, side=80), STEPS),
              ("ValueError", "control image sides must be multiples of 32 (got 80x80)"))


def traces(only=None):
    """[(name, record)] of the corpus, normalised through JSON (tuples -> lists, as the fixture reads back)."""
    names = [n for n, _, _ in CASES]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return [(name, json.loads(json.dumps(run_case(fn, **opts)))) for name, fn, opts in CASES if only is None or name in only]


def read_golden():
    """The fixture stores every distinct call once (`lines`) and a case as indices into that table."""
    with open(GOLDEN) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    lines = rows[0]["lines"]
    return [dict(r, calls=[lines[i] for i in r["calls"]]) for r in rows[1:]]


def write_golden(rows):
    table, index = [], {}
    out = []
    for r in rows:
        calls = []
        for c in r["calls"]:
            k = json.dumps(c, separators=(",", ":"))
            if k not in index:
                index[k] = len(table)
                table.append(c)
            calls.append(index[k])
        out.append(dict(r, calls=calls))
    with open(GOLDEN, "w") as f:
        for r in [{"lines": table}] + out:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")


def _first_difference(got, want):
    for key in ("exc", "ret", "graph_keys"):
        if got.get(key) != want.get(key):
            return f"{key}:\n    got  {got.get(key)}\n    want {want.get(key)}"
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if g != w:
            return f"call {i}:\n    got  {g}\n    want {w}"
    return f"{len(got['calls'])} calls, want {len(want['calls'])}: " + \
        str((got["calls"] + [None])[len(want["calls"])] if len(got["calls"]) > len(want["calls"]) else want["calls"][len(got["calls"])])


def test_pipeline_call_trace():
    """Every call the pipelines make into ops, the networks and the streams for the corpus -- arguments, order, exceptions, returned
    tensors, graph cache keys -- is the recorded one."""
    assert os.path.getsize(GOLDEN) < 64 * 1024, "the fixture outgrew tests/golden/ops_launch_trace.json's 64 KB"
    want = read_golden()
    got = traces()
    assert [n for n, _ in got] == [w["case"] for w in want], "the corpus and the fixture list different cases"
    for w in want:
        assert w.get("note") == note(w["case"]), w["case"]
    bad = [(n, g, w) for (n, g), w in zip(got, want) if dict(g, case=n) != {k: v for k, v in w.items() if k != "note"}]
    msg = "\n".join(f"case {n!r}: {_first_difference(g, w)}" for n, g, w in bad[:8])
    assert not bad, f"{len(bad)} of {len(want)} call traces changed:\n{msg}"


def test_refusals_by_type_and_text():
    got = dict(traces(only={n for n, _, _ in CASES if "refused" in n}))
    for name, r in got.items():
        key = name.replace("eager ", "").replace("captured ", "")
        assert tuple(r.get("exc", ())) == REFUSED[key], (name, r.get("exc"))


def test_corpus_takes_its_branches():
    """The corpus is not vacuous: the arms named in the case titles show in the records."""
    got = dict(traces())
    names = lambda n: [c[0] for c in got[n]["calls"]]  # noqa: E731
    for name, r in got.items():
        assert ("exc" in r) == ("refused" in name), (name, r.get("exc"))
        assert ("graph_keys" in r) == (name.startswith("captured") and "refused" not in name), name
    n = "eager sd15 ddim prefix=1 fork=1"
    assert ["ops.twin_branch enter", True] in got[n]["calls"] and "wait_stream" not in names(n)
    assert ["ops.twin_branch enter", False] in got[n + " plain recorder"]["calls"]
    assert ["ops.twin_branch enter", False] in got["eager sd15 ddim prefix=1 fork=0"]["calls"]
    twin = names(n + " twin recorder")
    assert twin.count("rec.begin_twin") == twin.count("rec.end_twin") == STEPS and twin.count("record_stream") == 3 * STEPS
    assert twin.index("rec.begin_twin") < twin.index("stream enter") < twin.index("rec.end_twin")
    assert "rec.begin_twin" not in names("eager sd15 ddim prefix=1 fork=0 twin recorder")
    cap = names("captured sd15 ddim prefix=1 fork=1")
    assert cap.count("wait_stream") == 2 and "stream enter" in cap and cap[-2:] == ["ops.ddim_step_dev", "ops.index_add"]
    assert "wait_stream" not in names("captured sd15 ddim prefix=1 fork=0")
    assert names("eager img2img without controlnet, pair prefix").count("ops.dup_rows") == 2
    assert "ops.dup_rows" not in names("eager img2img without controlnet, prefix=0")
    assert names("eager ip2p three branches").count("ops.cfg3_ddim_step") == STEPS
    assert names("eager blip plms").count("ops.cfg_plms_step") == STEPS + 1
    assert names("eager sdxl no cfg ddim").count("ops.ddim_step") == STEPS
    assert names("eager sdxl no cfg unipc").count("ops.unipc_step") == STEPS
    assert names("eager sdxl cfg unipc").count("ops.cfg_unipc_step") == STEPS
    assert names("captured blip plms fork=1")[-2] == "ops.cfg_plms_step_dev"
    assert names("captured ip2p three branches")[-2] == "ops.cfg3_ddim_step_dev"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write-golden"]:
        only = set(sys.argv[2:])
        fresh = [dict({"case": name}, **r) for name, r in traces(only or None)]
        if only:
            assert only == {r["case"] for r in fresh}, only - {r["case"] for r in fresh}
            fresh = {r["case"]: r for r in fresh}
            fresh = [fresh.get(w["case"], w) for w in read_golden()]
        for r in fresh:
            r.pop("note", None)
            if note(r["case"]):
                r["note"] = note(r["case"])
        write_golden([{k: r[k] for k in ("case", "note", "exc", "ret", "graph_keys", "calls") if k in r} for r in fresh])
        print(f"{GOLDEN}: {len(fresh)} cases, {os.path.getsize(GOLDEN)} bytes")
    elif sys.argv[1:2] == ["--show"]:
        for name, r in traces(set(sys.argv[2:]) or None):
            print(name, r.get("exc") or r.get("graph_keys") or r.get("ret"))
            for c in r["calls"]:
                print("   ", json.dumps(c))
