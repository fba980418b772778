"""The T5 key-to-text generator on the device (saspa_aug_amd/txt2sentence.py, csrc/saspa_t5.hip) against tests/t5_ref.py: the three
kernels within the budgets that tests/test_t5_host.py proves on the CPU (limits from the emulations, never from a kernel's output), the
sampler's decisions against float64 wherever float64 decides them, the tiny model against the reference, greedy and sampled ids in
fp32, batching invariance, the full-width model once, and the entry point."""
import json
import os
import runpy

import numpy as np
import pytest
import torch

import errbudget as E
import saspa_aug_amd  # noqa: F401
import t5_ref as R
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.txt2sentence import T5Generator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]


# ---- saspa_rmsnorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_within_budget(dev, dtype):
    worst = 0.0
    for shape in R.RMS_SHAPES:
        x, gamma = R.rms_operands(*shape, dtype, 0)
        ref, s = R.rmsnorm_ref64(x, gamma, R.RMS_EPS)
        got = ops.rmsnorm(x.to(dev), gamma.to(dev), R.RMS_EPS).cpu()
        st = E.check_budget(got, ref, s, R.UNITS[dtype], limits=R.RMS_LIMITS[dtype], what=f"rmsnorm {shape}")
        worst = max(worst, E.ratio(st, R.RMS_LIMITS[dtype]))
        # rows of a wider buffer (a pitch beyond C) and an `out` view: bit-identical
        wide = torch.zeros((shape[0], shape[1] + 16), dtype=dtype, device=dev)
        wide[:, :shape[1]] = x.to(dev)
        out = torch.full((shape[0], shape[1] + 8), 7.0, dtype=dtype, device=dev)
        ops.rmsnorm(wide[:, :shape[1]], gamma.to(dev), R.RMS_EPS, out=out[:, :shape[1]])
        assert torch.equal(out[:, :shape[1]].cpu(), got) and bool((out[:, shape[1]:] == 7.0).all())
    print(f"rmsnorm {dtype}: worst statistic at {worst:.3f} of its allowance")
    x, gamma = R.rms_operands(5, 768, dtype, 0)                      # negative control: a mutant's output fed to the same assertion
    ref, s = R.rmsnorm_ref64(x, gamma, R.RMS_EPS)
    for m in R.RMS_MUTANTS:
        with pytest.raises(AssertionError):
            E.check_budget(R.rmsnorm_emul(x, gamma, R.RMS_EPS, mutant=m), ref, s, R.UNITS[dtype], limits=R.RMS_LIMITS[dtype])


def test_rmsnorm_row_alone_is_bit_identical_and_refusals_launch_nothing(dev):
    for dtype in DTYPES:
        x, gamma = R.rms_operands(33, 1024, dtype, 1)
        full = ops.rmsnorm(x.to(dev), gamma.to(dev), R.RMS_EPS).cpu()
        for r in (0, 6, 32):
            assert torch.equal(ops.rmsnorm(x[r:r + 1].to(dev), gamma.to(dev), R.RMS_EPS).cpu()[0], full[r])
    lib = _lib.load()
    x = torch.ones((4, 64), device=dev)
    g = torch.ones((8200,), device=dev)
    out = torch.full((4, 8200), 7.0, device=dev)

    def call(c=64, ldx=64, ldo=8200, xoff=0, eps=1e-6, dtype=_lib.SASPA_F32):
        rc = lib.saspa_rmsnorm(dtype, x.data_ptr() + xoff, ldx, out.data_ptr(), ldo, 4, c, g.data_ptr(), eps, None)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote the output"
        return rc
    assert call(c=60) == _lib.SASPA_EALIGN                           # C % 8
    assert call(c=8200, ldx=8200) == _lib.SASPA_ERANGE               # C > 8192
    assert call(ldx=32) == _lib.SASPA_EINVAL                         # a pitch shorter than C
    assert call(xoff=4) == _lib.SASPA_EALIGN
    assert call(ldx=66) == _lib.SASPA_EALIGN
    assert call(eps=-1.0) == _lib.SASPA_EINVAL
    assert call(dtype=_lib.SASPA_F16) == _lib.SASPA_EINVAL
    got = ops.rmsnorm(x, g[:64].contiguous(), 0.0)                   # an accepted call writes
    assert bool((got == 1.0).all())


# ---- saspa_attn_relbias ----------------------------------------------------------------------------------------------------------
def _rel_dev(dev, q, k, v, ln, pos, bias, center, heads, rpe, scale):
    return ops.attn_relbias(q.to(dev), k.to(dev), v.to(dev), heads, k.shape[1], scale, pos.to(dev), bias.to(dev), center,
                            rows_per_entry=rpe, lens=None if ln is None else ln.to(dev)).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_relbias_within_budget(dev, dtype):
    worst = 0.0
    for case in R.rel_cases():
        heads, d, nk, rpe, _ = case
        q, k, v, ln, pos, bias, center = R.rel_operands(case, dtype, 0)
        scale = d ** -0.5
        ref, s = R.relbias_ref64(q, k, v, ln, pos, bias, center, heads, rpe, scale)
        got = _rel_dev(dev, q, k, v, ln, pos, bias, center, heads, rpe, scale)
        st = E.check_budget(got, ref, s, R.UNITS[dtype], limits=R.REL_LIMITS[dtype], what=f"attn_relbias {case}")
        worst = max(worst, E.ratio(st, R.REL_LIMITS[dtype]))
        assert bool((got[1] == 0).all())                             # len 0: a zero row
        # dead keys poisoned with NaN change nothing (they are never read): bit-identical
        kp, vp = k.clone(), v.clone()
        for e in range(R.ENTRIES):
            dead_from = int(ln[e * rpe:(e + 1) * rpe].max())
            kp[e, dead_from:], vp[e, dead_from:] = float("nan"), float("nan")
        assert torch.equal(_rel_dev(dev, q, kp, vp, ln, pos, bias, center, heads, rpe, scale), got), case
    print(f"attn_relbias {dtype}: worst statistic at {worst:.3f} of its allowance")
    case = (12, 64, 130, 20, 1)                                      # negative control
    q, k, v, ln, pos, bias, center = R.rel_operands(case, dtype, 0)
    ref, s = R.relbias_ref64(q, k, v, ln, pos, bias, center, 12, 20, 0.125)
    for m in R.REL_MUTANTS:
        with pytest.raises(AssertionError):
            E.check_budget(R.relbias_emul(q, k, v, ln, pos, bias, center, 12, 20, 0.125, mutant=m), ref, s, R.UNITS[dtype],
                           limits=R.REL_LIMITS[dtype])


def test_attn_relbias_row_alone_is_bit_identical(dev):
    for dtype in DTYPES:
        for case in ((12, 64, 130, 20, 1), (4, 16, 65, 3, 0), (4, 16, 7, 1, 2)):
            heads, d, nk, rpe, _ = case
            q, k, v, ln, pos, bias, center = R.rel_operands(case, dtype, 2)
            full = _rel_dev(dev, q, k, v, ln, pos, bias, center, heads, rpe, 0.25)
            for r in (0, 5, q.shape[0] - 2):
                e = r // rpe
                alone = _rel_dev(dev, q[r:r + 1], k[e:e + 1], v[e:e + 1], ln[r:r + 1], pos[r:r + 1], bias, center, heads, 1, 0.25)
                assert torch.equal(alone[0], full[r]), (case, r)


def test_attn_relbias_refusals_launch_nothing(dev):
    def call(rows=3, heads=2, d=16, nk=8, rpe=1, entries=3, ldk=None, off=0, ncol=9, ldb=None, no_pos=False):
        c = heads * d
        q = torch.zeros((rows, c), device=dev)
        k = torch.zeros((entries, nk, ldk or c), device=dev)
        out = torch.full((rows, c), 7.0, device=dev)
        pos = torch.zeros((rows,), device=dev, dtype=torch.int32)
        bias = torch.zeros((heads, ncol), device=dev)
        p = ops._attn_relbias_params(q, k, k, out, None, pos, bias, 4, heads, d, nk, rpe, 1.0)
        p.ldk = p.ldv = ldk or c
        p.k = k.data_ptr() + off
        if ldb is not None:
            p.ldb = ldb
        if no_pos:
            p.pos = None
        rc = _lib.load().saspa_attn_relbias(p, None)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote the output"
        return rc
    assert call(d=12) == _lib.SASPA_ERANGE                           # d % 8
    assert call(heads=1, d=136) == _lib.SASPA_ERANGE                 # d > 128
    assert call(nk=1025) == _lib.SASPA_ERANGE
    assert call(rpe=1025, entries=1) == _lib.SASPA_ERANGE
    assert call(ldk=34) == _lib.SASPA_EALIGN
    assert call(off=4) == _lib.SASPA_EALIGN
    assert call(rpe=3, entries=1, rows=6) == _lib.SASPA_EINVAL       # 1 entry x 3 rows < 6 rows
    assert call(ldb=4) == _lib.SASPA_EINVAL                          # a table pitch shorter than its columns
    assert call(no_pos=True) == _lib.SASPA_EINVAL
    q, k, v, ln, pos, bias, center = R.rel_operands((4, 16, 7, 1, 0), torch.float32, 0)
    assert torch.isfinite(_rel_dev(dev, q, k, v, ln, pos, bias, center, 4, 1, 0.25)).all()      # an accepted call writes


# ---- saspa_sample_topk -----------------------------------------------------------------------------------------------------------
def _sample_dev(dev, x, vocab, u, temperature, top_k, top_p):
    tok, logp, _ = ops.sample_topk(x.to(dev), vocab, u.to(dev), temperature=temperature, top_k=top_k, top_p=top_p)
    return tok.cpu().long(), logp.cpu()


@pytest.mark.parametrize("vocab", R.SAMPLE_VOCABS)
def test_sample_topk_equals_float64_where_it_decides(dev, vocab):
    total = und = 0
    worst_lp = 0.0
    for temperature, top_k, top_p in R.SAMPLE_GRID:
        x, u = R.sample_operands(64, vocab, 0)
        assert u[0] == 0.0 and u[1] == 1.0 - 2.0 ** -24
        s = R.sample_ref64(x, vocab, temperature, top_k, top_p, u)
        tok, logp = _sample_dev(dev, x, vocab, u, temperature, top_k, top_p)
        assert bool(((tok >= 0) & (tok < vocab)).all())
        dec = s["decidable"]
        total += 64
        und += int((~dec).sum())
        assert torch.equal(tok[dec], s["tok"][dec]), (temperature, top_k, top_p, tok, s["tok"])
        # log-probability under the kept distribution: <= 50 fp32 terms, relative error of p below 1e-5 -> 1e-4 absolute on the log
        dlp = (logp.double() - s["logp"])[dec].abs().max().item()
        worst_lp = max(worst_lp, dlp)
        assert dlp < 1e-4, (temperature, top_k, top_p, dlp)
        # pad columns: +1e30 there moved nothing -- the same launch on zero padding is bit-identical
        x0 = x.clone()
        x0[:, vocab:] = 0.0
        tok0, logp0 = _sample_dev(dev, x0, vocab, u, temperature, top_k, top_p)
        assert torch.equal(tok0, tok) and torch.equal(logp0, logp)
        # a row alone is the same row inside the batch, bit for bit
        for r in (0, 1, 37):
            t1, l1 = _sample_dev(dev, x[r:r + 1], vocab, u[r:r + 1], temperature, top_k, top_p)
            assert int(t1[0]) == int(tok[r]) and torch.equal(l1[0], logp[r])
    print(f"sample_topk vocab {vocab}: {und} of {total} cases undecidable in float64; max |dlogp| {worst_lp:.2e}")
    assert und <= 0.02 * total, (und, total)


def test_sample_topk_exact_ties_and_boundaries(dev):
    """Two exactly equal best logits: kept probabilities 1/2 and 1/2 in any arithmetic.  Ties go to the lowest id; the draw takes the
    first token whose cumulative mass EXCEEDS u (u = 0.5 moves on); top_p = 0.5 is REACHED by the first token alone."""
    x = torch.randn((4, 48), generator=torch.Generator().manual_seed(2))
    x[:, 40:] = 1e30
    x[:, 7] = x[:, 30] = 50.0
    u = torch.tensor([0.0, 0.25, 0.5, 0.75])
    for temperature in (1.0, 0.7):
        tok, logp = _sample_dev(dev, x, 40, u, temperature, 2, 1.0)
        assert tok.tolist() == [7, 7, 30, 30] and torch.equal(logp, torch.full((4,), float(np.log(np.float32(0.5)))))
        tok, logp = _sample_dev(dev, x, 40, u, temperature, 2, 0.5)
        assert tok.tolist() == [7, 7, 7, 7] and bool((logp == 0.0).all())
        tok, _ = _sample_dev(dev, x, 40, u, temperature, 1, 1.0)                 # greedy: the lowest id of the tie, whatever u
        assert tok.tolist() == [7, 7, 7, 7]
    # top_k beyond the vocabulary is clamped to it
    x8 = torch.zeros((1, 8))
    x8[0, :3] = torch.tensor([1.0, 3.0, 2.0])
    tok, _ = _sample_dev(dev, x8, 3, torch.tensor([0.999]), 1.0, 50, 1.0)
    assert tok.tolist() == [0]                                                   # the last of the three kept, in descending order


def test_sample_topk_refusals_launch_nothing(dev):
    lib = _lib.load()
    x = torch.zeros((2, 48), device=dev)
    u = torch.zeros((2,), device=dev)
    buf = torch.full((2, 2), 7, device=dev, dtype=torch.int32)

    def call(ld=48, vocab=40, temperature=1.0, top_k=5, top_p=1.0, off=0):
        rc = lib.saspa_sample_topk(x.data_ptr() + off, ld, vocab, 2, temperature, top_k, top_p, u.data_ptr(), buf[0].data_ptr(),
                                   buf[1].data_ptr(), None)
        torch.cuda.synchronize()
        assert bool((buf == 7).all()), "a refused call wrote the output"
        return rc
    assert call(top_k=0) == _lib.SASPA_ERANGE and call(top_k=65) == _lib.SASPA_ERANGE
    assert call(temperature=0.0) == _lib.SASPA_EINVAL and call(temperature=float("inf")) == _lib.SASPA_EINVAL
    assert call(top_p=0.0) == _lib.SASPA_EINVAL and call(top_p=1.5) == _lib.SASPA_EINVAL
    assert call(ld=32) == _lib.SASPA_EINVAL                          # ld < vocab
    assert call(ld=46, vocab=40) == _lib.SASPA_EALIGN
    assert call(off=4) == _lib.SASPA_EALIGN
    tok, _, _ = ops.sample_topk(x, 40, u, top_k=64)                  # an accepted call writes
    assert tok.tolist() == [0, 0]


# ---- the tiny model ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_case():
    """Weights, inputs and the CPU reference's results, computed once for the module and never changed."""
    cfg = CFG.tiny_t5()
    sd = W.t5_synth_state_dict(cfg, R.WEIGHT_SEED)
    ids, lens = R.tiny_inputs(cfg)
    dec = torch.randint(2, cfg["vocab"], (8, 9), generator=torch.Generator().manual_seed(5))
    dec[:, 0] = cfg["decoder_start"]
    ref, emu = R.Ref(sd, cfg), R.Ref(sd, cfg, emul=torch.bfloat16)
    enc, enc16 = ref.encode(ids, lens), emu.encode(ids, lens)
    logits, logits16 = ref.decoder_logits(enc, lens, dec), emu.decoder_logits(enc16, lens, dec)
    u = torch.rand((8, 20), generator=torch.Generator().manual_seed(R.UNIFORM_SEED))
    u11 = torch.rand((11, 20), generator=torch.Generator().manual_seed(R.GROUP_UNIFORM_SEED))
    greedy = ref.generate(ids, lens, do_sample=False, max_length=20)[0]
    sampled = ref.generate(ids, lens, do_sample=True, top_k=50, top_p=0.9, temperature=0.7, max_length=20, uniforms=u)[0]
    group = ref.generate(ids[2:3].expand(11, -1), lens[2:3].expand(11), do_sample=True, top_k=50, top_p=1.0, temperature=1.0,
                         max_length=20, uniforms=u11)[0]
    return dict(cfg=cfg, sd=sd, ids=ids, lens=lens, dec=dec, enc=enc, enc16=enc16, logits=logits, logits16=logits16, u=u, u11=u11,
                greedy=greedy, sampled=sampled, group=group)


def _maxrel(got, ref, live=None):
    d = (got.double().cpu() - ref.double()).abs()
    if live is not None:
        d, ref = d[live], ref[live]
    return (d.max() / ref.abs().max()).item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_model_against_reference(dev, tiny_case, dtype):
    c = tiny_case
    gen = T5Generator(c["sd"], c["cfg"], dev, dtype)
    live = torch.arange(20)[None] < c["lens"][:, None]
    enc = gen.encode(c["ids"], c["lens"])
    logits = gen.teacher_forced_logits((enc, c["lens"]), c["dec"])
    rel_e, rel_l = _maxrel(enc, c["enc"], live), _maxrel(logits, c["logits"])
    # the bf16 bar: 2x the distance of the reference's own bf16 emulation (rounding at the device's storage points) from its fp32 run
    emu_e, emu_l = _maxrel(c["enc16"], c["enc"], live), _maxrel(c["logits16"], c["logits"])
    bar_e, bar_l = (3e-4, 3e-4) if dtype == torch.float32 else (2 * emu_e, 2 * emu_l)
    print(f"tiny T5 {dtype}: encoder max-rel {rel_e:.3e} (bar {bar_e:.3e}), teacher-forced logits (9 positions) max-rel {rel_l:.3e} "
          f"(bar {bar_l:.3e}); bf16 emulation vs fp32 reference: encoder {emu_e:.3e}, logits {emu_l:.3e}")
    assert rel_e < bar_e and rel_l < bar_l


def test_decisions_fp32(dev, tiny_case):
    c = tiny_case
    gen = T5Generator(c["sd"], c["cfg"], dev, torch.float32)
    greedy = gen.generate(c["ids"], c["lens"], do_sample=False, max_length=20)
    assert greedy.shape == tuple(c["greedy"].shape) and np.array_equal(greedy, c["greedy"].numpy()), (greedy, c["greedy"])
    sampled = gen.generate(c["ids"], c["lens"], do_sample=True, top_k=50, top_p=0.9, temperature=0.7, max_length=20, uniforms=c["u"])
    assert sampled.shape == tuple(c["sampled"].shape) and np.array_equal(sampled, c["sampled"].numpy()), (sampled, c["sampled"])
    # 11 samples of one input: one encoder pass, its cross K / V shared by a group of 8 and a group of 3
    ids11, lens11 = c["ids"][2:3].expand(11, -1), c["lens"][2:3].expand(11)
    assert gen.plan_rows(ids11, lens11)[1:] == ([0, 0], list(range(11)) + [-1] * 5, 8)
    group = gen.generate(ids11, lens11, do_sample=True, top_k=50, top_p=1.0, temperature=1.0, max_length=20, uniforms=c["u11"])
    assert np.array_equal(group, c["group"].numpy()), (group, c["group"])
    # bf16: reported, never asserted
    g16 = T5Generator(c["sd"], c["cfg"], dev, torch.bfloat16).generate(c["ids"], c["lens"], do_sample=False, max_length=20)
    same = sum(g16[i].tolist() == c["greedy"][i].tolist() for i in range(8)) if g16.shape == tuple(c["greedy"].shape) else 0
    print(f"greedy: bf16 agrees with the reference on {same} of 8 id sequences")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sequence_alone_equals_itself_in_a_batch_of_13(dev, tiny_case, dtype):
    c = tiny_case
    cfg = c["cfg"]
    gen = T5Generator(c["sd"], cfg, dev, dtype)
    ids, lens = R.tiny_inputs(cfg, seed=77, n=13)
    ids[5], lens[5] = ids[4], lens[4]                                # one repeated input: it shares an entry inside the batch
    u = torch.rand((13, 20), generator=torch.Generator().manual_seed(4))
    kw = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7, max_length=20)
    batch = gen.generate(ids, lens, uniforms=u, **kw)
    for i in (0, 4, 5, 12):
        alone = gen.generate(ids[i:i + 1], lens[i:i + 1], uniforms=u[i:i + 1], **kw)[0]
        assert batch[i, :len(alone)].tolist() == alone.tolist() and bool((batch[i, len(alone):] == cfg["pad"]).all()), i


# ---- full width, once ------------------------------------------------------------------------------------------------------------
def test_full_width_once(dev):
    cfg = CFG.T5_COMMON_GEN
    sd = W.t5_synth_state_dict(cfg, 0)
    gen = T5Generator(sd, cfg, dev, torch.float32)
    g = torch.Generator().manual_seed(3)
    lens = torch.tensor([12, 5, 9, 1])
    ids = torch.zeros((4, 12), dtype=torch.long)
    for i, ln in enumerate(lens.tolist()):
        ids[i, :ln - 1] = torch.randint(3, cfg["vocab"], (ln - 1,), generator=g)
        ids[i, ln - 1] = cfg["eos"]
    enc = gen.encode(ids, lens)
    first = gen.teacher_forced_logits((enc, lens), torch.full((4, 1), cfg["decoder_start"]))
    assert first.shape == (4, 1, cfg["vocab"]) and torch.isfinite(first).all()
    ref = R.Ref(sd, cfg)
    renc = ref.encode(ids, lens)
    rlog = ref.decoder_logits(renc, lens, torch.full((4, 1), cfg["decoder_start"]))
    live = torch.arange(12)[None] < lens[:, None]
    rel_e, rel_l = _maxrel(enc, renc, live), _maxrel(first, rlog)
    print(f"full-width T5 fp32: encoder max-rel {rel_e:.3e}, first-step logits max-rel {rel_l:.3e}")
    assert rel_e < 5e-4 and rel_l < 5e-4                             # the captioner's full-width bar
    out = gen.generate(ids, lens, do_sample=True, max_length=6, generator=torch.Generator().manual_seed(0))
    assert out.shape[0] == 4 and 2 <= out.shape[1] <= 6 and out[:, 0].tolist() == [cfg["decoder_start"]] * 4 and (out < cfg["vocab"]).all()


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_entry_point_writes_the_file_and_run_aug_plans_on_it(dev, tmp_path, monkeypatch):
    from saspa_aug_amd import run_aug, utils
    from saspa_aug_amd.prompts_engineering import txt2sentance_prompts as TP
    monkeypatch.setattr(TP, "T5_CONFIG", CFG.tiny_t5())
    monkeypatch.chdir(tmp_path)                                      # the synthetic dataset materialises under ./data
    for k, v in dict(SASPA_SYNTHETIC_T5="1", SASPA_DATASET="synthetic", SASPA_T2S_NUM="11", SASPA_T2S_ALL_CLASSES="1",
                     SASPA_T2S_OUTPUT_DIR=str(tmp_path / "prompts"), SASPA_T2S_KEYWORDS="t", SASPA_PRECISION="fp32").items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("SASPA_WEIGHTS_DIR", raising=False)
    runpy.run_path(os.path.join(ROOT, "run_aug", "write_txt2sentence.py"), run_name="__main__")
    path = tmp_path / "prompts" / "LE_11_synthetic_all_classes_True.json"
    data = json.load(open(path))
    ds = run_aug.dataset_utils.DS_UTILS_DICT["synthetic"]()
    assert list(data) == ds.get_classes() and all(1 <= len(v) <= 11 and len(set(v)) == len(v) for v in data.values())
    s = run_aug.Settings(DATASET="synthetic", PROMPT_TYPE="txt2sentence-per_class", NUM_PER_IMAGE=2, SEED=3, USE_ARTISTIC_PROMPTS=False,
                         PROMPT_WITH_SUB_CLASS=False, PROMPTS_FILE=str(path))
    c2p = run_aug.read_prompts_from_json(s.PROMPTS_FILE, s.DATASET, per_class=True)
    utils.set_seed(s.SEED)
    items = run_aug.plan_work(s, ds.original_images_paths[:4], None, str(tmp_path / "out"), ds.get_image_stem_to_class_str_dict(),
                              image_size_fn=lambda p: (64, 64), class_to_prompts=c2p)
    assert len(items) == 8 and all(it.prompt for it in items)
    # without the variable the same run refuses
    monkeypatch.delenv("SASPA_SYNTHETIC_T5")
    with pytest.raises(RuntimeError, match="SASPA_SYNTHETIC_T5"):
        runpy.run_path(os.path.join(ROOT, "run_aug", "write_txt2sentence.py"), run_name="__main__")
