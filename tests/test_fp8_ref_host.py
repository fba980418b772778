"""CPU proof of the conditions tests/test_fp8_gpu.py holds the quantising LayerNorm and the fp8 emission to (tests/fp8_ref.py): the
byte rule accepts the fp32 emulation with no excluded element and rejects round-toward-zero, the row-scale tolerance is 4x the
emulation's worst case, the byte-difference cap is at least 4x what two legitimate emulations disagree on."""
import pytest
import torch

from tests import fp8_ref as R
from tests.test_errbudget import _rand


@pytest.mark.parametrize("rows,c,one_channel", [(r, c, False) for r, c in R.LN_CASES] + [(77, 640, True)])
def test_ln_byte_rule_accepts_rne_rejects_round_toward_zero(rows, c, one_channel):
    x, g, b = R.ln_case(_rand, rows, c, seed=3 if one_channel else 1)
    if one_channel:
        g, b = R.ln_one_channel_affine(c)
    y, sc, mag = R.ln_quant_ref(x, g, b)
    q, s = R.ln_quant_emul(x, g, b)
    rel = ((s.double() - sc) / sc).abs().max().item()
    print(f"{rows}x{c}: scale off by {rel:.2e} relative")
    assert rel <= R.LN_SCALE_MEASURED * 1.001 and R.LN_SCALE_RTOL == 4 * R.LN_SCALE_MEASURED
    assert not R.ln_quant_violations(q, s, y, mag).any()
    qt, st = R.ln_quant_emul(x, g, b, to_bytes=R.e4m3_bytes_rtz)
    share = R.ln_quant_violations(qt, st, y, mag).double().mean().item()
    print(f"{rows}x{c}: round-toward-zero violates the byte rule on {share:.3f} of the elements")
    assert share > 0.25


def test_ln_zero_gamma_beta_and_constant_row():
    x, g, b = R.ln_case(_rand, 5, 640)
    q, s = R.ln_quant_emul(x, torch.zeros_like(g), torch.zeros_like(b))
    assert (s == 1.0).all() and (q & 0x7f == 0).all()
    y, _, _ = R.ln_quant_ref(x, g, b)
    assert torch.equal(y[1], b.double())                                     # the constant row: y = beta exactly


def test_byte_share_cap_is_four_times_the_disagreement_of_legitimate_emulations():
    share = R.byte_disagreement(_rand)
    print(f"forward / reversed K-tiles, exp2 / libm exp: {share:.2e} of the emitted bytes differ")
    assert R.BYTE_SHARE_CAP >= max(4 * share, 1e-4)


def test_e4m3_helpers():
    v = torch.tensor([0.0, 2.0 ** -9, 0.0146, 1.0, 1.0625, 1.07, 17.0, 447.0, 500.0, -3.3])
    b = R.e4m3_bytes(v)
    assert R.e4m3_decode(b).tolist() == [0.0, 2.0 ** -9, 0.015625 - 2.0 ** -9, 1.0, 1.0, 1.125, 16.0, 448.0, 448.0, -3.25]
    assert R.e4m3_decode(R.e4m3_bytes_rtz(v)).tolist() == [0.0, 2.0 ** -9, 0.013671875, 1.0, 1.0, 1.0, 16.0, 416.0, 448.0, -3.25]
    assert R.code_distance(R.e4m3_bytes(torch.tensor([2.0 ** -9])), R.e4m3_bytes(torch.tensor([-2.0 ** -9]))).item() == 2
