"""The tables of weight formats (samd_hip/formats.py: DENSE_FORMATS; samd_hip/moe.py: EXPERT) against what they must agree with: the
served names, the library's prototypes, the wide calls' codes, and the raw-dict conventions by which a format is detected.  No device."""
import re

import pytest
import torch

import samd_hip
from samd_hip import SamdError, formats as FM, llama as LL, moe as MOE

P = samd_hip._PROTOS
LABELS = {"fp8": "float8_e4m3fn", "fp8b128": "block-scaled FP8", "mxfp4": "MXFP4", "int4g128": "INT4 (AWQ / GPTQ)", "int8g128": "INT8 (GPTQ)"}


def test_one_record_per_served_name():
    assert [f.name for f in FM.DENSE_FORMATS] == list(LL.QUANT_FORMATS) == list(LABELS) and FM.DENSE == {f.name: f for f in FM.DENSE_FORMATS}
    assert sorted(n for n in MOE.EXPERT if n is not None) == sorted(n for n in MOE.EXPERT_FORMATS_SERVED if n is not None)
    assert all(MOE.EXPERT[n].name == n for n in MOE.EXPERT)
    assert {f.name: f.label for f in FM.DENSE_FORMATS} == LABELS


def test_entry_points_exist_with_the_argument_counts_the_call_sites_pass():
    one, two = torch.zeros(1), (torch.zeros(1), torch.zeros(1))
    for f in FM.DENSE_FORMATS:
        n_ptr = len(f.tensors(two if f.codes_per_scale is None else one))
        assert n_ptr == (2 if f.name in ("fp8", "fp8b128") else 1)
        assert f.packer in P
        assert len(P[f.gemm][1]) == 1 + n_ptr + 8, f.gemm         # a, the weight pointers, RP, n, k, splits, partials, out, dtype, stream
        assert len(P[f.unpack][1]) == n_ptr + 5, f.unpack         # the weight pointers, N, K, out, dtype, stream
    for f in MOE.EXPERT.values():
        assert len(P["samd_moe_gate_up_silu" + f.launch_suffix][1]) == 11 and len(P["samd_moe_down_combine" + f.launch_suffix][1]) == 14
        assert hasattr(MOE, f.packer)


def test_suffixes_are_distinct_and_wide_codes_are_the_served_ones():
    assert len({f.suffix for f in FM.DENSE_FORMATS}) == len(FM.DENSE_FORMATS)
    assert [f.suffix for f in FM.DENSE_FORMATS] == ["_f8", "_f8b", "_f4", "_i4", "_i8"]
    assert len({f.launch_suffix for f in MOE.EXPERT.values()}) == len(MOE.EXPERT)
    assert {n: f.wide_code for n, f in MOE.EXPERT.items()} == MOE.WIDE_FORMAT_CODES_SERVED and 4 not in MOE.WIDE_FORMAT_CODES_SERVED.values()


def raw_weights(fmt, N=128, K=256):
    """one layer whose four projections arrive in `fmt`, as from_hf leaves them"""
    u8 = lambda *sz: torch.zeros(sz, dtype=torch.uint8)
    f8 = lambda *sz: torch.zeros(sz, dtype=torch.float8_e4m3fn)
    side = {"fp8": lambda: {"": f8(N, K), "_scale": torch.ones(N)},
            "fp8b128": lambda: {"": f8(N, K), "_sinv": torch.ones(N // 128, K // 128)},
            "mxfp4": lambda: {"": u8(N, K // 2), "_e8": u8(N, K // 32)},
            "int4g128": lambda: {"": u8(N, K // 2), "_z": u8(N, K // 128), "_s": torch.ones(N, K // 128, dtype=torch.float16)},
            "int8g128": lambda: {"": u8(N, K), "_z8": u8(N, K // 128), "_s8": torch.ones(N, K // 128, dtype=torch.float16)}}[fmt]
    layer = {k + sfx: t for k in FM.PROJECTIONS for sfx, t in side().items()}
    assert tuple(side()) == FM.DENSE[fmt].raw_keys
    return dict(layers=[layer])


@pytest.mark.parametrize("fmt", list(LABELS))
def test_a_raw_dict_is_detected_as_its_format_and_only_that(fmt):
    w = raw_weights(fmt)
    assert [f.name for f in FM.DENSE_FORMATS if f.carried_by(w)] == [fmt]
    assert LL._weight_format(None, w, torch.float16) == fmt == LL._weight_format(fmt, w, torch.float16)
    plain = dict(layers=[{k: torch.zeros(128, 256, dtype=torch.float16) for k in FM.PROJECTIONS}])
    assert not any(f.carried_by(plain) for f in FM.DENSE_FORMATS) and LL._weight_format(None, plain, torch.float16) is None


@pytest.mark.parametrize("fmt", list(LABELS))
def test_the_refusal_of_another_weight_format_reads_as_before(fmt):
    w = raw_weights(fmt)
    general = rf"the weights carry {re.escape(LABELS[fmt])} projections; weight_format .* would need them dequantised \(pass None or '{fmt}'\)"
    pinned = {"fp8b128": (r"the weights carry block-scaled FP8 projections; .*pass None or 'fp8b128'", "block-scaled FP8 projections.*pass None or 'fp8b128'"),
              "fp8": (r"the weights carry float8_e4m3fn projections; .*pass None or 'fp8'\)",)}.get(fmt, ())
    for other in ["fp16", torch.float16] + [n for n in LABELS if n != fmt]:
        for rx in (general,) + pinned:
            with pytest.raises(SamdError, match=rx):
                LL._weight_format(other, w, torch.float16)
