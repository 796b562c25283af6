"""The switch-over of the quantised dense runners' one-pass prefill (samd_hip.llama.quant_prefill_min_rows: the class default, the
SAMD_QUANT_PREFILL_MIN_ROWS override, every rejected value) and the five unpack entry points in the header and in the binding.  CPU only."""
import ctypes as C
import os
import re

import pytest

import samd_hip
from samd_hip import SamdError
from samd_hip.llama import QUANT_FORMATS, LlamaRunner, quant_prefill_min_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "SAMD_QUANT_PREFILL_MIN_ROWS"
UNPACK = ("samd_gemm_unpack_f8", "samd_gemm_unpack_f8b", "samd_gemm_unpack_f4", "samd_gemm_unpack_i4", "samd_gemm_unpack_i8")


def test_default_is_the_class_constant(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    d = LlamaRunner.QUANT_PF_MIN_ROWS
    assert isinstance(d, int) and d >= 128 and d % 64 == 0
    assert quant_prefill_min_rows(d) == d
    assert quant_prefill_min_rows(640) == 640                    # the argument is the default, whatever the class says
    monkeypatch.setenv(ENV, "")                                  # an empty value is an unset one
    assert quant_prefill_min_rows(d) == d
    assert QUANT_FORMATS == ("fp8", "fp8b128", "mxfp4", "int4g128", "int8g128")


@pytest.mark.parametrize("value", ["128", "192", "256", " 320 ", "4096"])
def test_override_takes_every_multiple_of_64_from_128(monkeypatch, value):
    monkeypatch.setenv(ENV, value)
    assert quant_prefill_min_rows(LlamaRunner.QUANT_PF_MIN_ROWS) == int(value)


@pytest.mark.parametrize("value,why", [("129", "multiple of 64"), ("200", "multiple of 64"), ("100", "multiple of 64"),      # not a multiple of 64
                                       ("64", ">= 128"), ("0", ">= 128"), ("-128", ">= 128"),                                  # below 128
                                       ("many", "expected an integer"), ("128.0", "expected an integer"), ("1e3", "expected an integer")])
def test_rejected_values_raise_and_name_the_rule(monkeypatch, value, why):
    monkeypatch.setenv(ENV, value)
    with pytest.raises(SamdError, match=re.escape(why)) as e:
        quant_prefill_min_rows(LlamaRunner.QUANT_PF_MIN_ROWS)
    assert ENV in str(e.value)


def test_header_declares_the_unpack_entry_points_and_the_binding_lists_them():
    hdr = open(os.path.join(ROOT, "include", "samd_hip.h")).read()
    declared = dict(re.findall(r"^int (samd_gemm_unpack_[a-z0-9]+)\s*\(([^)]*)\);", hdr, flags=re.M))
    assert tuple(sorted(declared)) == tuple(sorted(UNPACK))
    ctype = {"const void *": C.c_void_p, "void *": C.c_void_p, "const float *": C.c_void_p, "int32_t": C.c_int32}
    L = samd_hip.lib()
    for name in UNPACK:
        args = [re.match(r"(.*?)\s*\b\w+$", a.strip()).group(1).strip() for a in declared[name].split(",")]
        res, protos = samd_hip._PROTOS[name]
        assert res is C.c_int and protos == [ctype[a] for a in args], (name, args)
        assert hasattr(L, name), f"{name} declared in include/samd_hip.h but not exported"
    # the scaled forms take (packed, scales, N, K, out, dtype, stream), the others carry their side data inside the packed buffer
    assert len(samd_hip._PROTOS["samd_gemm_unpack_f8"][1]) == len(samd_hip._PROTOS["samd_gemm_unpack_f8b"][1]) == 7
    assert all(len(samd_hip._PROTOS[n][1]) == 6 for n in UNPACK[2:])
