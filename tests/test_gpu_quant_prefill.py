"""One-pass prefill of the quantised dense runners (weight_format fp8, fp8b128, mxfp4, int4g128, int8g128): each projection is unpacked on
the device (samd_gemm_unpack_*) into a scratch matrix and multiplied by the library, everything else is _prefill_wide as it stands.

THE EXACT CRITERION.  The model-dtype twin of a quantised runner is a runner whose projections ARE the Python-dequantised weights in the
dtype (fp8.dequantize_rows / dequantize_blocks, mxfp4.dequantize_blocks, int4 / int8.dequantize_groups of what quantising on load produces,
rounded once to the dtype).  Its _prefill_wide is unchanged code, and after the unpack the quantised runner issues the same calls on the same
operands, so cache length, kv_rows(N), the last logits, the start token and every on_chunk slice (tokens, logits, hidden states) are equal
BIT FOR BIT: no tolerance.  On a library without the unpack path the quantised runner takes 64-row chunks through the streaming kernels,
whose sums are accumulated in another order, and the comparison fails.

Tiny Llama: hidden 512, 4 heads / 2 KV heads of 128, intermediate 768, 2 layers, vocabulary 1024 -- q|k|v [1024, 512], o [512, 512],
gate|up [1536, 512], down [512, 768]: every projection has >= 2 tiles and >= 2 chunks, down has 3 chunks.  Prompts of 128 (the forced
switch-over itself), 200 and 257 tokens with SAMD_QUANT_PREFILL_MIN_ROWS=128.  One Qwen2-shaped (q|k|v bias) case in int8g128 and one
Qwen3-shaped (q / k norm) case in mxfp4."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import samd_hip
from samd_hip import fp8 as F8
from samd_hip import int4 as I4
from samd_hip import int8 as I8
from samd_hip import mxfp4 as MX
from samd_hip.llama import LlamaRunner
from test_gpu_fp8_runner import linears
from test_gpu_lm_shapes import hf_llama
from test_gpu_mxfp4_runner import _near_tie

ENV = "SAMD_QUANT_PREFILL_MIN_ROWS"
CFG = dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=1024,
           max_position_embeddings=512, rms_norm_eps=1e-5, head_dim=128)
FORMATS = ("fp8", "fp8b128", "mxfp4", "int4g128", "int8g128")
DTYPES = [torch.float16, torch.bfloat16]
PROMPTS = (128, 200, 257)
T = 64


def dequantised(W, fmt, dtype):
    """the weights a `fmt` runner in `dtype` that quantises W (already in `dtype`) on load multiplies by, in `dtype`"""
    if fmt == "fp8":
        return F8.dequantize_rows(*F8.quantize_rows(W)).to(dtype)
    if fmt == "fp8b128":
        return F8.dequantize_blocks(*F8.quantize_blocks(W)).to(dtype)
    if fmt == "mxfp4":
        return MX.dequantize_blocks(*MX.quantize_blocks(W, dtype)).to(dtype)
    mod = I4 if fmt == "int4g128" else I8
    return mod.dequantize_groups(*mod.quantize_groups(W, dtype)).to(dtype)


def pair(lm, fmt, dtype, max_cache_len=512):
    """(the quantised runner of lm, its model-dtype twin).  Quantising is per row, per group or block along k, or per 128 x 128 block, and
    every part of q|k|v and gate|up has a multiple of 128 rows, so quantising the parts equals quantising the fused matrices."""
    lm = lm.to(dtype)
    twin_lm = copy.deepcopy(lm)
    with torch.no_grad():
        for lin, src in zip(linears(twin_lm), linears(lm)):
            assert lin.weight.shape[0] % 128 == 0
            lin.weight.copy_(dequantised(src.weight.detach(), fmt, dtype))
    quant = LlamaRunner.from_hf(lm, max_cache_len=max_cache_len, dtype=dtype, weight_format=fmt)
    twin = LlamaRunner.from_hf(twin_lm, max_cache_len=max_cache_len, dtype=dtype, weight_format=dtype)
    assert quant.weight_format == fmt and quant.row_major_released and quant.max_draft_rows() == 64 and quant.tune_prefill() == {}
    assert twin.weight_format is None and not twin.row_major_released
    return quant, twin


def start_token(sess):
    torch.cuda.synchronize()
    out = C.c_int32(-1)
    rc = C.CDLL("libamdhip64.so").hipMemcpy(C.byref(out), C.c_void_p(sess.device_views()["start_token"]), C.c_size_t(4), 2)    # device to host
    assert rc == 0
    return out.value


def run(runner, prompt, with_chunks):
    runner.kv.zero_()
    sess = samd_hip.Session(runner.max_len)
    calls = []
    cb = (lambda tok, lg, n, hid: calls.append((n, tok[:n].clone(), lg[:n].clone(), hid[:n].clone()))) if with_chunks else None
    logits = runner.prefill(sess, torch.tensor([prompt], device="cuda"), cb).clone()
    torch.cuda.synchronize()
    k, v = runner.kv_rows(len(prompt))
    return dict(logits=logits, start=start_token(sess), k=k.clone(), v=v.clone(), calls=calls, cache_length=sess.get_cache_length())


def assert_same_bits(got, want, N, label):
    assert got["cache_length"] == want["cache_length"] == N, label
    assert bool(torch.isfinite(want["logits"].float()).all()) and bool(want["k"].float().abs().sum() > 0), label
    assert torch.equal(got["k"], want["k"]) and torch.equal(got["v"], want["v"]), (label, "kv_rows")
    assert torch.equal(got["logits"], want["logits"]), (label, "last logits", (got["logits"].float() - want["logits"].float()).abs().max().item())
    assert got["start"] == want["start"], label
    assert len(got["calls"]) == len(want["calls"]), label
    for c, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a[0] == b[0] == min(T, N - T * c), (label, c)
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), (label, c, "on_chunk's tokens, logits or hidden states")


def compare(quant, twin, vocab, monkeypatch, label):
    monkeypatch.setenv(ENV, "128")
    monkeypatch.delenv("SAMD_PREFILL", raising=False)
    for N in PROMPTS:
        prompt = np.random.default_rng(N).integers(3, vocab, N).tolist()
        for with_chunks in (False, True):
            got, want = run(quant, prompt, with_chunks), run(twin, prompt, with_chunks)
            assert len(want["calls"]) == (-(-N // T) if with_chunks else 0)
            assert_same_bits(got, want, N, f"{label} N={N} on_chunk={with_chunks}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_pass_prefill_equals_the_model_dtype_twin_bit_for_bit(fmt, dtype, monkeypatch):
    quant, twin = pair(hf_llama(CFG, seed=31, std=0.05), fmt, dtype)
    for k in ("wqkv", "wo", "wgu", "wdown"):
        n, kk = quant.w["layers"][0][k].shape
        assert n // 128 >= 2 and kk // 256 >= 2
    assert quant.w["layers"][0]["wdown"].shape[1] // 256 == 3
    compare(quant, twin, CFG["vocab_size"], monkeypatch, f"{fmt} {dtype}")
    assert quant.row_major_released and quant.max_draft_rows() == 64, "no row-major copy comes back"


@pytest.mark.parametrize("kind,fmt,dtype", [("qwen2", "int8g128", torch.float16), ("qwen3", "mxfp4", torch.bfloat16)])
def test_qwen_shapes_equal_their_twins(kind, fmt, dtype, monkeypatch):
    from test_gpu_qwen import TINY, hf_qwen
    quant, twin = pair(hf_qwen(kind, dict(intermediate_size=768), seed=23), fmt, dtype)
    assert quant.qkv_epilogue and (quant.shape.qkv_bias, quant.shape.qk_norm) == ((True, False) if kind == "qwen2" else (False, True))
    compare(quant, twin, TINY["vocab_size"], monkeypatch, f"{kind} {fmt} {dtype}")


def test_chunked_mode_keeps_the_64_row_loop(monkeypatch):
    """SAMD_PREFILL=chunked: the streaming kernels in 64-row chunks as before -- the same cache length, no scratch, and the arg-max of the
    last logits wherever the twin's own wide and chunked prefills agree on it (where they do not, the row is a near-tie of the arithmetic)"""
    quant, twin = pair(hf_llama(CFG, seed=32, std=0.05), "int4g128", torch.float16)
    monkeypatch.setenv(ENV, "128")
    decided = 0
    for N in PROMPTS:
        prompt = np.random.default_rng(100 + N).integers(3, CFG["vocab_size"], N).tolist()
        monkeypatch.setenv("SAMD_PREFILL", "chunked")
        got, t_chunked = run(quant, prompt, True), run(twin, prompt, True)
        monkeypatch.delenv("SAMD_PREFILL")
        t_wide = run(twin, prompt, True)
        assert got["cache_length"] == t_wide["cache_length"] == N
        assert len(got["calls"]) == -(-N // T) and [c[0] for c in got["calls"]] == [min(T, N - c0) for c0 in range(0, N, T)]
        for a, b, c in zip(got["calls"], t_wide["calls"], t_chunked["calls"]):
            agree = b[2].float().argmax(-1) == c[2].float().argmax(-1)
            assert torch.equal(a[2].float().argmax(-1)[agree], b[2].float().argmax(-1)[agree]), N
            decided += int(agree.sum())
        if t_wide["start"] == t_chunked["start"]:
            assert got["start"] == t_wide["start"]
    assert decided > 0, "the arg-max comparison did not pass empty"
    assert "quant_prefill_scratch" not in quant.memory_report(), "a chunked prefill allocates no scratch"


def test_short_prompts_keep_the_chunks_and_a_bad_override_raises(monkeypatch):
    quant, twin = pair(hf_llama(CFG, seed=33, std=0.05), "fp8", torch.bfloat16)
    monkeypatch.delenv("SAMD_PREFILL", raising=False)
    prompt = np.random.default_rng(7).integers(3, CFG["vocab_size"], 200).tolist()
    monkeypatch.setenv(ENV, "256")                               # 200 < 256: chunks, so no scratch
    run(quant, prompt, False)
    assert "quant_prefill_scratch" not in quant.memory_report()
    monkeypatch.setenv(ENV, "192")                               # 200 >= 192: one pass
    got = run(quant, prompt, False)
    assert "quant_prefill_scratch" in quant.memory_report()
    assert_same_bits(got, run(twin, prompt, False), 200, "fp8 bf16 at a switch-over of 192")
    for bad in ("100", "64", "lots"):
        monkeypatch.setenv(ENV, bad)
        with pytest.raises(samd_hip.SamdError, match=ENV):
            quant.prefill(samd_hip.Session(512), torch.tensor([prompt], device="cuda"))


def test_scratch_is_reported_after_the_first_one_pass_prefill_only(monkeypatch):
    quant, _ = pair(hf_llama(CFG, seed=34, std=0.05), "int8g128", torch.float16)
    monkeypatch.setenv(ENV, "128")
    monkeypatch.delenv("SAMD_PREFILL", raising=False)
    before, bytes_before = quant.memory_report(), quant.weight_bytes()
    assert "quant_prefill_scratch" not in before
    run(quant, list(range(3, 73)), False)                        # 70 tokens: below the switch-over
    assert "quant_prefill_scratch" not in quant.memory_report()
    run(quant, list(range(3, 203)), False)
    after = quant.memory_report()
    largest = max(t.shape[0] * t.shape[1] for k, t in quant.w["layers"][0].items() if k in I8.PROJECTIONS)
    assert largest == 1536 * 512 and after["quant_prefill_scratch"] == 2 * largest         # one [max N x K] matrix in the model dtype
    assert {k: v for k, v in after.items() if k != "quant_prefill_scratch"} == before      # nothing else moved, "total" included
    assert quant.weight_bytes() == bytes_before
    run(quant, list(range(3, 303)), False)                       # kept, not grown or re-allocated
    assert quant.memory_report() == after and quant.row_major_released


def _dequantised_lm(fmt, seed):
    """a tiny fp16 model whose projections hold the dequantised weights: HF's forward on it is the near-tie oracle of the runner that
    quantises it on load (quantising a dequantised matrix gives the same codes back)"""
    lm = hf_llama(CFG, seed=seed, std=0.05)
    with torch.no_grad():
        for lin in linears(lm):
            lin.weight.copy_(dequantised(lin.weight.detach().to(torch.float16), fmt, torch.float16))
    return lm


@pytest.mark.parametrize("fmt", FORMATS)
def test_speculative_equals_autoregressive_after_a_one_pass_prefill(fmt, monkeypatch):
    """evaluation/equal.py's criterion behind a 200-token prompt that takes the one-pass prefill: SAM-drafted decoding == the greedy output
    of the same quantised runner; only a near-tie may split them, and only past len(prompt) + 8 (the allowance of the formats' own
    _ar_and_spec tests)"""
    import samd_sam_only as SO
    lm = _dequantised_lm(fmt, 41)
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", fmt)
    monkeypatch.setenv(ENV, "128")
    monkeypatch.delenv("SAMD_PREFILL", raising=False)
    rng = np.random.default_rng(2)
    prompt = rng.integers(3, CFG["vocab_size"], 200).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=512)
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    seq_ar = ar.generate(ids, generation_config=gcfg).output_ids[0]
    assert ar._runner.weight_format == fmt and "quant_prefill_scratch" in ar._runner.memory_report()
    docs = [seq_ar[len(prompt):]] + [rng.integers(3, CFG["vocab_size"], 50).tolist() for _ in range(4)] + [[i] for i in range(CFG["vocab_size"])]
    cfg = SO.SamdConfig(max_predicts=16, alpha=4.0, len_bias=0)
    spec = SO.SamdModel(cfg, lm, SO.DraftModel(cfg, sam_static=SO.build_sam(docs, 2), device="cuda"), eos_token_id=2, dtype=torch.float16, device="cuda")
    out = spec.generate(ids, generation_config=gcfg)
    assert spec._runner.weight_format == fmt and "quant_prefill_scratch" in spec._runner.memory_report()
    seq = out.output_ids[0]
    assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
    m = min(len(seq), len(seq_ar))
    diff = [i for i in range(m) if seq[i] != seq_ar[i]]
    if diff:
        i = diff[0]
        assert i > len(prompt) + 8 and _near_tie(lm, seq[:i], seq[i], seq_ar[i]), f"diverged at {i}"
