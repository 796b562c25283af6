"""Act-order GPTQ on the GPU ("Act-order GPTQ"): the three permuting launches against the launches they derive
from, by equality; one act-order projection end to end against float64 on the naturally ordered weights; a two-layer act-order model
through LlamaRunner.from_hf against fp32 HuggingFace on the dequantised natural-order weights, with a model-dtype runner as yardstick."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import samd_hip
from samd_hip import _ptr, check, current_stream, lib, torch_dtype_code
from samd_hip import int4 as I4
from samd_hip.formats import DENSE
from samd_hip.llama import LlamaRunner
from test_act_order_cpu import ORDERED, QUANT, act_order_module, cfg, dequant_natural, random_codes, random_g_idx
from test_gpu_int4_gemm import TOL as TOL4
from test_gpu_int8_gemm import TOL as TOL8

DTYPES = [torch.float16, torch.bfloat16]
ROWS = [1, 5, 16, 64]


def tables(K, seed):
    """a fixed-seed random permutation, the identity and the reversal, int32 on the device"""
    g = torch.Generator().manual_seed(seed)
    return [t.to(torch.int32).cuda() for t in (torch.randperm(K, generator=g), torch.arange(K), torch.arange(K - 1, -1, -1))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("K", [256, 1280])
def test_permuting_norm_is_the_norm_indexed_by_the_table(dtype, rows, K):
    L, dt, st = lib(), torch_dtype_code(dtype), current_stream()
    g = torch.Generator(device="cuda").manual_seed(K + rows)
    x0 = torch.randn((rows, K), generator=g, device="cuda").to(dtype)
    w = (1 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dtype)
    part = torch.randn((3, rows, K), generator=g, device="cuda")
    # no residual, a residual in the model dtype, a residual as three fp32 split-K partials
    for delta, n_p, stride in ((None, 0, 0), (part[0].to(dtype).contiguous(), 0, 0), (part, 3, rows * K)):
        xa, want = x0.clone(), torch.full((rows, K), float("nan"), device="cuda", dtype=dtype)
        check(L.samd_rmsnorm(_ptr(xa), _ptr(delta), _ptr(w), _ptr(want), rows, K, 1e-5, dt, n_p, stride, st))
        for perm in tables(K, seed=K):
            xb, got = x0.clone(), torch.full((rows, K), float("nan"), device="cuda", dtype=dtype)
            check(L.samd_rmsnorm_perm(_ptr(xb), _ptr(delta), _ptr(w), _ptr(got), rows, K, 1e-5, dt, n_p, stride, _ptr(perm), None, st))
            assert torch.equal(got.view(torch.int16), want[:, perm.long()].view(torch.int16)) and torch.equal(xa.view(torch.int16), xb.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", ROWS + [70])                   # 70: four-row tiles with a short last one
@pytest.mark.parametrize("K", [256, 1280])
def test_gather_cols(dtype, rows, K):
    x = torch.randn((rows, K), generator=torch.Generator(device="cuda").manual_seed(rows), device="cuda").to(dtype)
    for perm in tables(K, seed=K + 1):
        out = torch.full((rows, K), float("nan"), device="cuda", dtype=dtype)
        check(lib().samd_gather_cols(_ptr(x), _ptr(perm), _ptr(out), rows, K, torch_dtype_code(dtype), current_stream()))
        assert torch.equal(out.view(torch.int16), x[:, perm.long()].view(torch.int16))
        inplace = x.clone()
        check(lib().samd_gather_cols(_ptr(inplace), _ptr(perm), _ptr(inplace), rows, K, torch_dtype_code(dtype), current_stream()))
        assert torch.equal(inplace.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("heads,kv_heads", [(2, 2), (4, 2)])
@pytest.mark.parametrize("vt", [0, 1])
def test_permuting_attention_output(dtype, rows, heads, kv_heads, vt):
    """the merge with a table t puts element c at column t[c]: the existing launch's output indexed by the inverse of t"""
    L, dt, st, max_len, cached = lib(), torch_dtype_code(dtype), current_stream(), 512, 300
    g = torch.Generator(device="cuda").manual_seed(rows + heads)
    q = torch.randn((64, heads, 128), generator=g, device="cuda").to(dtype)          # (buffers as the runner sizes them: whole row tiles)
    k, v = (torch.randn((kv_heads, max_len, 128), generator=g, device="cuda").to(dtype) for _ in range(2))
    mask = torch.tensor([((1 << (i + 1)) - 1) - ((1 << 64) if i == 63 else 0) for i in range(64)] + [0] * 192, dtype=torch.int64, device="cuda")
    d_L = torch.tensor([cached], dtype=torch.int32, device="cuda")
    d_n = torch.tensor([rows if rows < 5 else rows - 2], dtype=torch.int32, device="cuda")       # rows >= n are zeroed by both
    ws_bytes = L.samd_tree_attention_workspace(rows, heads, 128)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    args = lambda out: (_ptr(q), _ptr(k), _ptr(v), _ptr(out), dt, rows, heads, kv_heads, 128, max_len, _ptr(mask), _ptr(d_L), _ptr(d_n),
                        1.0 / 128 ** 0.5, _ptr(ws), ws_bytes)
    want = torch.full((64, heads * 128), float("nan"), device="cuda", dtype=dtype)
    check((L.samd_tree_attention_vt if vt else L.samd_tree_attention_warm)(*args(want), None, st))
    assert torch.isfinite(want[:rows].float()).all()
    for t in tables(heads * 128, seed=heads):
        got = torch.full((64, heads * 128), float("nan"), device="cuda", dtype=dtype)
        check(L.samd_tree_attention_perm(*args(got), vt, _ptr(t), None, st))
        assert torch.equal(got.view(torch.int16), want[:, torch.argsort(t.long())].view(torch.int16))     # (rows past n_q_pad: untouched NaN bits in both)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("K,g", [(512, 128), (1024, 256)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_projection_end_to_end(bits, K, g, dtype):
    """GPTQ tensors with a random g_idx -> the public importer -> the packer -> samd_gather_cols + the streaming GEMM, against
    x.double() @ dequant(W).double().T with W dequantised in the checkpoint's own K order.  Exact-integer inputs (power-of-two scales, x in
    -4 .. 4: every partial sum a multiple of 1/8 below 2^24) by equality; random inputs within test_gpu_int4_gemm / test_gpu_int8_gemm's
    tolerance for these kernels."""
    N, rows, fmt, L, dt, st = 256, 16, DENSE["int4g128" if bits == 4 else "int8g128"], lib(), torch_dtype_code(dtype), current_stream()
    gi = random_g_idx(K, g, seed=K)
    for exact in (True, False):
        codes, z, s = random_codes(bits, N, K, g, seed=K + bits, pow2_scales=exact)
        q, zz, ss, perm = ORDERED[bits](act_order_module(bits, codes, z, s, gi, g), "p", config=cfg(bits, g))
        raw = dict(zip(("w" + sfx for sfx in fmt.raw_keys), (q, zz, ss)))
        packed = fmt.pack(raw, "w", "cuda", dtype, dt)
        gen = torch.Generator(device="cuda").manual_seed(K)
        x = (torch.randint(-4, 5, (rows, K), generator=gen, device="cuda") if exact else torch.randn((rows, K), generator=gen, device="cuda")).to(dtype)
        xp, part = torch.empty_like(x), torch.full((2, rows, N), float("nan"), device="cuda")
        table = perm.to(torch.int32).cuda()
        check(L.samd_gather_cols(_ptr(x), _ptr(table), _ptr(xp), rows, K, dt, st))
        check(getattr(L, fmt.gemm)(_ptr(xp), *fmt.pointers(packed), rows, N, K, 2, _ptr(part), None, dt, st))
        got = part.double().sum(0)
        want = x.double() @ dequant_natural(codes, z, s, gi, dtype).cuda().double().t()
        if exact:
            assert torch.equal(got, want)
        else:
            bound = (TOL4 if bits == 4 else TOL8)[dtype] * max(1.0, want.abs().max().item())
            err = (got - want).abs().max().item()
            print(f"act-order projection {bits}-bit K={K} g={g} {dtype}: err {err:.3e}, bound {bound:.3e}")
            assert err <= bound


CFG = dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
           max_position_embeddings=512, rms_norm_eps=1e-5, head_dim=128)
SHARED = {"q_proj": "in", "k_proj": "in", "v_proj": "in", "o_proj": "o", "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "down"}


def to_act_order_checkpoint(lm, bits, dtype):
    """an act-order GPTQ checkpoint of lm -- every projection quantised per group of 128 ALONG ITS g_idx, codes stored in natural K order --
    and lm itself with the projections replaced by the dequantised natural-order weights"""
    from test_gpu_fp8_runner import PROJ
    Q, ck = QUANT[bits], copy.deepcopy(lm)
    for li, (lyr, lyr_ref) in enumerate(zip(ck.model.layers, lm.model.layers)):
        g_idx = {}
        for a, b in PROJ:
            lin = getattr(getattr(lyr_ref, a), b)
            gi = g_idx.setdefault(SHARED[b], random_g_idx(lin.in_features, 128, seed=10 * li + len(g_idx)))
            perm = torch.argsort(gi.long(), stable=True).cuda()
            q, z, s = Q.quantize_groups(lin.weight.detach().to(dtype)[:, perm], dtype)            # the groups of W[:, perm] are g_idx's
            codes = (I4.unpack_nibbles(q) if bits == 4 else q)[:, I4.inverse_perm(perm)]
            assert int(z.min()) >= 1
            mod = act_order_module(bits, codes.cpu(), z.cpu(), s.to(torch.float16).cpu(), gi)
            setattr(getattr(lyr, a), b, mod.cuda())
            with torch.no_grad():
                lin.weight.copy_(dequant_natural(codes, z, s, gi.cuda(), dtype))
    ck.config.quantization_config = cfg(bits)
    return ck


@pytest.mark.parametrize("bits,dtype", [(4, torch.float16), (8, torch.bfloat16)])
def test_act_order_runner_against_the_model_dtype_twin(bits, dtype):
    """from_hf on an act-order checkpoint, no extra argument: chunked prefill (96 tokens), one-pass prefill (256), verify steps of 5 and 33
    rows, against fp32 HuggingFace on the dequantised natural-order weights.  The yardstick is a model-dtype runner holding those weights,
    under test_gpu_int4_runner's bound with that runner in HF low precision's place: err(act-order) <= 1.5 x err(twin) + 0.02.  Not bit
    equality: the K order of every sum differs.  Then 32 greedy tokens of generate() agree, up to a near-tie of the fp32 logits."""
    from test_gpu_lm_shapes import hf_llama
    from test_gpu_mxfp4_runner import _near_tie
    lm = hf_llama(CFG, seed=31 + bits, std=0.05)
    ck = to_act_order_checkpoint(lm, bits, dtype)
    runner = LlamaRunner.from_hf(ck, max_cache_len=512, dtype=dtype)
    assert runner.weight_format == f"int{bits}g128" and runner.act_order == [True, True] and runner.memory_report()["act_order_tables"] == 2 * 4 * 4 * 512
    twin = LlamaRunner.from_hf(lm, max_cache_len=512, dtype=dtype)
    assert twin.weight_format is None and twin.act_order == [False, False]
    rng = np.random.default_rng(bits)
    for P in (96, 256):
        prompt = rng.integers(3, 512, P).tolist()
        drafts = [rng.integers(3, 512, n).tolist() for n in (5, 33)]
        with torch.no_grad():
            ref = [lm(input_ids=torch.tensor([prompt + d], device="cuda")).logits[0, P - 1:].float() for d in drafts]
        errs = []
        for r in (runner, twin):
            sess = samd_hip.Session(512)
            e = [(r.prefill(sess, torch.tensor([prompt], device="cuda")).float() - ref[0][0]).abs().max().item()]
            for d, want in zip(drafts, ref):
                n = len(d)
                got = r.forward_tokens(sess, torch.tensor(d, dtype=torch.int32, device="cuda"), torch.arange(n, dtype=torch.int32, device="cuda"),
                                       r.pf_mask, n, P)
                e.append((got.float() - want[1:]).abs().max().item())
            errs.append(e)
        print(f"act-order int{bits} {dtype} P={P}: prefill / 5 rows / 33 rows  ours {errs[0]}  twin {errs[1]}")
        assert all(a <= 1.5 * t + 0.02 for a, t in zip(*errs)), errs
    assert getattr(runner, "_qpf_scratch", None) is not None                  # the 256-token prompt took the one-pass form
    # greedy generate(): the act-order checkpoint and the dequantised module, each through its own runner
    import samd_sam_only as SO
    prompt = rng.integers(3, 512, 40).tolist()
    ids, gcfg, ar = torch.tensor([prompt], device="cuda"), SO.SamdGenerationConfig(max_new_tokens=32, max_cache_len=512), SO.SamdConfig(max_predicts=1)
    seqs = [SO.SamdModel(ar, m, SO.DraftModel(ar, device="cuda"), eos_token_id=2, dtype=dtype, device="cuda").generate(ids, generation_config=gcfg).output_ids[0]
            for m in (ck, lm)]
    diff = [i for i in range(min(map(len, seqs))) if seqs[0][i] != seqs[1][i]]
    assert not diff or _near_tie(lm, seqs[0][:diff[0]], seqs[0][diff[0]], seqs[1][diff[0]]), diff[:3]
