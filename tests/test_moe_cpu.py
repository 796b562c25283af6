"""Qwen3-MoE support without a GPU: the float64 restatement of the sparse block (tests/moe_ref.py) against HF's own Qwen3MoeSparseMoeBlock,
shape and sparse-layer parsing from the config, the layer guards of from_hf with every rejection (on CPU-built modules, before any device
work), and static checks of the compiled kernels inside libsamd_hip.so."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from samd_hip import SamdError
from samd_hip import moe as MOE
from samd_hip.llama import LlamaRunner, LlamaShape
import moe_ref as M
from test_codeobject_cpu import READELF, SO, gfx950_code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
TINY = dict(hidden_size=256, intermediate_size=512, moe_intermediate_size=256, num_hidden_layers=4, num_attention_heads=2, num_key_value_heads=1,
            head_dim=128, vocab_size=300, max_position_embeddings=512, rms_norm_eps=1e-6, num_experts=8, num_experts_per_tok=2)


def qwen3_moe(**kw):
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(**dict(TINY, **kw))
    return cfg, Qwen3MoeForCausalLM(cfg)


@pytest.mark.parametrize("norm_topk", [True, False])
@pytest.mark.parametrize("E,k", [(8, 2), (128, 8)])
def test_restatement_matches_hf_sparse_block_in_float64(E, k, norm_topk):
    """HF's block in float64 keeps its logits unrounded and runs its softmax in fp32 (softmax(..., dtype=torch.float)), as the restatement
    does: outputs agree to float64 round-off on every row whose k-th / (k + 1)-th probability is not an exact tie"""
    from transformers import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeSparseMoeBlock
    cfg = Qwen3MoeConfig(hidden_size=64, moe_intermediate_size=32, num_experts=E, num_experts_per_tok=k, norm_topk_prob=norm_topk)
    torch.manual_seed(E + k)
    blk = Qwen3MoeSparseMoeBlock(cfg).double()
    with torch.no_grad():
        for p in blk.parameters():
            p.normal_(std=0.3)
        x = torch.randn(1, 60, 64, dtype=torch.float64)
        want = blk(x)[0]
        _, hf_w, hf_idx = blk.gate(x[0])
    got, logits, idx, w = M.block(x[0], blk.gate.weight, blk.experts.gate_up_proj, blk.experts.down_proj, k, norm_topk, torch.float64)
    probs = torch.softmax(logits.float(), dim=-1).sort(dim=-1, descending=True).values
    clear = probs[:, k - 1] > probs[:, k]
    assert int(clear.sum()) >= 55
    assert torch.equal(idx[clear].sort(dim=-1).values, hf_idx[clear].sort(dim=-1).values)
    scale = want.abs().max().item()
    assert (got - want)[clear].abs().max().item() <= 1e-12 * scale, ((got - want)[clear].abs().max().item(), scale)
    # the tie rule and the rounding of the weights
    lg = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 2.0]], dtype=torch.float64)
    eye = torch.eye(6, dtype=torch.float64)
    _, i2, w2 = M.route(lg, eye, 3, True, torch.bfloat16)
    assert i2.tolist() == [[1, 2, 4]] and torch.equal(w2, w2.to(torch.bfloat16).double()) and abs(float(w2.sum()) - 1) < 0.02


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,k,H,R", [(128, 8, 2048, 64), (8, 2, 512, 64), (64, 4, 1024, 64), (256, 8, 768, 64)])
def test_planted_router_inputs_are_decided_by_the_reference_alone(dtype, E, k, H, R):
    """the inputs of the GPU router test, built the same way on the CPU: at most 2 % of the rows are undecided under the fp32 accumulation
    bound, and no decided row has two selected logits closer than the bound"""
    g = torch.Generator().manual_seed(E + k)
    router = M.orthogonal_router(E, H, g, "cpu").to(dtype)
    h = M.planted_rows(router, R, k, g).to(dtype)
    decided, bound = M.decided_rows(h, router, k)
    assert int((~decided).sum()) <= 0.02 * R
    assert torch.equal(M.ordered_rows(h, router, k), decided)
    assert float(bound.max()) < 0.05


def test_draft_head_runner_is_rejected_before_device_work():
    cfg, lm = qwen3_moe()
    with pytest.raises(SamdError, match="draft head"):
        LlamaRunner.from_hf(lm, 256, device="cpu", draft_head=True)


def test_shape_reads_the_moe_fields_and_the_sparse_layer_map():
    cfg, _ = qwen3_moe(norm_topk_prob=True)
    s = LlamaShape(cfg)
    assert (s.model_type, s.n_experts, s.top_k, s.moe_inter, s.norm_topk, s.qk_norm, s.qkv_bias) == ("qwen3_moe", 8, 2, 256, True, True, False)
    assert s.sparse == [True] * 4 and s.moe
    assert LlamaShape(qwen3_moe(mlp_only_layers=[0])[0]).sparse == [False, True, True, True]
    assert LlamaShape(qwen3_moe(decoder_sparse_step=2)[0]).sparse == [False, True, False, True]
    assert LlamaShape(qwen3_moe(mlp_only_layers=[1], decoder_sparse_step=2, norm_topk_prob=False)[0]).sparse == [False, False, False, True]
    s0 = LlamaShape(qwen3_moe(num_experts=0)[0])
    assert not s0.moe and s0.sparse == [False] * 4
    for i in range(4):                                           # exactly Qwen3MoeDecoderLayer.__init__'s decision
        cfg, lm = qwen3_moe(mlp_only_layers=[i], decoder_sparse_step=1 + i % 2)
        assert LlamaShape(cfg).sparse == LlamaRunner._hf_sparse_layers(lm.model.layers)
    # dense models know nothing of it
    from transformers import LlamaConfig
    d = LlamaShape(LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, vocab_size=300))
    assert not d.moe and d.sparse == [False, False] and d.n_experts == 0


@pytest.mark.parametrize("kw", [dict(hidden_size=384, num_attention_heads=3), dict(moe_intermediate_size=320), dict(num_experts=257),
                                dict(num_experts=16, num_experts_per_tok=9), dict(num_experts=4, num_experts_per_tok=5)])
def test_shapes_the_kernels_do_not_serve_raise_at_load(kw):
    cfg, lm = qwen3_moe(**kw)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaShape(cfg)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_layer_guard_accepts_sparse_and_mixed_stacks():
    for kw in ({}, dict(mlp_only_layers=[0]), dict(decoder_sparse_step=2), dict(mlp_only_layers=[0, 1, 2, 3])):
        cfg, lm = qwen3_moe(**kw)
        assert LlamaRunner._hf_layer_extras(lm.model.layers) == (False, True)
        assert LlamaRunner._hf_sparse_layers(lm.model.layers) == LlamaShape(cfg).sparse
        with pytest.raises(SamdError, match="no MI355X"):        # everything is accepted up to the point where the device is needed
            LlamaRunner.from_hf(lm, 256, device="cpu")


def test_dense_modules_return_what_they_did():
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen2Config, Qwen2ForCausalLM, Qwen3Config, Qwen3ForCausalLM
    kw = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, vocab_size=300)
    for C, Mod, want in ((LlamaConfig, LlamaForCausalLM, (False, False)), (Qwen2Config, Qwen2ForCausalLM, (True, False)), (Qwen3Config, Qwen3ForCausalLM, (False, True))):
        lm = Mod(C(**kw))
        assert LlamaRunner._hf_layer_extras(lm.model.layers) == want
        assert LlamaRunner._hf_sparse_layers(lm.model.layers) == [False, False]
        s = LlamaShape(lm.config)
        assert not s.moe and (s.qkv_bias, s.qk_norm) == want


def test_shared_expert_and_other_mlp_parameters_are_rejected_by_name():
    cfg, lm = qwen3_moe()
    mlp = lm.model.layers[1].mlp
    mlp.shared_expert = torch.nn.Linear(256, 256, bias=False)
    with pytest.raises(SamdError, match="shared expert"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    cfg, lm = qwen3_moe()
    lm.model.layers[2].mlp.gate.register_parameter("e_score_correction_bias", torch.nn.Parameter(torch.zeros(8)))
    with pytest.raises(SamdError, match="e_score_correction_bias"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    cfg, lm = qwen3_moe()
    lm.model.layers[0].mlp.experts.register_parameter("down_proj_bias", torch.nn.Parameter(torch.zeros(8, 256)))
    with pytest.raises(SamdError, match="down_proj_bias"):
        LlamaRunner.from_hf(lm, 256, device="cpu")
    cfg, lm = qwen3_moe()                                        # a sparse layer the config does not imply
    lm.config.mlp_only_layers = [3]
    with pytest.raises(SamdError, match="sparse MLP layers"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


@pytest.mark.parametrize("kw,match", [(dict(weight_format="fp8"), "fp8"), (dict(weight_format="mxfp4"), "mxfp4"), (dict(native_gemm=False), "native_gemm")])
def test_quantised_experts_and_the_library_gemm_path_are_rejected(kw, match):
    cfg, lm = qwen3_moe(mlp_only_layers=[0])
    with pytest.raises(SamdError, match=match):
        LlamaRunner.from_hf(lm, 256, device="cpu", **kw)
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu", **kw)


def test_weight_format_from_the_environment_is_rejected_too(monkeypatch):
    monkeypatch.setenv("SAMD_WEIGHT_FORMAT", "fp8")
    cfg, lm = qwen3_moe()
    with pytest.raises(SamdError, match="mixture-of-experts"):
        LlamaRunner.from_hf(lm, 256, device="cpu")


def test_eagle_heads_refuse_a_moe_base_module_and_a_moe_head():
    from samd.tree_model.eagle2 import Eagle2, Eagle2Head
    head_cfg = dict(hidden_size=256, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2, vocab_size=300, rms_norm_eps=1e-5, bias=True)
    _, lm = qwen3_moe()
    with pytest.raises(SamdError, match="mixture-of-experts"):
        Eagle2(None, lm, torch.float32, "cpu", head=Eagle2Head(head_cfg, dtype=torch.float32, device="cpu"))
    with pytest.raises(SamdError, match="draft head"):
        MOE.reject_unsupported(draft_head=True)


def _kernels():
    blob = open(SO, "rb").read()
    for k, co in enumerate(gfx950_code_objects(blob)):
        yield k, co


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(READELF)), reason="needs the built library and llvm-readelf")
def test_moe_kernels_are_in_the_library_and_use_no_scratch(tmp_path):
    kernels = {}
    for k, co in _kernels():
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for block in notes.split(".name:")[1:]:
            name = block.split()[0]
            get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            kernels[name] = dict(scratch=get("private_segment_fixed_size"), vgpr_spills=get("vgpr_spill_count"))
    count = lambda frag: len([n for n in kernels if frag in n])
    # the two expert GEMMs: 2 dtypes x 4 row tiles; router and combine: 2 dtypes; lists and pack: one each
    assert (count("k_moe_gate_up_silu"), count("k_moe_down"), count("k_moe_route"), count("k_moe_combine"), count("k_moe_lists"), count("k_moe_pack")) == \
        (8, 8, 2, 2, 1, 1), sorted(n for n in kernels if "k_moe_" in n)
    bad = {n: v for n, v in kernels.items() if "k_moe_" in n and (v["scratch"] or v["vgpr_spills"])}
    assert not bad, f"the mixture-of-experts kernels must not spill or use scratch: {bad}"


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")
def test_no_register_copy_touches_an_in_flight_load_destination_of_the_expert_gemms(tmp_path):
    """the check of test_mxfp4_codeobject_cpu.py on the two expert GEMMs: their weight loads are hand-issued in-out operands of one value each, so
    in the prologue (first hand-issued load to the first barrier behind it) no v_mov reads or writes a load destination"""
    found = 0
    for k, co in _kernels():
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        text = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
        for chunk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            head = chunk.split("\n", 1)[0]
            if "k_moe_gate_up_silu" not in head and "k_moe_down" not in head:
                continue
            found += 1
            body = [l.split("//")[0].strip() for l in chunk.split("\n")[1:]]
            dests, load_at = set(), []
            for i, l in enumerate(body):
                m = re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\d+, s\[\d+:\d+\].* nt", l)      # (the hand-issued form: SGPR base, nt)
                if m:
                    dests |= set(range(int(m.group(1)), int(m.group(2)) + 1))
                    load_at.append(i)
            assert len(load_at) >= 16, head
            assert any("global_load_lds_dwordx4" in l for l in body), f"{head}: the A tile is not filled by LDS-DMA"
            barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier") and i > load_at[0])
            bad = []
            for i in range(load_at[0], barrier):
                m = re.match(r"v_mov_b32_e32 v(\d+), (?:v(\d+))?", body[i])
                if m and (int(m.group(1)) in dests or (m.group(2) is not None and int(m.group(2)) in dests)):
                    bad.append(body[i])
            assert not bad, f"{head}: register copies of hand-issued load destinations: {bad[:8]}"
    assert found == 16, f"expected 16 expert GEMM instantiations (2 kernels x 2 dtypes x 4 row tiles), found {found}"
