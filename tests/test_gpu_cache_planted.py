"""After any number of speculative steps, cache rows [0, L) of every layer are the K and V of the committed text t[0 .. L) -- as a float64
teacher-forced forward of that text computes them (tests/cache_planting.py: invariant, reference, metric, bar, workloads, faults; the CPU
proof that every named fault lies >= 10 bars (bf16) / >= 100 bars (fp16) outside is tests/test_cache_planting_cpu.py).

A driver of its own runs DecodeEngine.start / .step over ScriptedAcceptance(runner, ...) with the workload's static automaton and
parameters -- the loop of SamdModel._run, keeping every StepReport.  Every step's (type, n, accept, kv_index[:accept], is_tree) and cache
length equal the CPU simulation's record.  After every step, once the stream is idle, every cache row at or past the new L -- every layer,
K and V or V^T, through the runner's own storage -- is overwritten with NaN: those rows are dead (the next step writes its n rows before
anything reads them), so a kernel that reads one, or a compaction that leaves a committed row outside [0, L), shows as a NaN or a gross
error below L.  The prefill runs over an all-NaN cache.  At the end: e <= 1.5 x e_twin + 2 ulp for every (layer, K|V) over all L
committed rows, no NaN below L, finite logits of the last verify.

MEASURED on the MI355X, e of the runner / e_twin of HuggingFace in the model dtype on the same GPU (`base` workload, 42 steps, 232 committed
rows, 2 KV heads; the bar is 1.5 x e_twin + 2 ulp):

                                  layer-0 K          layer-0 V          layer-1 K          layer-1 V
  fp16  dense (both V layouts,    0.00110 / 0.00147  0.00107 / 0.00107  0.00204 / 0.00227  0.00249 / 0.00202
        graphs on and off)
  bf16  dense (likewise)          0.00915 / 0.01047  0.00675 / 0.00675  0.02019 / 0.01667  0.01765 / 0.01514
  fp16  4 KV heads                0.00112 / 0.00135  0.00092 / 0.00092  0.00218 / 0.00227  0.00206 / 0.00231
  fp16  SAMD_NORM_FOLD=0          0.00110 / 0.00147  0.00107 / 0.00107  0.00204 / 0.00227  0.00226 / 0.00202
  fp16  block attention           0.00110 / 0.00147  0.00107 / 0.00107  0.00200 / 0.00227  0.00197 / 0.00202
  fp16  sweep (357 rows)          0.00112 / 0.00170  0.00107 / 0.00107  0.00212 / 0.00281  0.00190 / 0.00231
  bf16  wide (323 rows)           0.00972 / 0.01166  0.00675 / 0.00675  0.01568 / 0.01830  0.01537 / 0.01537
  fp16  end of the cache          0.00109 / 0.00126  0.00107 / 0.00107  0.00207 / 0.00228  0.00195 / 0.00221
  fp16  Qwen2 shape               0.00104 / 0.00123  0.00079 / 0.00079  0.00208 / 0.00225  0.00218 / 0.00207
  bf16  Qwen3 shape               0.01483 / 0.01534  0.00708 / 0.00708  0.03654 / 0.04392  0.03309 / 0.04538
  fp16  fp8                       0.00123 / 0.00155  0.00086 / 0.00084  0.00237 / 0.00201  0.00202 / 0.00170
  bf16  fp8b128                   0.00947 / 0.01126  0.00679 / 0.00804  0.01570 / 0.01523  0.01796 / 0.01662
  fp16  mxfp4                     0.00105 / 0.00144  0.00080 / 0.00080  0.00186 / 0.00187  0.00172 / 0.00179
  bf16  int4g128                  0.00842 / 0.01121  0.00700 / 0.00700  0.01482 / 0.01547  0.01639 / 0.01525
  fp16  int8g128                  0.00099 / 0.00150  0.00095 / 0.00095  0.00183 / 0.00178  0.00177 / 0.00190
  fp16  generate, greedy (166)    0.00099 / 0.00137  0.00083 / 0.00083  0.00253 / 0.00214  0.00179 / 0.00180
  fp16  Token Recycle (128)       0.00109 / 0.00121  0.00107 / 0.00107  0.00193 / 0.00204  0.00263 / 0.00231
  fp16  EAGLE-2 (118)             0.00114 / 0.00136  0.00107 / 0.00107  0.00225 / 0.00240  0.00208 / 0.00187

The largest e / e_twin is 1.23 (fp16 dense, layer-1 V) and the largest e / bar 0.62 (the same tensor): every configuration meets 1.5 x, no
kernel was changed.  Layer-0 V equals the twin's to the printed digits wherever the projection is one product of the same rounded weights.
32 tests in 10 s; the slowest are the first dense case (1.5 s: it builds the models, the references and the automaton that the others
share), the fp8 / mxfp4 / INT cases (0.2 - 0.35 s: a model and a runner of their own) and the EAGLE-2 run (0.3 s).

A FINDING ABOUT THE TEST'S OWN INPUTS.  A master that holds dequantize(quantize(W)) and a runner that quantises THAT on load agree for fp8,
fp8b128 and mxfp4, but not for int4g128 / int8g128: the min / max group quantiser does not return its own codes (2 - 10 % of the weights
move, by up to 4.8 % / 0.5 % of the largest), and the cache then misses the bar on every tensor (e up to 4 x e_twin).  The INT cases
therefore import checkpoint modules that carry the codes, as tests/test_gpu_int4_runner.py and tests/test_gpu_int8_runner.py do.
"""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import cache_planting as P
import samd_hip
from samd_hip.engine import DecodeEngine, ScriptedAcceptance
from samd_hip.llama import LlamaRunner
from samd_sam_only.sam._common import so_params

F16, BF16 = torch.float16, torch.bfloat16


# ---- shared, read-only ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def model(kind, kv_heads, fmt=None, dtype=None):
    """(fp32 module on the GPU, float64 master on the CPU, the module the runner is made from).  With a weight format the projections of
    the first hold the Python-dequantised weights, as the formats' own runner tests build them, so master, twin and runner multiply by the
    same numbers: fp8 / fp8b128 / mxfp4 quantise those on load (which gives the same codes back); the min / max quantiser of the INT
    formats does not return its own codes, so there the runner imports a checkpoint module that carries them."""
    if kind == "llama":
        lm = P.tiny_llama(kv_heads, seed=1 + kv_heads, device="cuda")
    else:
        lm = P.tiny_qwen(kind, seed=17)
    source = lm
    if fmt in ("int4g128", "int8g128"):
        from test_gpu_int4_runner import to_int4_checkpoint
        from test_gpu_int8_runner import to_int8_checkpoint
        source = to_int4_checkpoint(lm, dtype, "awq") if fmt == "int4g128" else to_int8_checkpoint(lm, dtype, "gptq_v2")
    elif fmt is not None:
        from test_gpu_fp8_runner import linears
        from test_gpu_quant_prefill import dequantised
        with torch.no_grad():
            for lin in linears(lm):
                lin.weight.copy_(dequantised(lin.weight.detach().to(dtype), fmt, dtype).float())
    return lm, P.as_master(lm), source


@lru_cache(maxsize=None)
def twin(key, dtype):
    return P.low_precision_twin(model(*key)[0], dtype)


@lru_cache(maxsize=None)
def references(key, dtype, text):
    """(float64 reference cache of `text`, e_twin [layers, 2]) -- computed once per model, dtype and committed text"""
    want = P.reference_cache(model(*key)[1], list(text))
    return want, P.cache_error(P.reference_cache(twin(key, dtype), list(text)), want)


@lru_cache(maxsize=None)
def plan(name):
    w = P.build_workload(name)
    recs = P.simulate(w)
    P.assert_plan(name, recs)
    return w, recs, samd_hip.StaticAutomaton.build(w["docs"], w["eos"], 0).upload()


class Recording(ScriptedAcceptance):
    """ScriptedAcceptance that remembers the buffers of every bucket it ran"""

    def verify(self, session, R, rows_fetch=None):
        b = super().verify(session, R, rows_fetch=rows_fetch)
        self.buffers = getattr(self, "buffers", {})
        self.buffers[R] = b
        return b


def poison_dead_rows(runner, L):
    """NaN into every cache row at or past L, in the layout the runner keeps"""
    s = runner.shape
    runner.kv[:, 0, :, L:] = float("nan")
    if runner.v_transposed:
        for li in range(s.layers):
            runner.kv[li, 1].view(s.kv_heads, s.head_dim, runner.max_len)[:, :, L:] = float("nan")
    else:
        runner.kv[:, 1, :, L:] = float("nan")


def committed_rows(runner, L):
    k, v = runner.kv_rows(L)
    return torch.stack([k, v], dim=1).double().cpu()


def hold_cache(runner, key, dtype, text, label):
    L = len(text)
    torch.cuda.synchronize()
    got = committed_rows(runner, L)
    want, e_twin = references(key, dtype, tuple(text))
    e, bar = P.cache_error(got, want), P.bar(e_twin, dtype)
    print(f"{label}: L={L}  " + "  ".join(f"{n} e {a:.5f} e_twin {b:.5f} bar {c:.5f}" for n, a, b, c in
                                           zip(P.NAMES, e.flatten().tolist(), e_twin.flatten().tolist(), bar.flatten().tolist())))
    assert not bool(torch.isnan(got).any()), f"{label}: NaN in a committed row"
    assert bool((e <= bar).all()), (label, e.tolist(), bar.tolist())
    return e, e_twin


def drive(key, name, dtype, monkeypatch, *, graphs=True, env=(), max_cache_len=None, fold=True, **runner_kw):
    """the step loop of SamdModel._run with the checks of the module docstring; -> the runner"""
    w, recs, static = plan(name)
    monkeypatch.setenv("SAMD_QKV_FUSED", "force")
    for k, v in env:
        monkeypatch.setenv(k, v)
    max_len = max_cache_len or w["max_cache_len"]
    runner = LlamaRunner.from_hf(model(*key)[2], max_cache_len=max_len, dtype=dtype, share_weights=False, **runner_kw)
    if fold is not None:
        assert runner.norm_fold == fold
    assert w["max_predicts"] <= runner.max_draft_rows()
    target, prompt = w["target"], w["prompt"]
    sa = Recording(runner, w["vocab"], len(target))
    sa.set_target(target)
    sess = samd_hip.Session(max_len + samd_hip.MAX_DRAFT)
    eng = DecodeEngine(sa, sess, static, so_params(w["max_predicts"], w["alpha"], w["K"], w["len_bias"]), use_graphs=graphs)
    runner.kv.fill_(float("nan"))
    rep = eng.start(torch.tensor([prompt], device="cuda"))
    L = len(prompt)
    torch.cuda.synchronize()
    poison_dead_rows(runner, L)
    done = 0
    for rec in recs:
        assert L + w["max_predicts"] < max_len, "the simulation stops where the engine's rule stops"
        assert (rep.type, rep.n, L) == (rec["type"], rec["n"], rec["L"]), (done, rep.type, rep.n, L)
        n = rep.n
        rep = eng.step(n)
        assert not rep.error
        assert (rep.accept, rep.kv_index, rep.is_tree, rep.tokens) == (rec["a"], rec["kv_index"], rec["type"], rec["accepted"]), (done, rec)
        L += rep.accept
        torch.cuda.synchronize()
        assert sess.get_cache_length() == L == rec["L1"]
        poison_dead_rows(runner, L)
        done += 1
    assert done == len(recs) and (done == w["steps"] or L + w["max_predicts"] >= max_len)
    logits = sa.buffers[runner.bucket(n)]["logits"][:n]
    assert bool(torch.isfinite(logits.float()).all()), "the last verify's logits"
    label = f"{key} {name} {dtype} graphs={graphs} {dict(env)} {runner_kw} max_len={max_len}"
    hold_cache(runner, key, dtype, target[:L], label)
    return runner, eng


# ---- dense Llama -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("layout", ["t", "rows"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_dense_llama_keeps_the_committed_text(dtype, layout, graphs, monkeypatch):
    runner, eng = drive(("llama", 2), "base", dtype, monkeypatch, graphs=graphs, env=(("SAMD_V_LAYOUT", layout),))
    assert runner.v_transposed == (layout == "t")
    assert runner.rows_exact(8) == (5,) and runner.rows_exact(16) == (9,)
    if graphs:
        assert {(8, 5), (16, 9)} <= set(eng._graphs_exact), "the exact-row graphs of 5- and 9-node drafts ran"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_four_kv_heads(dtype, monkeypatch):
    drive(("llama", 4), "base", dtype, monkeypatch)


@pytest.mark.parametrize("attention", ["split3", "block"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_other_attention_modes(dtype, attention, monkeypatch):
    runner, _ = drive(("llama", 2), "base", dtype, monkeypatch, fold=False, attention=attention)
    assert runner.attention == attention and runner.v_transposed


def test_eight_launch_forward_without_the_norm_fold(monkeypatch):
    drive(("llama", 2), "base", F16, monkeypatch, env=(("SAMD_NORM_FOLD", "0"),), fold=False)


def test_cache_length_that_is_no_multiple_of_8_takes_the_row_major_cache(monkeypatch):
    runner, _ = drive(("llama", 2), "base", BF16, monkeypatch, max_cache_len=515)
    assert runner.v_transposed is False


# ---- every bucket, wide drafts, the end of the cache ------------------------------------------------------------------------------------
def test_every_row_bucket(monkeypatch):
    _, eng = drive(("llama", 2), "sweep", F16, monkeypatch)
    assert {8, 16, 32, 48, 64} <= set(eng.bucket_steps)


def test_drafts_of_more_than_64_nodes(monkeypatch):
    _, eng = drive(("llama", 2), "wide", BF16, monkeypatch)
    assert eng.bucket_steps.get(128, 0) >= 1


@pytest.mark.parametrize("layout", ["t", "rows"])
def test_the_run_up_to_the_end_of_the_cache(layout, monkeypatch):
    """max_cache_len = prompt + 40, driven until the engine's own stopping rule ends the run: the last steps' buckets are wider than what
    is left of the cache, and nothing of them may land in another head's rows (or, transposed, in another column's head)"""
    w = P.build_workload("end")
    assert w["max_cache_len"] == len(w["prompt"]) + 40
    runner, _ = drive(("llama", 2), "end", F16, monkeypatch, env=(("SAMD_V_LAYOUT", layout),))
    assert runner.v_transposed == (layout == "t")


# ---- Qwen shapes: the q|k|v epilogue launch writes the rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype", [("qwen2", F16), ("qwen3", BF16), ("qwen3", F16)])
def test_qwen_shapes(kind, dtype, monkeypatch):
    runner, _ = drive((kind, 2), "base", dtype, monkeypatch, fold=False)
    assert runner.qkv_epilogue and (runner.shape.qkv_bias, runner.shape.qk_norm) == ((True, False) if kind == "qwen2" else (False, True))


# ---- weight formats: the eight-launch layer, K / V rows from split-K partials ------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dtype", [("fp8", F16), ("fp8b128", BF16), ("mxfp4", F16), ("int4g128", BF16), ("int8g128", F16)])
def test_weight_formats(fmt, dtype, monkeypatch):
    kw = {} if fmt.startswith("int") else dict(weight_format=fmt)              # (a checkpoint module makes the runner its format by itself)
    runner, _ = drive(("llama", 2, fmt, dtype), "base", dtype, monkeypatch, fold=False, **kw)
    assert runner.weight_format == fmt and runner.row_major_released


# ---- real logits: the final cache against the run's own output ----------------------------------------------------------------------------------
def _planted_corpus(seq, n_prompt, rng):
    """the continuation as a document, and around it forks whose other branches occur more often: tree drafts that list the run's own
    continuation late"""
    cont = seq[n_prompt:]
    docs = [cont]
    for p in range(4, len(cont) - 2, 5):
        for k in range(2):
            stub = cont[max(0, p - 6):p] + rng.integers(3, P.VOCAB, 2).tolist()
            docs += [stub] * (2 + k)
    return docs + [[i] for i in range(P.VOCAB)]


def _autoregressive(lm, ids, gcfg):
    import samd_sam_only as SO
    ar_cfg = SO.SamdConfig(max_predicts=1)
    ar = SO.SamdModel(ar_cfg, lm, SO.DraftModel(ar_cfg, device="cuda"), eos_token_id=2, dtype=F16, device="cuda")
    return ar.generate(ids, generation_config=gcfg).output_ids[0]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_generate_on_real_logits_leaves_the_cache_of_its_output(sampled, monkeypatch):
    """SamdModel.generate with a static corpus on the tiny model: the committed text is output_ids.  Greedy, and one seeded sampled run
    (temperature 0.8) through the fused sampling step."""
    import random
    import samd_sam_only as SO
    monkeypatch.setenv("SAMD_QKV_FUSED", "force")
    key = ("llama", 2)
    lm = model(*key)[0]
    rng = np.random.default_rng(21)
    prompt = rng.integers(3, P.VOCAB, 70).tolist()
    ids = torch.tensor([prompt], device="cuda")
    kw = dict(greedy=False, temperature=0.8) if sampled else {}
    gcfg = SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512, **kw)
    seq_ar = _autoregressive(lm, ids, SO.SamdGenerationConfig(max_new_tokens=96, max_cache_len=512))
    cfg = SO.SamdConfig(max_predicts=24, alpha=4.0, K=8, len_bias=0)
    spec = SO.SamdModel(cfg, lm, SO.DraftModel(cfg, sam_static=SO.build_sam(_planted_corpus(seq_ar, len(prompt), rng), 2), device="cuda"),
                        eos_token_id=2, dtype=F16, device="cuda")
    torch.manual_seed(5)
    random.seed(5)
    out = spec.generate(ids, generation_config=gcfg)
    assert spec.lookup_stats["tree"][0] > 0
    print(f"lookup statistics [steps, tokens]: {dict(spec.lookup_stats)}")
    if not sampled:
        assert out.decode_steps < out.decode_tokens, "drafts were never accepted"
        assert spec.lookup_stats["tree"][1] > spec.lookup_stats["tree"][0], "no tree draft was accepted beyond its root"
    else:
        assert spec.engine.supports_fused_sampling()
    seq = out.output_ids[0]
    assert seq[:len(prompt)] == prompt and len(seq) > len(prompt) + 8
    hold_cache(spec._runner, key, F16, seq, f"generate sampled={sampled}")


def test_token_recycle_leaves_the_cache_of_its_output(monkeypatch):
    """the samd package's Token Recycle trees (compaction from the host in the plugin engine), second request of the same model"""
    import samd as S
    import samd_sam_only as SO
    key = ("llama", 2)
    lm = model(*key)[0]
    prompt = np.random.default_rng(22).integers(3, P.VOCAB, 64).tolist()
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=64, max_cache_len=512)
    cfg = S.SamdConfig(n_predicts=16, len_threshold=4, len_bias=0, tree_method="token_recycle")
    tr = S.SamdModel(cfg, lm, S.DraftModel(cfg, lm=lm, device="cuda"), eos_token_id=2, dtype=F16, device="cuda")
    for _ in range(2):
        out = tr.generate(ids, generation_config=gcfg)
    assert out.decode_steps < out.decode_tokens, "Token Recycle never got a draft accepted on a repeated request"
    hold_cache(tr._runner, key, F16, out.output_ids[0], "token recycle")


def test_eagle2_plugin_leaves_the_cache_of_its_output(monkeypatch):
    import samd as S
    import samd_sam_only as SO
    from samd.tree_model.eagle2 import Eagle2, Eagle2Head
    key = ("llama", 2)
    lm = model(*key)[0]
    prompt = np.random.default_rng(23).integers(3, P.VOCAB, 70).tolist()
    prompt[40:52] = prompt[10:22]
    ids = torch.tensor([prompt], device="cuda")
    gcfg = SO.SamdGenerationConfig(max_new_tokens=48, max_cache_len=512)
    tree_cfg = dict(hidden_size=P.CFG["hidden_size"], intermediate_size=P.CFG["intermediate_size"], num_attention_heads=P.CFG["num_attention_heads"],
                    num_key_value_heads=2, vocab_size=P.VOCAB, rms_norm_eps=1e-5, bias=True)
    cfg = S.SamdConfig(n_predicts=12, len_threshold=3, len_bias=0, tree_method="eagle2", tree_config=tree_cfg)
    head = Eagle2Head(tree_cfg, dtype=F16, device="cuda")
    head.random_init(seed=3, std=0.08)
    draft = S.DraftModel(cfg, tree_model=Eagle2(cfg, lm, F16, "cuda", head=head), lm=lm, device="cuda")
    eagle = S.SamdModel(cfg, lm, draft, eos_token_id=2, dtype=F16, device="cuda")
    out = eagle.generate(ids, generation_config=gcfg)
    assert eagle.lookup_stats["tree"][0] > 0, "the EAGLE-2 tree path never ran"
    hold_cache(eagle._runner, key, F16, out.output_ids[0], "eagle2")
