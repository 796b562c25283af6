"""Mixture-of-experts MLP blocks (Qwen3-MoE) on the streaming kernels: which layers are sparse, the shapes the kernels serve, the expert
weights in their packed form and the three launches of a sparse layer (include/samd_hip.h: samd_moe_route, samd_moe_gate_up_silu,
samd_moe_down_combine).

A sparse layer holds `mlp.gate.weight` [E, H] (the router), `mlp.experts.gate_up_proj` [E, 2 I, H] and `mlp.experts.down_proj` [E, H, I] (this
transformers' fused form).  The experts are packed once at load -- per expert the 128-column tile layout of the dense streaming GEMM, gate
and up interleaved in groups of 64 so that a tile holds matching columns, experts end to end -- and no row-major copy is kept."""
import torch

from . import SamdError, _ptr, check, current_stream, lib

MAX_EXPERTS = 256
MAX_TOPK = 8
# the parameters of a sparse layer's MLP that the runner reads (named_parameters of an HF Qwen3MoeDecoderLayer)
SPARSE_MLP_PARAMS = ("mlp.gate.weight", "mlp.experts.gate_up_proj", "mlp.experts.down_proj")
DENSE_MLP_PARAMS = ("mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


def sparse_layer_map(n_layers, n_experts, mlp_only_layers, decoder_sparse_step):
    """which decoder layers hold a sparse MLP block, as Qwen3MoeDecoderLayer.__init__ decides it"""
    only = set(int(i) for i in (mlp_only_layers or ()))
    step = int(decoder_sparse_step or 1)
    return [i not in only and n_experts > 0 and (i + 1) % step == 0 for i in range(n_layers)]


def check_shape(hidden, moe_inter, n_experts, top_k):
    """the shapes the expert kernels serve; anything else raises at load"""
    if hidden % 256 != 0 or moe_inter < 256 or moe_inter % 256 != 0:
        raise SamdError(f"mixture-of-experts layers need hidden_size % 256 == 0 and moe_intermediate_size % 256 == 0 (got {hidden}, {moe_inter})")
    if not 1 <= n_experts <= MAX_EXPERTS:
        raise SamdError(f"mixture-of-experts layers serve 1..{MAX_EXPERTS} experts (num_experts = {n_experts})")
    if not 1 <= top_k <= min(MAX_TOPK, n_experts):
        raise SamdError(f"mixture-of-experts layers serve 1..{MAX_TOPK} experts per token, at most num_experts (num_experts_per_tok = {top_k})")


def reject_unsupported(weight_format=None, native_gemm=True, draft_head=False):
    """what a runner with sparse layers does not offer; raises before any device work"""
    if weight_format in ("fp8", "mxfp4"):
        raise SamdError(f"mixture-of-experts models are not available with weight_format '{weight_format}': quantised experts are not supported")
    if not native_gemm:
        raise SamdError("mixture-of-experts layers exist only in the streaming kernels' packed form: native_gemm=False is not available")
    if draft_head:
        raise SamdError("mixture-of-experts layers are not supported on an EAGLE draft head")


def pack_experts(gate_up, down):
    """(packed gate|up, packed down) of HF's fused expert tensors [E, 2 I, H] / [E, H, I], already on the GPU in the model dtype"""
    E, N2, H = gate_up.shape
    if tuple(down.shape) != (E, H, N2 // 2):
        raise SamdError(f"expert tensors of shapes {tuple(gate_up.shape)} and {tuple(down.shape)} do not belong together")
    gate_up, down = gate_up.contiguous(), down.contiguous()
    pgu, pd = torch.empty_like(gate_up), torch.empty_like(down)
    check(lib().samd_moe_pack_experts(_ptr(gate_up), _ptr(pgu), E, N2, H, 1, current_stream()))
    check(lib().samd_moe_pack_experts(_ptr(down), _ptr(pd), E, H, N2 // 2, 0, current_stream()))
    return pgu, pd


class MoeBuffers:
    """device buffers of the three launches for one row bucket: topk_idx / topk_w [RP, k], act [RP * k, I], the workspace (routing lists +
    down products) and out [RP, hidden]"""

    def __init__(self, rows_pad, hidden, moe_inter, n_experts, top_k, dtype, dt_code, device):
        self.rows_pad, self.hidden, self.moe_inter, self.n_experts, self.top_k, self.dt = rows_pad, hidden, moe_inter, n_experts, top_k, dt_code
        self.topk_idx = torch.full((rows_pad, top_k), -1, dtype=torch.int32, device=device)
        self.topk_w = torch.zeros((rows_pad, top_k), dtype=dtype, device=device)
        self.act = torch.zeros((rows_pad * top_k, moe_inter), dtype=dtype, device=device)
        self.ws = torch.zeros(lib().samd_moe_workspace(rows_pad, hidden, n_experts, top_k, dt_code), dtype=torch.uint8, device=device)
        self.out = torch.zeros((rows_pad, hidden), dtype=dtype, device=device)

    def route(self, h, router, d_n, norm_topk):
        check(lib().samd_moe_route(_ptr(h), _ptr(router), _ptr(d_n), self.rows_pad, self.hidden, self.n_experts, self.top_k, int(bool(norm_topk)),
                                   _ptr(self.topk_idx), _ptr(self.topk_w), _ptr(self.ws), self.dt, current_stream()))

    def lists(self, d_n):
        """the routing lists from self.topk_idx as it stands (routing decided elsewhere)"""
        check(lib().samd_moe_lists(_ptr(self.topk_idx), _ptr(d_n), self.rows_pad, self.n_experts, self.top_k, _ptr(self.ws), current_stream()))

    def experts(self, h, wgu_packed, wdown_packed, d_n):
        L, st = lib(), current_stream()
        check(L.samd_moe_gate_up_silu(_ptr(h), _ptr(wgu_packed), _ptr(self.ws), self.rows_pad, self.hidden, self.moe_inter, self.n_experts, self.top_k,
                                      _ptr(self.act), self.dt, st))
        check(L.samd_moe_down_combine(_ptr(self.act), _ptr(wdown_packed), _ptr(self.topk_idx), _ptr(self.topk_w), _ptr(d_n), _ptr(self.ws),
                                      self.rows_pad, self.hidden, self.moe_inter, self.n_experts, self.top_k, _ptr(self.out), self.dt, st))
        return self.out

    def routing_state(self):
        """(n_active, active experts, counts, lists) read back from the workspace: for tests and profiling"""
        active, count, lst, stride, words = (lib().samd_moe_workspace_layout(f) for f in range(5))
        w = self.ws[:4 * words].view(torch.int32).cpu()
        n = int(w[0])
        return (n, w[active:active + n].tolist(), w[count:count + n].tolist(),
                [w[lst + stride * a:lst + stride * a + int(w[count + a])].tolist() for a in range(n)])
