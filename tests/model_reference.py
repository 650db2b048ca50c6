"""A cacheless high-precision forward of the Llama-family models (Llama, Mixtral, Qwen2 qkv bias, Qwen3
per-head q/k RMSNorm), for tests that compare the engine with something that is not the engine.

It recomputes a whole token sequence causally in one pass and returns the logits (and, for MoE, the routing
margin) at EVERY position: one forward of a finished sequence's ``prompt + output`` is the reference of
its prefill row and of each of its decode steps.  It runs on the CPU in float32 or float64, has no KV cache,
no block tables, no slots and no batching metadata, and shares nothing with the engine but the weights,
the token ids and ``ops.reference.apply_rope``.  The RoPE table (Llama-3 frequency rescaling included) is
computed here, from the published formula.

``rnd=_bf`` rounds every op's output to bf16: the bf16-storage / fp32-compute forward, i.e. what an exact
bf16 kernel stack would produce.  Its distance from the unrounded forward is the error floor of bf16
activations, which the GPU tests measure themselves against.

GPT-2 is not covered."""
import math

import torch
import torch.nn.functional as F

from distributed_llms_amd.ops import reference as ref


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def rope_table(cfg, dtype=torch.float32) -> torch.Tensor:
    """[max_position, head_dim]: cos in the first half, sin in the second (the layout apply_rope reads).
    ``rope_type: llama3``: wavelengths above original / low_freq_factor are stretched by ``factor``, those
    below original / high_freq_factor kept, the band between blended linearly in original / wavelength."""
    d = cfg.head_dim
    inv = [cfg.rope_theta ** (-2.0 * i / d) for i in range(d // 2)]
    sc = cfg.rope_scaling
    if sc and sc.get("rope_type", sc.get("type")) == "llama3":
        old = sc["original_max_position_embeddings"]
        lo, hi, factor = sc["low_freq_factor"], sc["high_freq_factor"], sc["factor"]
        out = []
        for f in inv:
            wl = 2 * math.pi / f
            if wl < old / hi:
                out.append(f)
            elif wl > old / lo:
                out.append(f / factor)
            else:
                s = (old / wl - lo) / (hi - lo)
                out.append((1 - s) * f / factor + s * f)
        inv = out
    fr = torch.outer(torch.arange(cfg.max_position, dtype=torch.float64), torch.tensor(inv, dtype=torch.float64))
    return torch.cat([fr.cos(), fr.sin()], dim=-1).to(dtype)


def weights_from_hf(cfg, sd, dtype=torch.float32, rnd=None):
    """The fused tensors ``forward_all`` reads, from an HF-named state dict (the one the engine loads).
    ``rnd`` (``_bf``): round the weights first, as a bf16 engine's load does."""
    r = rnd or (lambda t: t)
    g = lambda n: r(sd[n].detach().to("cpu", dtype))
    layers = []
    for l in range(cfg.num_layers):
        p = f"model.layers.{l}."
        a = p + "self_attn."
        lw = {"attn_norm": g(p + "input_layernorm.weight"),
              "wqkv": torch.cat([g(a + "q_proj.weight"), g(a + "k_proj.weight"), g(a + "v_proj.weight")], 0),
              "wo": g(a + "o_proj.weight"), "mlp_norm": g(p + "post_attention_layernorm.weight")}
        if cfg.attn_bias:
            lw["bqkv"] = torch.cat([g(a + "q_proj.bias"), g(a + "k_proj.bias"), g(a + "v_proj.bias")], 0)
        if cfg.qk_norm:
            lw["q_norm"], lw["k_norm"] = g(a + "q_norm.weight"), g(a + "k_norm.weight")
            if cfg.attn_bias:
                lw["bo"] = g(a + "o_proj.bias")
        if cfg.is_moe:
            e = p + "block_sparse_moe."
            lw["router"] = g(e + "gate.weight")
            lw["experts_gate_up"] = torch.stack([torch.cat([g(e + f"experts.{i}.w1.weight"),
                                                            g(e + f"experts.{i}.w3.weight")], 0)
                                                 for i in range(cfg.num_experts)])
            lw["experts_down"] = torch.stack([g(e + f"experts.{i}.w2.weight") for i in range(cfg.num_experts)])
        else:
            lw["w_gate_up"] = torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0)
            lw["w_down"] = g(p + "mlp.down_proj.weight")
        layers.append(lw)
    embed = g("model.embed_tokens.weight")
    return {"layers": layers, "embed": embed, "final_norm": g("model.norm.weight"),
            "lm_head": embed if cfg.tie_embeddings else g("lm_head.weight")}


def forward_all(cfg, w, toks: torch.Tensor, cos_sin: torch.Tensor, rnd=None, chunk: int = 32, last_only=False):
    """Causal forward of ``toks`` [B, T] in the dtype of ``w`` -> (logits [B, T, V], routing margin [B, T]:
    the smallest gap, over the layers, between the router probabilities of the k-th and (k+1)-th expert; inf
    for dense models).  ``last_only``: the LM head (and the margin) on the last position only, [B, V] / [B].
    ``rnd``: applied to every op's output (see the module docstring)."""
    r = rnd or (lambda t: t)
    hq, hkv, d, eps = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.norm_eps
    scale = 1.0 / math.sqrt(d)
    out, margin = [], []
    for b0 in range(0, toks.shape[0], chunk):
        t = toks[b0:b0 + chunk]
        b, n = t.shape
        pos = torch.arange(n, device=t.device).repeat(b)
        x = w["embed"][t]
        gap = torch.full((b, n), float("inf"), device=t.device, dtype=x.dtype)
        for lw in w["layers"]:
            h = r(_rms(x, lw["attn_norm"], eps))
            qkv = r(h @ lw["wqkv"].t())
            if "bqkv" in lw:
                qkv = r(qkv + lw["bqkv"])
            qkv = qkv.view(b * n, hq + 2 * hkv, d)
            q, k = qkv[:, :hq], qkv[:, hq:hq + hkv]
            if "q_norm" in lw:
                q, k = r(_rms(q, lw["q_norm"], eps)), r(_rms(k, lw["k_norm"], eps))
            q = r(ref.apply_rope(q, pos, cos_sin)).view(b, n, hq, d).transpose(1, 2)
            k = r(ref.apply_rope(k, pos, cos_sin)).view(b, n, hkv, d).transpose(1, 2)
            v = qkv[:, hq + hkv:].reshape(b, n, hkv, d).transpose(1, 2)
            k = k.repeat_interleave(hq // hkv, dim=1)
            v = v.repeat_interleave(hq // hkv, dim=1)
            a = r(F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=scale))
            o = a.transpose(1, 2).reshape(b, n, hq * d) @ lw["wo"].t()
            if "bo" in lw:
                o = o + lw["bo"]
            x = r(x + o)
            h = r(_rms(x, lw["mlp_norm"], eps)).view(b * n, -1)
            if cfg.is_moe:
                probs = torch.softmax(h @ lw["router"].t(), dim=-1)
                top = probs.view(b, n, -1).topk(cfg.experts_per_token + 1, dim=-1).values
                gap = torch.minimum(gap, top[..., -2] - top[..., -1])
                tw, ids = torch.topk(probs, cfg.experts_per_token, dim=-1)
                tw = tw / tw.sum(-1, keepdim=True)
                y = torch.zeros_like(h)
                for e in range(cfg.num_experts):
                    tok, slot = (ids == e).nonzero(as_tuple=True)
                    if tok.numel():
                        gu = h[tok] @ lw["experts_gate_up"][e].t()
                        i = gu.shape[-1] // 2
                        ye = (F.silu(gu[:, :i]) * gu[:, i:]) @ lw["experts_down"][e].t()
                        y.index_add_(0, tok, ye * tw[tok, slot].unsqueeze(1))
            else:
                gu = h @ lw["w_gate_up"].t()
                i = gu.shape[-1] // 2
                y = r(F.silu(gu[:, :i]) * gu[:, i:]) @ lw["w_down"].t()
            x = r(x + y.view(b, n, -1))
        if last_only:
            x, gap = x[:, -1], gap[:, -1]
        out.append(r(_rms(x, w["final_norm"], eps)) @ w["lm_head"].t())
        margin.append(gap)
    return torch.cat(out), torch.cat(margin)


def _ref_logits(stage, w32, toks: torch.Tensor, chunk: int = 32, rnd=None):
    """fp32 forward of ``toks`` [B, T] (all positions, causal) with a stage's (fused, unpadded) weights
    ``w32`` and RoPE table, as tests/test_production_shapes_gpu.py has always run it; last-position logits
    [B, V] and routing margins [B]."""
    return forward_all(stage.cfg, w32, toks, stage.cos_sin, rnd=rnd, chunk=chunk, last_only=True)
