"""LoRA adapters: sources, validation and the per-stage tensors the kernels read.

A source (``EngineConfig.lora_modules``: name -> source) is a local PEFT directory
(``adapter_config.json`` + ``adapter_model.safetensors`` / ``.bin``, keys
``base_model.model.<module path>.lora_A.weight`` / ``lora_B.weight``) or
``synthetic:<rank>:<seed>[:<module>+<module>...]`` (seeded N(0, s) factors, lora_alpha = 2 r; every
stage and device draws the same values).  Everything an adapter or an engine configuration cannot
run is refused here, when the adapter is loaded or the engine is built, never at step time.

A stage holds the tensors of its own layers only, per projection as [slots, ...] (ops/lora.py
LoraWeight), slot = the adapter name's index in sorted order; the set is fixed for the engine's life.
"""
from __future__ import annotations

import json
import os
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from ..config import EngineConfig, ModelConfig
from ..ops import reference as ref
from ..ops.lora import LoraWeight
from . import weights as W

ATTN_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_TARGETS = ("gate_proj", "up_proj", "down_proj")
TARGETS = ATTN_TARGETS + MLP_TARGETS
_HF_PATH = {m: "self_attn." + m for m in ATTN_TARGETS}
_HF_PATH.update({m: "mlp." + m for m in MLP_TARGETS})


def projections(cfg: ModelConfig) -> Dict[str, Tuple[Tuple[str, ...], Tuple[int, ...], int]]:
    """Runtime projection -> (its LoRA modules in column order, their widths, input width K)."""
    h = cfg.hidden_size
    p = {"wqkv": (("q_proj", "k_proj", "v_proj"), (cfg.q_size, cfg.kv_size, cfg.kv_size), h),
         "wo": (("o_proj",), (h,), cfg.q_size)}
    if not cfg.is_moe:
        i = cfg.intermediate_size
        p["w_gate_up"] = (("gate_proj", "up_proj"), (i, i), h)
        p["w_down"] = (("down_proj",), (h,), i)
    return p


def supported_targets(cfg: ModelConfig) -> Tuple[str, ...]:
    return ATTN_TARGETS if cfg.is_moe else TARGETS


@dataclass
class Adapter:
    """One adapter on the host: float32 factors per (layer, module), a [r, K] and b [N, r]."""
    name: str
    rank: int
    scale: float
    targets: Tuple[str, ...]
    tensors: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=dict)
    make: Optional[Callable[[int, str], Tuple[torch.Tensor, torch.Tensor]]] = field(default=None, repr=False)

    def factors(self, layer: int, module: str):
        """(a, b) of ``module`` in ``layer``, or None where the adapter has none."""
        if module not in self.targets:
            return None
        if self.make is not None:
            return self.make(layer, module)
        return self.tensors.get((layer, module))


def _check_targets(name: str, targets, cfg: ModelConfig) -> Tuple[str, ...]:
    ok = supported_targets(cfg)
    out = []
    for t in targets:
        leaf = str(t).split(".")[-1]
        if leaf not in ok:
            kind = "on a Mixtral model only the attention projections can carry LoRA" if leaf in MLP_TARGETS \
                else "expert, embedding and LM-head targets are not supported"
            raise ValueError(f"adapter {name!r}: target module {t!r} is not supported ({kind}); supported: {list(ok)}")
        out.append(leaf)
    if not out:
        raise ValueError(f"adapter {name!r}: no target modules")
    return tuple(sorted(set(out), key=TARGETS.index))


def _check_rank(name: str, rank, max_rank: int) -> int:
    if isinstance(rank, bool) or not isinstance(rank, int) or rank < 1:
        raise ValueError(f"adapter {name!r}: rank must be a positive integer, got {rank!r}")
    if rank > max_rank:
        raise ValueError(f"adapter {name!r}: rank {rank} exceeds max_lora_rank {max_rank}")
    return rank


def _module_shape(cfg: ModelConfig, module: str) -> Tuple[int, int]:
    """(N, K) of a LoRA module's base weight."""
    for mods, widths, k in projections(cfg).values():
        if module in mods:
            return widths[mods.index(module)], k
    raise KeyError(module)


def synthetic_adapter(name: str, spec: str, cfg: ModelConfig, max_rank: int) -> Adapter:
    parts = spec.split(":")
    if len(parts) not in (3, 4) or parts[0] != "synthetic" or not parts[1].isdigit() or not parts[2].isdigit():
        raise ValueError(f"adapter {name!r}: expected synthetic:<rank>:<seed>[:<module>+<module>...], got {spec!r}")
    rank = _check_rank(name, int(parts[1]), max_rank)
    seed = int(parts[2])
    targets = _check_targets(name, parts[3].split("+") if len(parts) == 4 else supported_targets(cfg), cfg)

    def make(layer: int, module: str):
        n, k = _module_shape(cfg, module)
        g = torch.Generator(device="cpu")
        g.manual_seed(W.tensor_seed(seed, layer, "lora." + module))
        a = torch.randn(rank, k, generator=g) * 0.05
        b = torch.randn(n, rank, generator=g) * (0.1 / rank ** 0.5)
        return a, b

    return Adapter(name, rank, ref.lora_scale(2 * rank, rank), targets, make=make)


_KEY_RE = re.compile(r"^base_model\.model\.(?:model\.)?layers\.(\d+)\.(.+)\.lora_([AB])\.weight$")


def peft_adapter(name: str, path: str, cfg: ModelConfig, max_rank: int) -> Adapter:
    """Load a PEFT directory.  Refused: targets other than the seven dense projections,
    ``modules_to_save``, ``bias`` other than "none", DoRA, per-module rank / alpha patterns, a rank
    above ``max_rank``, and any tensor that is not a ``lora_A`` / ``lora_B`` weight of a target."""
    cpath = os.path.join(path, "adapter_config.json")
    if not os.path.isfile(cpath):
        raise ValueError(f"adapter {name!r}: no adapter_config.json in {path!r}")
    with open(cpath) as f:
        c = json.load(f)
    if c.get("peft_type", "LORA") != "LORA":
        raise ValueError(f"adapter {name!r}: peft_type {c.get('peft_type')!r} is not LORA")
    if c.get("use_dora"):
        raise ValueError(f"adapter {name!r}: DoRA (use_dora) is not supported")
    if c.get("bias", "none") != "none":
        raise ValueError(f"adapter {name!r}: bias={c.get('bias')!r} is not supported (only \"none\")")
    if c.get("modules_to_save"):
        raise ValueError(f"adapter {name!r}: modules_to_save {c['modules_to_save']!r} is not supported")
    if c.get("rank_pattern") or c.get("alpha_pattern"):
        raise ValueError(f"adapter {name!r}: rank_pattern / alpha_pattern are not supported")
    rank = _check_rank(name, c.get("r"), max_rank)
    tm = c.get("target_modules")
    if isinstance(tm, str) or not tm:
        raise ValueError(f"adapter {name!r}: target_modules must be a list of module names, got {tm!r}")
    targets = _check_targets(name, tm, cfg)
    scale = ref.lora_scale(c.get("lora_alpha", rank), rank, bool(c.get("use_rslora")))
    st, bn = os.path.join(path, "adapter_model.safetensors"), os.path.join(path, "adapter_model.bin")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.isfile(bn):
        sd = torch.load(bn, map_location="cpu", weights_only=True)
    else:
        raise ValueError(f"adapter {name!r}: no adapter_model.safetensors / adapter_model.bin in {path!r}")
    halves: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
    for key, t in sd.items():
        m = _KEY_RE.match(key)
        leaf = m.group(2).split(".")[-1] if m else None
        if m is None or leaf not in targets or m.group(2) != _HF_PATH[leaf]:
            raise ValueError(f"adapter {name!r}: tensor {key!r} is not a lora_A / lora_B weight of a target module")
        layer = int(m.group(1))
        if layer >= cfg.num_layers:
            raise ValueError(f"adapter {name!r}: tensor {key!r} names layer {layer} of a {cfg.num_layers}-layer model")
        halves.setdefault((layer, leaf), {})[m.group(3)] = t.to(torch.float32)
    tensors = {}
    for (layer, leaf), ab in halves.items():
        n, k = _module_shape(cfg, leaf)
        if set(ab) != {"A", "B"} or tuple(ab["A"].shape) != (rank, k) or tuple(ab["B"].shape) != (n, rank):
            raise ValueError(f"adapter {name!r}: layer {layer} {leaf}: expected lora_A [{rank}, {k}] and lora_B "
                             f"[{n}, {rank}]")
        tensors[(layer, leaf)] = (ab["A"].contiguous(), ab["B"].contiguous())
    return Adapter(name, rank, scale, targets, tensors=tensors)


def load_adapter(name: str, source: str, cfg: ModelConfig, max_rank: int) -> Adapter:
    if not isinstance(name, str) or not name:
        raise ValueError(f"adapter names must be non-empty strings, got {name!r}")
    if str(source).startswith("synthetic:"):
        return synthetic_adapter(name, source, cfg, max_rank)
    return peft_adapter(name, str(source), cfg, max_rank)


def check_engine(ecfg: EngineConfig, cfg: ModelConfig) -> None:
    """What an engine with ``lora_modules`` cannot be (tp > 1: EngineConfig.check_tensor_parallel)."""
    if not ecfg.lora_modules:
        return
    if not 1 <= ecfg.max_lora_rank <= ref.LORA_MAX_RANK:
        raise ValueError(f"max_lora_rank must be in [1, {ref.LORA_MAX_RANK}], got {ecfg.max_lora_rank}")
    if cfg.arch == "gpt2":
        raise ValueError("LoRA adapters are not supported on GPT-2 models")
    if ecfg.quant != "none":
        raise ValueError(f"LoRA adapters are not supported with quant={ecfg.quant!r}")
    if os.environ.get("DLLM_PP_FINE", "0") == "1":
        raise ValueError("LoRA adapters are not supported with sub-layer pipeline cuts (DLLM_PP_FINE=1)")


def adapter_slots(ecfg: EngineConfig) -> Dict[str, int]:
    """Adapter name -> slot (its index in sorted order), the same on every stage."""
    return {n: i for i, n in enumerate(sorted(ecfg.lora_modules))}


@dataclass
class StageLora:
    names: List[str]
    scale: torch.Tensor                            # [slots] float32
    layers: List[Dict[str, LoraWeight]]            # per stage layer: runtime projection -> adapters

    def nbytes(self) -> int:
        return sum(w.nbytes() for d in self.layers for w in d.values())


def build_stage_lora(stage, ecfg: EngineConfig) -> Optional[StageLora]:
    """Load every configured adapter's tensors for ``stage``'s own layers (None: none configured)."""
    cfg = stage.cfg
    if not ecfg.lora_modules:
        return None
    check_engine(ecfg, cfg)
    if stage.tp.enabled:
        ecfg.check_tensor_parallel(stage.tp.size)
    if stage.atom_start % 5 not in (0, 3) or stage.atom_end % 5 not in (0, 3):
        raise ValueError("LoRA adapters are not supported with sub-layer pipeline cuts")
    names = sorted(ecfg.lora_modules)
    adapters = [load_adapter(n, ecfg.lora_modules[n], cfg, ecfg.max_lora_rank) for n in names]
    rp = ref.lora_rank_pad(max(a.rank for a in adapters))
    dev, dt = stage.device, stage.dtype
    scale = torch.tensor([a.scale for a in adapters], dtype=torch.float32, device=dev)
    layers = []
    for l in range(stage.layer_start, stage.layer_end):
        d = {}
        for proj, (mods, widths, k) in projections(cfg).items():
            if not stage._keep(l, proj) or not any(m in a.targets for a in adapters for m in mods):
                continue
            n = sum(widths)
            if k % 32 or n % 16 or any(sum(widths[:i]) % 64 for i in range(len(widths))):
                raise ValueError(f"LoRA on {proj}: input width {k} must be a multiple of 32, the output width {n} "
                                 f"of 16 and the first column of every module ({widths}) of 64")
            a_all =torch.zeros(len(adapters), len(mods) * rp, k, dtype=torch.float32)
            b_all = torch.zeros(len(adapters), n, rp, dtype=torch.float32)
            starts = [sum(widths[:i]) for i in range(len(mods))]
            for s, ad in enumerate(adapters):
                for i, m in enumerate(mods):
                    ab = ad.factors(l, m)
                    if ab is not None:          # a module the adapter does not target stays a zero slice
                        a_all[s, i * rp:i * rp + ad.rank] = ab[0]
                        b_all[s, starts[i]:starts[i] + widths[i], :ad.rank] = ab[1]
            d[proj] = LoraWeight(a_all.to(device=dev, dtype=dt).contiguous(),
                                 b_all.to(device=dev, dtype=dt).contiguous(), scale, tuple(starts))
        layers.append(d)
    return StageLora(names, scale, layers)
