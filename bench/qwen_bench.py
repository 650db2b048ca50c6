"""qkv_prep (Qwen2 qkv bias / Qwen3 per-head q, k RMSNorm) kernel times against the byte floor.

For the two full-size presets at T = 256 and T = 32768: the in-place kernel's time (HIP events, median and
minimum of interleaved rounds) next to the repository's rms_norm over the same byte count in the same
process -- rows = T, hidden = the touched elements of a token, so both read and write 2 bytes per touched
element.  One JSON line per (model, T); ``ratio`` = qkv_prep / rms_norm medians.

    python bench/qwen_bench.py [--tokens 256 32768] [--rounds 30] [--inner 10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from distributed_llms_amd import _ext, ops
from distributed_llms_amd.config import get_model_config
from distributed_llms_amd.models import weights as W
from distributed_llms_amd.ops import reference as ref


def timed(fn, inner):
    """Microseconds per call over ``inner`` back-to-back launches between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["qwen2.5-7b", "qwen3-8b"])
    ap.add_argument("--tokens", nargs="+", type=int, default=[256, 32768])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qwen_bench needs a GPU")
    dev, bf = "cuda", torch.bfloat16
    for name in a.models:
        cfg = get_model_config(name)
        hq, hkv, d = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim
        blk = {k: W.synth_tensor(0, 0, k, s, bf, dev) for k, s in W.block_shapes(cfg).items()
               if k in ("bqkv", "q_norm", "k_norm")}
        args = (blk.get("bqkv"), blk.get("q_norm"), blk.get("k_norm"), hq, hkv, d, cfg.norm_eps)
        slots = hq + 2 * hkv if cfg.attn_bias else hq + hkv
        for t in a.tokens:
            g = torch.Generator(device=dev).manual_seed(t)
            qkv = torch.randn(t, cfg.qkv_size, generator=g, device=dev).to(bf)
            # same results as the contract on the first and last rows, at the size that is timed
            rows = torch.cat([torch.arange(min(t, 64)), torch.arange(max(0, t - 64), t)]).unique()
            want = ref.qkv_prep(qkv[rows.to(dev)].cpu().clone(), *[None if x is None else x.cpu() for x in args[:3]],
                                *args[3:])
            got = ops.qkv_prep_(qkv.clone(), *args)[rows.to(dev)].cpu()
            err = ((got.double() - want.double()).abs() / want.double().abs().clamp(min=1e-30)).max().item()
            assert err <= 2.0 ** -7, f"{name} T={t}: relative error {err} against the reference"
            x = torch.randn(t, slots * d, generator=g, device=dev).to(bf)      # the comparator's rows
            w = torch.ones(slots * d, dtype=bf, device=dev)
            y = torch.empty_like(x)
            k = _ext.kernels()
            s = torch.cuda.current_stream().cuda_stream
            ptr = lambda v: 0 if v is None else v.data_ptr()                      # noqa: E731
            # both through the raw bindings: at T = 256 the Python wrapper's checks cost more than the kernel
            prep = lambda: k.qkv_prep(qkv.data_ptr(), ptr(args[0]), ptr(args[1]), ptr(args[2]), t, hq, hkv, d,  # noqa: E731
                                      cfg.norm_eps, s)
            norm = lambda: k.rms_norm(y.data_ptr(), x.data_ptr(), 0, w.data_ptr(), t, slots * d, 1e-6, s)  # noqa: E731
            for f in (prep, norm):
                timed(f, 3)
            tp, tn = [], []
            for _ in range(a.rounds):                                             # interleaved rounds
                tp.append(timed(prep, a.inner))
                tn.append(timed(norm, a.inner))
            moved = 2 * t * slots * d * 2
            mp, mn = statistics.median(tp), statistics.median(tn)
            print(json.dumps({
                "model": name, "tokens": t, "touched_heads": slots, "bytes_moved": moved,
                "qkv_prep_us_median": round(mp, 2), "qkv_prep_us_min": round(min(tp), 2),
                "rms_norm_us_median": round(mn, 2), "rms_norm_us_min": round(min(tn), 2),
                "qkv_prep_TBps": round(moved / mp / 1e6, 3), "rms_norm_TBps": round(moved / mn / 1e6, 3),
                "ratio": round(mp / mn, 3), "max_rel_err_vs_reference": err}), flush=True)


if __name__ == "__main__":
    main()
