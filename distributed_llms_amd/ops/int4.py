"""Int4 weight-only (W4A16) dense projections -- the 4-bit half of the quantization the reference only
documents (bitsandbytes int8/int4 sketched, never run); :mod:`.quant` is the 8-bit half.

Round-to-nearest at load: a weight [N, K] (N % 128 == 0, K % 128 == 0) becomes 4-bit codes with one bf16 scale per
128 consecutive k of a row (contract: ops/reference.py, "int4 weights").  Activations stay bf16.  0.5 byte per
weight plus 2 bytes per 128: Llama-3-70B's 141 GB of bf16 projections become 36 GB, and a decode projection at
small batch -- a pure weight stream -- reads a quarter of the bytes.

* :func:`pack`: the codes in MFMA-fragment-major order (csrc/kernels/gemm_w4.hip: one 1 KiB block per 16-row tile
  and group, a lane's 16 bytes = one row's group); scales as [N / 16, K / 128, 16];
* ``gemm_w4a16`` for M < :data:`INT4_DEQUANT_MIN_M`: weights straight from global memory into registers, x through
  an LDS ring, split-K into the per-stream GEMM workspace with an ordered reduce -- the same bits on every launch;
* from that M: ``dequant_w4`` into a per-stream scratch tensor and the bf16 route of :func:`..gemm.linear`
  (prefill keeps gemm_pf); the weights are rounded to bf16 once there.

Imported checkpoints (:func:`from_checkpoint`: AWQ "gemm", GPTQ v1 / v2; formats in ops/reference.py): per-group
zero points 0..15 and f16 (or bf16) scales, w = (code - zero) * scale.  Such a weight keeps one int32 per (row,
group) -- the scale's f32 bits with the zero in bits 0..3 (csrc/kernels/gemm_w4.hip, "Zero-point variant") -- and
runs the zero-point instantiations of the same kernels; ``w4_repack`` (csrc/kernels/w4_repack.hip) turns the
checkpoint's K-major words into the fragment order on the device, each projection into its rows of the fused weight.

Opt-in (``EngineConfig.quant = "int4"``): embeddings, norms, the LM head and the KV cache stay bf16.  The result
is always dense (``defer`` is accepted and ignored), SwiGLU is ``ops.silu_mul`` on it.  CPU tensors take the
reference (same codes and scales, f32 math)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _ext
from . import gemm
from . import reference as ref
from .quant import QUANT_KEYS

# ops.quantize_layers refuses a stage none of whose projections this format takes
NOTHING_CONVERTED = 'quant="int4" converted no weight of this stage (N and K multiples of 128)'
GROUP = ref.W4_GROUP

# From this M the op dequantizes and runs the bf16 GEMMs.  bench/int4_bench.py (profiles/int4.md): the smallest
# measured M at which the dequant route wins on most of the Llama-3-8B shapes -- at 512 on three of four (at 384 and
# at 192 on two, at 256 on one; below 128 the kernel wins everywhere)
INT4_DEQUANT_MIN_M = 512


def _tiles(n: int, k: int):
    if n % 128 or k % GROUP or n < 128 or k < GROUP:
        raise ValueError(f"int4 weight: N % 128 == 0 and K % {GROUP} == 0, got [{n}, {k}]")
    return n // 16, k // GROUP


def pack(u: torch.Tensor) -> torch.Tensor:
    """Codes ``u`` [N, K] uint8 (0..15) -> uint8 [N / 16, K / 128, 1024] in the kernel's order: block (t, g), lane
    r + 16 q (row r of the tile), word j, code e of k = 128 g + 32 j + 8 q + e at bit 4 (e / 2) + 16 (e % 2)."""
    t, g = _tiles(*u.shape)
    v = u.view(t, 16, g, 4, 4, 2, 2, 2)                  # t, r, g, j, q, p1, p0, h: e = 4 p1 + 2 p0 + h
    b = v[..., 0, :] | (v[..., 1, :] << 4)               # byte 2 h + p1 of the word: bits 4 p0 of it
    return b.permute(0, 2, 4, 1, 3, 6, 5).contiguous().view(t, g, 1024)      # t, g, q, r, j, h, p1


def unpack(packed: torch.Tensor) -> torch.Tensor:
    """The inverse of :func:`pack`: codes [N, K] uint8."""
    t, g, _ = packed.shape
    b = packed.view(t, g, 4, 16, 4, 2, 2)                # t, g, q, r, j, h, p1
    v = torch.stack([b & 15, b >> 4], dim=-1)            # ..., p0
    return v.permute(0, 3, 1, 4, 2, 6, 7, 5).contiguous().view(16 * t, GROUP * g)   # t, r, g, j, q, p1, p0, h


class Int4Weight:
    """An [N, K] weight as fragment-packed 4-bit codes ``packed`` (uint8 [N / 16, K / 128, 1024]) and, per (row,
    group) in [N / 16, K / 128, 16] order, either

    * symmetric (round-to-nearest at load): bf16 ``scale``, w ~= (code - 8) * scale; or
    * with zero points (imported checkpoints): ``sz`` int32, the f32 bits of an f16 / bf16 scale | the zero 0..15,
      w = (code - zero) * scale.  ``scale`` is then None; :meth:`scales` / :meth:`zeros` give both back.

    ``Int4Weight(packed, scale)`` with a bf16 scale is the symmetric weight; with ``zeros`` (uint8, the scale's shape)
    or an f16 scale (zeros absent: 8) the two are fused into ``sz``; an int32 ``scale`` is taken as ``sz`` itself, of
    ``scale_dtype`` scales."""

    __slots__ = ("packed", "scale", "sz", "scale_dtype")
    takes_fp8_act = False        # W4A16: activations stay bf16

    def __init__(self, packed: torch.Tensor, scale: torch.Tensor, zeros: Optional[torch.Tensor] = None,
                 scale_dtype: torch.dtype = torch.float16):
        if packed.dtype != torch.uint8 or packed.dim() != 3 or packed.shape[2] != 1024 or packed.shape[0] % 8 \
                or scale.dtype not in (torch.bfloat16, torch.float16, torch.int32) \
                or scale.shape != (*packed.shape[:2], 16) or scale.device != packed.device:
            raise ValueError("Int4Weight: packed uint8 [N / 16, K / 128, 1024] (N % 128 == 0) and scale bf16 / f16 "
                             "(or int32 scale | zero) [N / 16, K / 128, 16] on one device")
        if zeros is not None and (scale.dtype == torch.int32 or zeros.dtype != torch.uint8
                                  or zeros.shape != scale.shape or zeros.device != scale.device):
            raise ValueError("Int4Weight: zeros uint8 of the scale's shape and device, next to a bf16 / f16 scale")
        self.packed, self.scale, self.sz, self.scale_dtype = packed.contiguous(), None, None, scale.dtype
        if scale.dtype == torch.int32:
            self.sz, self.scale_dtype = scale.contiguous(), scale_dtype
        elif zeros is None and scale.dtype == torch.bfloat16:
            self.scale = scale.contiguous()
        else:
            z = torch.full_like(scale, 8, dtype=torch.int32) if zeros is None else zeros.to(torch.int32)
            self.sz = (scale.float().contiguous().view(torch.int32) & ~15) | z

    @property
    def shape(self):
        return torch.Size((16 * self.packed.shape[0], GROUP * self.packed.shape[1]))

    @property
    def device(self):
        return self.packed.device

    @property
    def dtype(self):
        return torch.uint8

    def numel(self) -> int:
        return 2 * self.packed.numel()

    def nbytes(self) -> int:
        return self.packed.numel() + (2 * self.scale.numel() if self.sz is None else 4 * self.sz.numel())

    def to(self, device) -> "Int4Weight":
        return Int4Weight(self.packed.to(device), (self.scale if self.sz is None else self.sz).to(device),
                          scale_dtype=self.scale_dtype)

    def _plain(self, t: torch.Tensor) -> torch.Tensor:
        return t.permute(0, 2, 1).reshape(self.shape[0], -1)

    def codes(self) -> torch.Tensor:
        return unpack(self.packed)

    def scales(self) -> torch.Tensor:
        """Scales in plain [N, K / 128] order (bf16, or the imported checkpoint's f16)."""
        if self.sz is None:
            return self._plain(self.scale)
        return self._plain((self.sz & ~15).view(torch.float32).to(self.scale_dtype))

    def zeros(self) -> Optional[torch.Tensor]:
        """Zero points in plain [N, K / 128] order (uint8); None for the symmetric weight (8 everywhere)."""
        return None if self.sz is None else self._plain((self.sz & 15).to(torch.uint8))

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        return ref.dequantize_w4(self.codes(), self.scales(), self.zeros()).to(dtype)

    def linear(self, x, bias=None, defer: bool = False, swiglu: bool = False):
        """What ops.linear / ops.linear_swiglu do with this weight: always dense, SwiGLU as silu_mul on the result."""
        if bias is not None:
            raise ValueError("linear: int4 weights take no bias")
        y = linear_int4(x, self, defer=defer)
        if swiglu:
            from . import silu_mul
            return silu_mul(y)
        return y

    def __repr__(self):
        return f"Int4Weight(shape={tuple(self.shape)}, device={self.device}, zeros={self.sz is not None})"


def from_codes(u: torch.Tensor, s: torch.Tensor, z: Optional[torch.Tensor] = None) -> Int4Weight:
    """Codes [N, K] uint8, scales [N, K / 128] (bf16; f16 or with ``z``: the zero-point weight) and zero points
    [N, K / 128] uint8 -> the packed weight."""
    t, g = _tiles(*u.shape)
    tile = lambda a: a.view(t, 16, g).permute(0, 2, 1).contiguous()
    return Int4Weight(pack(u), tile(s), None if z is None else tile(z))


FORMATS = {"awq": 0, "gptq": 1, "gptq_v2": 2}      # w4_repack's format argument


def from_checkpoint(parts, fmt: str) -> Int4Weight:
    """One weight from the ``(qweight, qzeros, scales)`` of projections stacked along N (q|k|v, gate|up), as an AWQ
    ("awq") or GPTQ ("gptq": zero - 1 stored, "gptq_v2") checkpoint holds them (ops/reference.py).  On the GPU each
    part is repacked by ``w4_repack`` into its rows of the weight; on the CPU by the torch unpackers and :func:`pack`."""
    if fmt not in FORMATS or not parts:
        raise ValueError(f"from_checkpoint: format {fmt!r} {tuple(FORMATS)} and at least one projection")
    dev, sdt, shapes = parts[0][0].device, parts[0][2].dtype, []
    for qw, qz, sc in parts:
        k, n = (qw.shape[0], 8 * qw.shape[1]) if fmt == "awq" else (8 * qw.shape[0], qw.shape[1])
        _tiles(n, k)
        if qw.dtype != torch.int32 or qz.dtype != torch.int32 or sc.dtype != sdt \
                or sdt not in (torch.float16, torch.bfloat16) or qz.shape != (k // GROUP, n // 8) \
                or sc.shape != (k // GROUP, n) or not qw.device == qz.device == sc.device == dev:
            raise ValueError(f"from_checkpoint ({fmt}): qweight int32 {tuple(qw.shape)} needs qzeros int32 "
                             f"[{k // GROUP}, {n // 8}] and scales f16 / bf16 [{k // GROUP}, {n}] on one device, got "
                             f"{qz.dtype} {tuple(qz.shape)}, {sc.dtype} {tuple(sc.shape)}")
        shapes.append((n, k))
    k = shapes[0][1]
    if any(kk != k for _, kk in shapes):
        raise ValueError(f"from_checkpoint: projections of different K {shapes}")
    if dev.type != "cuda":
        u, z, s = (torch.cat(a, 0) for a in zip(*(ref.unpack_w4(fmt, *p) for p in parts)))
        return from_codes(u, s, z)
    total = sum(n for n, _ in shapes)
    packed = torch.empty(total // 16, k // GROUP, 1024, dtype=torch.uint8, device=dev)
    w = Int4Weight(packed, torch.empty(total // 16, k // GROUP, 16, dtype=torch.int32, device=dev), scale_dtype=sdt)
    row0 = 0
    for (n, _), p in zip(shapes, parts):
        repack_into(w, row0, *p, fmt)
        row0 += n
    return w


def repack_into(w: Int4Weight, row0: int, qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                fmt: str) -> None:
    """``w4_repack``: one checkpoint projection into rows ``row0 ..`` of the zero-point weight ``w`` (GPU)."""
    k, n = (qweight.shape[0], 8 * qweight.shape[1]) if fmt == "awq" else (8 * qweight.shape[0], qweight.shape[1])
    if w.sz is None or k != w.shape[1] or scales.dtype != w.scale_dtype or not w.device.type == "cuda" \
            or qzeros.shape != (k // GROUP, n // 8) or scales.shape != (k // GROUP, n):
        raise ValueError(f"repack_into: a [{n}, {k}] {scales.dtype} projection into {w!r} of {w.scale_dtype} scales")
    qweight, qzeros, scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
    _ext.kernels().w4_repack(w.packed.data_ptr(), w.sz.data_ptr(), qweight.data_ptr(), qzeros.data_ptr(),
                             scales.data_ptr(), FORMATS[fmt], int(scales.dtype == torch.bfloat16), n, k, w.shape[0],
                             row0, torch.cuda.current_stream().cuda_stream)


def quantize_weight(w: torch.Tensor) -> Int4Weight:
    """Group-wise round-to-nearest quantization of an [N, K] weight (any float dtype, any device)."""
    _tiles(*w.shape)
    return from_codes(*ref.quantize_w4(w))


def splits(m: int, n: int, k: int, cus: int = 256, comm_cus: Optional[int] = None) -> int:
    """K slices of gemm_w4a16: its grid (N / 128 column tiles x ceil(M / 64) row tiles x slices) reaches about one
    workgroup per CU that no comm kernel may hold (ops/gemm.py); a slice is at least two groups, and the f32
    slabs fit the GEMM workspace."""
    comm = gemm.comm_cus() if comm_cus is None else comm_cus
    tiles = (n // 128) * -(-m // 64)
    return gemm.ws_splits(max(1, min((cus - comm) // tiles, (k // GROUP) // 2)), m, n)


# dequant-route scratch, one per (device, stream) like the GEMM workspace: ModelStage.quantize reserves the size of
# the stage's largest int4 weight, so a captured step sees a fixed pointer; a grown buffer's predecessor stays alive
_scratch = {}
_scratch_numel = {}
_retired = []


def reserve_scratch(device: torch.device, numel: int) -> None:
    """At least ``numel`` bf16 elements of dequant scratch on ``device`` (allocated now for the current stream)."""
    device = torch.device(device)
    if device.type != "cuda":
        return
    i = device.index if device.index is not None else torch.cuda.current_device()
    _scratch_numel[i] = max(_scratch_numel.get(i, 0), int(numel))
    _scratch_for(device, 0)


def _scratch_for(device: torch.device, numel: int) -> torch.Tensor:
    i = device.index if device.index is not None else torch.cuda.current_device()
    key = (i, torch.cuda.current_stream(device).cuda_stream)
    need = max(numel, _scratch_numel.get(i, 0))
    t = _scratch.get(key)
    if t is None or t.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("int4: no dequant scratch for this stream; reserve_scratch() before capturing a graph")
        if t is not None:
            _retired.append(t)
        _scratch_numel[i] = need
        t = _scratch[key] = torch.empty(need, dtype=torch.bfloat16, device=device)
    return t


def dequant(w: Int4Weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``w`` as a plain bf16 [N, K] tensor (``dequant_w4`` on the GPU, bit-identical to ``dequantize(bfloat16)``)."""
    n, k = w.shape
    if not w.device.type == "cuda":
        return w.dequantize(torch.bfloat16)
    if out is None:
        out = torch.empty(n, k, dtype=torch.bfloat16, device=w.device)
    _ext.kernels().dequant_w4(out.data_ptr(), w.packed.data_ptr(), (w.scale if w.sz is None else w.sz).data_ptr(), n, k,
                              int(w.sz is not None), torch.cuda.current_stream().cuda_stream)
    return out


def linear_int4(x: torch.Tensor, w: Int4Weight, defer: bool = False, splits_: int = 0,
                dequant_min_m: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x wd^T with an :class:`Int4Weight` (contract: ops/reference.py linear_w4); always dense.  ``splits_``:
    the kernel's K slices (0: :func:`splits`); ``dequant_min_m``: the cutover (None: INT4_DEQUANT_MIN_M); ``out``:
    where the kernel route writes (bf16, contiguous, x's leading extents x N)."""
    n, k = w.shape
    if x.shape[-1] != k:
        raise ValueError(f"linear_int4: x[..., {x.shape[-1]}] vs w {tuple(w.shape)}")
    if x.device != w.device:
        raise ValueError(f"linear_int4: x on {x.device}, w on {w.device}")
    if not x.is_cuda:
        return ref.linear_w4(x, w.codes(), w.scales(), w.zeros())
    from . import _ck
    _ck(x, "linear_int4.x", torch.bfloat16)
    m = x.numel() // k
    if m < 1:
        raise ValueError("linear_int4: no rows")
    if m >= (INT4_DEQUANT_MIN_M if dequant_min_m is None else dequant_min_m):
        return gemm.linear(x, dequant(w, _scratch_for(x.device, n * k)[:n * k].view(n, k)))
    y = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device) if out is None else out
    _ck(y, "linear_int4.out", torch.bfloat16, (*x.shape[:-1], n), x.device)
    stream = torch.cuda.current_stream().cuda_stream
    ws = gemm._workspace(x.device, stream)
    s = gemm.ws_splits(splits_, m, n) if splits_ else splits(m, n, k, gemm._cus(x.device))
    _ext.kernels().gemm_w4a16(y.data_ptr(), x.data_ptr(), w.packed.data_ptr(),
                              (w.scale if w.sz is None else w.sz).data_ptr(), ws.data_ptr(), ws.numel(), m, n, k, s,
                              int(w.sz is not None), stream)
    return y


def quantize_layers(layers, keys=QUANT_KEYS) -> int:
    """Replace the dense projections of every layer dict whose N and K are multiples of 128 by
    :class:`Int4Weight` (in place) and reserve the dequant scratch for the largest; returns how many were
    converted.  A weight that already is one (an imported checkpoint's) counts and stays as it is, as does
    everything else."""
    count, largest, device = 0, 0, None
    for lw in layers:
        for name in keys:
            t = lw.get(name)
            if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] % 128 == 0 and t.shape[1] % GROUP == 0:
                lw[name] = quantize_weight(t)
                count += 1
                largest, device = max(largest, t.numel()), t.device
            elif isinstance(t, Int4Weight):
                count += 1
                largest, device = max(largest, t.numel()), t.device
    if count and device.type == "cuda":
        reserve_scratch(device, largest)
    return count
