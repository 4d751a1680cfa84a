"""Host emulation of the int8 (W8A8) form of rr_config.fp8 (handle option "q8_format" = 1), for the tests.

* quant_rows_i8: the per-row quantiser of the quantising LayerNorm (layernorm_q8_kernel<true>) and of the weight packer
  (host_quantize_rows_i8): scale = amax / 127 (1 for a zero row), code = rint(x / scale) (nearest even) clamped to +-127.
* smooth_scales: the outlier smoothing folded at rr_finalize_weights (host_smooth_scales): s_j = 2^round(log2(m_j / median m)),
  m_j = max(|gamma_j|, |beta_j|), clamped to [1, 2^10].
* int8_rounding: the oracle's device_rounding(fp8=True) with its e4m3 GEMM (linear_fp8) swapped for the int8 one.  Each 8-bit
  GEMM knows its producing LayerNorm from the weight name; the LayerNorm output is divided by that LayerNorm's smoothing (exact:
  powers of two), quantised per row, and multiplied by the int8 weights, packed from W * s per output channel.  As the device
  does, the cross-encoder's QKV stays 16-bit (run_layer's cross-encoder call leaves 16-bit rows behind every layer).
"""
import contextlib

import numpy as np
import torch

import oracle.rerank_oracle as O

_INV127 = np.float32(1.0) / np.float32(127.0)


def quant_rows_i8(x: torch.Tensor):
    """(codes as float32 integers, per-row scales [.., 1]) of a float32 tensor, the device's arithmetic."""
    x = x.float()
    amax = x.abs().amax(dim=-1, keepdim=True)
    s = torch.where(amax > 0, amax * torch.tensor(_INV127), torch.ones_like(amax))
    inv = torch.ones_like(s) / s
    q = torch.round((x * inv).clamp(-127.0, 127.0))          # torch.round: half to even
    return q, s


def smooth_scales(gamma, beta) -> np.ndarray:
    g = np.abs(np.asarray(gamma, dtype=np.float32))
    b = np.abs(np.asarray(beta, dtype=np.float32))
    m = np.maximum(g, b)
    n = m.size
    med = float(np.partition(m, n // 2)[n // 2]) if n else 0.0
    e = np.zeros(n, dtype=np.int64)
    if med > 0.0:
        pos = m > 0
        e[pos] = np.floor(np.log2(m[pos].astype(np.float64) / med) + 0.5).astype(np.int64)
    return np.ldexp(np.float32(1.0), np.clip(e, 0, 10)).astype(np.float32)


def _producing_ln(name: str) -> str:
    """state_dict prefix of the LayerNorm whose output an 8-bit GEMM reads."""
    if name.endswith(".intermediate.dense"):
        return name[: -len(".intermediate.dense")] + ".attention.output.LayerNorm"
    head, _, rest = name.partition(".attention.self.")
    stack, _, idx = head.rpartition(".")
    assert rest in ("query", "key", "value") and int(idx) >= 1, name
    return f"{stack}.{int(idx) - 1}.output.LayerNorm"


def linear_i8(x, w, name, smooth=True, mm=None):
    if ".attention.self." in name and name.startswith("reranker."):
        return O.linear(x, w, name, mm)          # the device's cross-encoder QKV: 16-bit (see the module docstring)
    ln = _producing_ln(name)
    s = torch.from_numpy(smooth_scales(w[ln + ".weight"], w[ln + ".bias"]) if smooth else
                         np.ones(x.shape[-1], dtype=np.float32))
    W = w[name + ".weight"].float()
    qs = O._QSCALE if name.endswith(".query") else 1.0     # the packer quantises W * log2(e)/sqrt(dh) for the query rows
    qa, sa = quant_rows_i8(x.float() / s)
    qw, sw = quant_rows_i8((W * qs if qs != 1.0 else W) * s[None, :])
    acc = (qa.double().reshape(-1, qa.shape[-1]) @ qw.double().t()).float().reshape(*x.shape[:-1], W.shape[0])   # exact int32 sums
    y = acc * (sa * sw.reshape(1, -1) * (1.0 / qs))
    b = w.get(name + ".bias")
    return y if b is None else y + b


@contextlib.contextmanager
def int8_rounding(dtype=torch.float16, fp8_first: int = 0, fp8_qkv: bool = True, smooth: bool = True):
    """`with int8_rounding(dtype, ...) as mm:` — the oracle with the int8 configuration's rounding points."""
    orig = O.linear_fp8
    with O.device_rounding(dtype, fp8=True, fp8_first=fp8_first, fp8_qkv=fp8_qkv) as mm:
        O.linear_fp8 = lambda x, w, name: linear_i8(x, w, name, smooth=smooth, mm=mm)
        try:
            yield mm
        finally:
            O.linear_fp8 = orig
