"""The rounding-model constants every float64 reference (moe_ref64, rowops_ref64, logprob_ref64, olmo_ref64, lora_ref64, linear_ref64) shares.

    GEMM / reduction element:  |out - ref| <= u |ref| + C32 sqrt(n) u32 (|A| |B|)  (+ tiny)
        u = 2^-8 bf16, 2^-11 f16, 2^-24 fp32 (output rounding, a relative half-ulp doubled for margin; f16 adds its subnormal
        spacing 2^-24 as an absolute floor); u32 = 2^-24; n = contraction length; |A| |B| the product of the absolute operands
        (the magnitude fp32 accumulation errors scale with)."""
import numpy as np
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U32 = 2.0 ** -24
C32 = 4.0
# absolute floor of the output rounding: f16's subnormal spacing (bf16 and fp32 share fp32's range)
TINY = {torch.bfloat16: 1e-38, torch.float16: 2.0 ** -24, torch.float32: 1e-38}


def bound(ref: torch.Tensor, mag: torch.Tensor, n: int, dtype) -> torch.Tensor:
    return U[dtype] * ref.abs() + C32 * np.sqrt(max(n, 1)) * U32 * mag + TINY[dtype]
