"""Float64 restatement of the LoRA kernels' products (include/dta.h "Low-rank adapters") for the kernels' ROUNDED inputs, with the operand
magnitudes of the project's per-element bound ref64_common.bound(ref, mag, n, dtype):

    |out - ref| <= u |ref| + C32 sqrt(n) u32 mag (+ tiny)        u: the output's rounding, n: the contraction length, mag = |A| |B|

* down:    ref = (X Mᵀ) rscale,  mag = (|X| |M|ᵀ) |rscale|,  n = K.
* wgrad:   ref = rscale (Lᵀ X),  mag = |rscale| (|L|ᵀ |X|),  n = T (fp32 slabs summed in order, rounded once to the output dtype).
Everything stays on the tensors' device (float64 GEMMs of the long shapes take milliseconds on the card, minutes on the host)."""
import torch


def _col(rscale, R, like):
    return torch.ones(R, dtype=torch.float64, device=like.device) if rscale is None else torch.as_tensor(rscale, dtype=torch.float64, device=like.device)


def down_ref(x, m, rscale=None):
    s = _col(rscale, m.shape[0], x)
    return (x.double() @ m.double().t()) * s, (x.double().abs() @ m.double().abs().t()) * s.abs(), x.shape[1]


def wgrad_ref(l, x, rscale=None):
    s = _col(rscale, l.shape[1], x)[:, None]
    return (l.double().t() @ x.double()) * s, (l.double().abs().t() @ x.double().abs()) * s.abs(), x.shape[0]
