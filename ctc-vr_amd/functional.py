"""rnnt_loss: the transducer loss with gradients, torchaudio.functional.rnnt_loss's signature over librnnt_hip.so.

CUDA tensors run rnnt_transducer_loss (float32) or rnnt_transducer_loss_elem (bfloat16, float16: the lattice is read and the
gradient written in 16 bits) on torch's current stream; CPU tensors run rnnt_transducer_loss_host, the plain C++ twin.  There is
no eager-PyTorch path."""
import numpy as np
import torch

from . import lib as rlib
from .lib import RnntError  # noqa: F401  (what a refused call raises)

REDUCTIONS = ("none", "mean", "sum")
ELEMS = {torch.float32: rlib.LOSS_F32, torch.bfloat16: rlib.LOSS_BF16, torch.float16: rlib.LOSS_F16}


class _RnntLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank, clamp, fused_log_softmax):
        B, T, U1, V = logits.shape
        x = logits.detach().contiguous()
        tg = targets.detach().cpu().numpy().astype(np.int32)
        if tg.shape != (B, U1 - 1):
            raise RnntError(f"rnnt_loss: logits {tuple(logits.shape)} want targets of shape {(B, U1 - 1)}, got {tg.shape}", rlib.ERR_ARG)
        ll = logit_lengths.detach().cpu().numpy().astype(np.int32)
        tl = target_lengths.detach().cpu().numpy().astype(np.int32)
        if x.is_cuda:
            with torch.cuda.device(x.device):
                nbytes = rlib.transducer_loss_workspace(B, T, U1)
                work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                nll = torch.empty(B, dtype=torch.float64, device=x.device)
                grad = torch.empty_like(x)
                rlib.transducer_loss_device(x.data_ptr(), (B, T, U1, V), tg, ll, tl, blank, fused_log_softmax, clamp, nll.data_ptr(), grad.data_ptr(),
                                            work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream,
                                            elem=None if x.dtype == torch.float32 else ELEMS[x.dtype])
        else:                                                      # a 16-bit lattice widens exactly; the f64 gradient is rounded f32 -> E
            nll_np, grad_np = rlib.transducer_loss_host(x.float().numpy(), tg, ll, tl, blank, fused_log_softmax, clamp)
            nll, grad = torch.from_numpy(nll_np), torch.from_numpy(grad_np.astype(np.float32)).to(x.dtype)
        ctx.save_for_backward(grad)
        return nll.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        if grad.dtype == torch.float32:
            return grad * grad_out.to(grad.dtype).view(-1, 1, 1, 1), None, None, None, None, None, None
        # 16 bits: the product is formed in float32 per element and rounded once; the scale itself is never rounded to 16 bits
        scaled = torch.mul(grad, grad_out.to(torch.float32).view(-1, 1, 1, 1), out=torch.empty_like(grad))
        return scaled, None, None, None, None, None, None


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, reduction="mean", fused_log_softmax=True):
    """The RNN-T loss of torchaudio.functional.rnnt_loss, with its signature and argument conventions.

    logits [B, T, Umax + 1, V] float32, bfloat16 or float16 (the joint's output); targets [B, Umax] integer labels without the
    blank; logit_lengths [B] (frames per row, 1..T); target_lengths [B] (labels per row, 0..Umax).  blank = -1 means V - 1.  reduction: "none" ([B]), "mean"
    or "sum" over the batch.  fused_log_softmax=False: `logits` already holds log-probabilities.  Returns a FLOAT32 tensor on
    logits' device whatever their dtype -- for 16-bit logits a deliberate departure from torchaudio's "logits' dtype": a loss near
    100 keeps 2 to 3 digits in bfloat16, and autocast keeps losses in float32; `.backward()` gives logits.grad in logits' dtype.

    A 16-bit lattice (what the joint's last Linear writes under torch.autocast) is read and its gradient written in 16 bits: every
    element widens exactly to float32, the arithmetic is the float32 call's, each gradient element is rounded once, to nearest
    even; no float32 copy of the lattice exists at any point.  The backward rounds grad * incoming once more, from a float32 product.

    The forward computes d nll_b / d logits eagerly (one more pass over the lattice) and saves it; the backward multiplies it by
    the incoming gradient.  clamp > 0 clamps every element of d nll_b / d logits to [-clamp, clamp] BEFORE that scaling (so before
    the 1 / B of "mean"); this order is restated from torchaudio's documentation and is not pinned against torchaudio itself.
    Cells beyond a row's lengths and targets beyond its length are never read; their gradient is exactly 0.

    Any other dtype: TypeError; non-contiguous input is made contiguous.  A refused call (a length or label out of
    range, the blank inside a transcript, Umax > 255, ...) raises RnntError with the library's status code."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in ELEMS:
        raise TypeError(f"rnnt_loss: logits must be a float32, bfloat16 or float16 tensor, got {getattr(logits, 'dtype', type(logits))}")
    if logits.dim() != 4:
        raise RnntError(f"rnnt_loss: logits must be [B, T, Umax + 1, V], got {tuple(logits.shape)}", rlib.ERR_ARG)
    if reduction not in REDUCTIONS:
        raise ValueError(f"rnnt_loss: reduction must be one of {REDUCTIONS}, got {reduction!r}")
    V = logits.size(-1)
    costs = _RnntLoss.apply(logits, targets, logit_lengths, target_lengths, V - 1 if blank == -1 else int(blank), float(clamp), bool(fused_log_softmax))
    return costs if reduction == "none" else (costs.mean() if reduction == "mean" else costs.sum())
