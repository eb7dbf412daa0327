"""rnnt_loss, transducer_joint and ctc_loss: the training-side functions over librnnt_hip.so.

rnnt_loss: the transducer loss with gradients, torchaudio.functional.rnnt_loss's signature.  CUDA tensors run rnnt_transducer_loss
(float32) or rnnt_transducer_loss_elem (bfloat16, float16: the lattice is read and the gradient written in 16 bits) on torch's
current stream; CPU tensors run rnnt_transducer_loss_host, the plain C++ twin.  transducer_joint / TransducerJoint: the joint
lattice in front of it with its backward (rnnt_joint_lattice_forward / _backward).  transducer_joint_loss / TransducerJoint.loss: the
two fused, so that no [B, T, U1, V] tensor exists on the device (rnnt_joint_loss_forward / _backward).  ctc_loss / CTCHead: the CTC term of the reference's
objective, torch.nn.functional.ctc_loss's signature (rnnt_ctc_loss / rnnt_ctc_loss_elem / rnnt_ctc_loss_host).  lstm_predictor /
RNNPredictor: the predictor's LSTM over a whole label sequence with back-propagation through time (rnnt_lstm_forward / _backward /
_host), under the reference's parameter names.  rel_attention / RelPositionMultiHeadedAttention: the attention core of an encoder layer
(relative positions, chunk mask) with gradients and no [T, T] tensor (rnnt_rel_attention_forward / _backward / _host).  There is no
eager-PyTorch path on the device."""
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


# ---- the joint lattice with gradients (rnnt_joint_lattice_forward / _backward) ---------------------------------------------------
def _aligned(t):
    """contiguous and 16-byte aligned (a view into a larger tensor may start anywhere)"""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _lens_np(lens):
    return None if lens is None else (lens.detach().cpu().numpy() if isinstance(lens, torch.Tensor) else np.asarray(lens)).astype(np.int32)


class _TransducerJoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, p, w, b, logit_lengths, target_lengths):
        B, T, D = e.shape
        U1, V = p.shape[1], w.shape[0]
        ea, pa, wa, ba = _aligned(e), _aligned(p), _aligned(w), _aligned(b)
        if ea.is_cuda:
            with torch.cuda.device(ea.device):
                nbytes = rlib.joint_lattice_workspace(B, T, U1, V)
                work = torch.empty(nbytes, dtype=torch.uint8, device=ea.device)
                out = torch.empty(B, T, U1, V, dtype=torch.float32, device=ea.device)
                rlib.joint_lattice_forward_device(ea.data_ptr(), pa.data_ptr(), wa.data_ptr(), ba.data_ptr(), (B, T, U1, V), out.data_ptr(),
                                                  work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        else:                                                      # the host side is f64 like every host twin, one batch row at a time
            rlib.joint_lattice_workspace(B, T, U1, V)              # the same refusals as on the device
            w64, b64 = wa.double(), ba.double()
            out = torch.stack([(torch.tanh(ea[i].double().unsqueeze(1) + pa[i].double().unsqueeze(0)) @ w64.T + b64).float() for i in range(B)])
        ctx.save_for_backward(e, p, w, b)
        ctx.lens = (_lens_np(logit_lengths), _lens_np(target_lengths))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        e, p, w, b = ctx.saved_tensors
        B, T, _ = e.shape
        U1, V = p.shape[1], w.shape[0]
        ll, tl = ctx.lens
        ea, pa, wa, ga = _aligned(e), _aligned(p), _aligned(w), _aligned(grad_out.to(torch.float32))
        if ea.is_cuda:
            with torch.cuda.device(ea.device):
                nbytes = rlib.joint_lattice_workspace(B, T, U1, V)
                work = torch.empty(nbytes, dtype=torch.uint8, device=ea.device)
                de, dp, dw, db = torch.empty_like(ea), torch.empty_like(pa), torch.empty_like(wa), torch.empty(V, dtype=torch.float32, device=ea.device)
                rlib.joint_lattice_backward_device(ea.data_ptr(), pa.data_ptr(), wa.data_ptr(), ga.data_ptr(), ll, tl, (B, T, U1, V), de.data_ptr(),
                                                   dp.data_ptr(), dw.data_ptr(), db.data_ptr(), work.data_ptr(), nbytes,
                                                   torch.cuda.current_stream().cuda_stream)
        else:
            de, dp, dw, db = (torch.from_numpy(a.astype(np.float32)) for a in
                              rlib.joint_lattice_backward_host(ea.numpy(), pa.numpy(), wa.numpy(), ga.numpy(), ll, tl))
        return de, dp, dw, db, None, None


def transducer_joint(enc_proj, pred_proj, weight, bias, logit_lengths=None, target_lengths=None):
    """The joint lattice of the reference's TransducerJoint (prejoin linear, add, tanh) behind its two projections, differentiable:
    logits[b, t, u, :] = tanh(enc_proj[b, t, :] + pred_proj[b, u, :]) @ weight.T + bias, float32 [B, T, U1, V].

    enc_proj [B, T, 256] = joint.enc_ffn(encoder output), pred_proj [B, U1, 256] = joint.pred_ffn(predictor output), weight [V, 256] and
    bias [V] = joint.ffn_out's; V a multiple of 4 in 4..416.  All four float32 on one device: CUDA tensors run rnnt_joint_lattice_forward
    and, in .backward(), rnnt_joint_lattice_backward on torch's current stream (bf16x3 MFMAs, bit-for-bit repeatable); CPU tensors run
    the float64 host side (rnnt_joint_lattice_backward_host for the gradients).  Neither tanh(e + p) nor e + p is ever stored: the
    backward recomputes tanh from the four inputs, which are all that is saved.

    logit_lengths [B] (frames per row) and target_lengths [B] (labels per row), as given to rnnt_loss: when present the backward never
    reads the incoming gradient at cells with t >= T_b or u > U_b (rnnt_loss writes exact zeros there; another caller's padding may
    hold anything) and they contribute nothing.  The forward writes every cell either way.

    Any dtype but float32: TypeError.  A refused call (V out of range, a length out of range, too many cells) raises RnntError with the
    library's status code."""
    for name, t in (("enc_proj", enc_proj), ("pred_proj", pred_proj), ("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"transducer_joint: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    D = rlib.JOINT_D
    if enc_proj.dim() != 3 or pred_proj.dim() != 3 or weight.dim() != 2 or bias.dim() != 1 or enc_proj.size(2) != D or pred_proj.size(2) != D or \
            weight.size(1) != D or pred_proj.size(0) != enc_proj.size(0) or bias.size(0) != weight.size(0):
        raise RnntError(f"transducer_joint: want enc_proj [B, T, {D}], pred_proj [B, U1, {D}], weight [V, {D}], bias [V]; got "
                        f"{tuple(enc_proj.shape)}, {tuple(pred_proj.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}", rlib.ERR_ARG)
    if len({t.device for t in (enc_proj, pred_proj, weight, bias)}) != 1:
        raise RnntError("transducer_joint: the four tensors must be on one device", rlib.ERR_ARG)
    B = enc_proj.size(0)
    for name, lens, hi in (("logit_lengths", logit_lengths, enc_proj.size(1)), ("target_lengths", target_lengths, pred_proj.size(1) - 1)):
        if lens is not None:                                       # refused at the forward, not first in the backward
            a = _lens_np(lens)
            if a.shape != (B,) or (a < (1 if name == "logit_lengths" else 0)).any() or (a > hi).any():
                raise RnntError(f"transducer_joint: {name} must be [{B}] values up to {hi}, got {a.tolist()}", rlib.ERR_ARG)
    return _TransducerJoint.apply(enc_proj, pred_proj, weight, bias, logit_lengths, target_lengths)


# ---- the fused joint and loss (rnnt_joint_loss_forward / _backward): no [B, T, U1, V] tensor on the device ------------------------
class _TransducerJointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, p, w, b, targets, logit_lengths, target_lengths, blank, clamp):
        B, T, D = e.shape
        U1, V = p.shape[1], w.shape[0]
        ea, pa, wa, ba = _aligned(e), _aligned(p), _aligned(w), _aligned(b)
        tg = targets.detach().cpu().numpy().astype(np.int32)
        if tg.shape != (B, U1 - 1):
            raise RnntError(f"transducer_joint_loss: pred_proj {tuple(p.shape)} wants targets of shape {(B, U1 - 1)}, got {tg.shape}", rlib.ERR_ARG)
        ll, tl = _lens_np(logit_lengths), _lens_np(target_lengths)
        if ea.is_cuda:
            with torch.cuda.device(ea.device):
                wbytes, sbytes = rlib.joint_loss_workspace(B, T, U1, V)
                work = torch.empty(wbytes, dtype=torch.uint8, device=ea.device)
                state = torch.empty(sbytes, dtype=torch.uint8, device=ea.device)
                nll = torch.empty(B, dtype=torch.float64, device=ea.device)
                rlib.joint_loss_forward_device(ea.data_ptr(), pa.data_ptr(), wa.data_ptr(), ba.data_ptr(), tg, ll, tl, (B, T, U1, V), blank, nll.data_ptr(),
                                               state.data_ptr(), sbytes, work.data_ptr(), wbytes, torch.cuda.current_stream().cuda_stream)
            ctx.save_for_backward(e, p, w, b, state)
        else:                                                      # the float64 host twin: there the lattice and its gradient exist
            nll = torch.from_numpy(rlib.joint_loss_host(ea.numpy(), pa.numpy(), wa.numpy(), ba.numpy(), tg, ll, tl, blank, clamp)[0])
            ctx.save_for_backward(e, p, w, b)
        ctx.tg = tg
        ctx.args = (ll, tl, blank, clamp)
        return nll.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        e, p, w, b = ctx.saved_tensors[:4]
        B, T, _ = e.shape
        U1, V = p.shape[1], w.shape[0]
        ll, tl, blank, clamp = ctx.args
        ea, pa, wa, ba = _aligned(e), _aligned(p), _aligned(w), _aligned(b)
        if ea.is_cuda:
            with torch.cuda.device(ea.device):
                scale = _aligned(grad_out.float())
                wbytes, sbytes = rlib.joint_loss_workspace(B, T, U1, V)
                work = torch.empty(wbytes, dtype=torch.uint8, device=ea.device)
                de, dp, dw, db = torch.empty_like(ea), torch.empty_like(pa), torch.empty_like(wa), torch.empty(V, dtype=torch.float32, device=ea.device)
                state = ctx.saved_tensors[4]
                rlib.joint_loss_backward_device(ea.data_ptr(), pa.data_ptr(), wa.data_ptr(), ba.data_ptr(), state.data_ptr(), sbytes, scale.data_ptr(), clamp,
                                                (B, T, U1, V), blank, de.data_ptr(), dp.data_ptr(), dw.data_ptr(), db.data_ptr(), work.data_ptr(), wbytes,
                                                torch.cuda.current_stream().cuda_stream)
        else:
            outs = rlib.joint_loss_host(ea.numpy(), pa.numpy(), wa.numpy(), ba.numpy(), ctx.tg, ll, tl, blank, clamp, grad_out.detach().double().numpy())[1]
            de, dp, dw, db = (torch.from_numpy(a.astype(np.float32)) for a in outs)
        return de, dp, dw, db, None, None, None, None, None


def transducer_joint_loss(enc_proj, pred_proj, weight, bias, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, reduction="mean"):
    """rnnt_loss(transducer_joint(enc_proj, pred_proj, weight, bias), targets, logit_lengths, target_lengths, ...) as ONE differentiable
    function that never stores the [B, T, U1, V] lattice or its gradient on the device.

    enc_proj [B, T, 256], pred_proj [B, Umax + 1, 256], weight [V, 256], bias [V] float32 as for transducer_joint (V a multiple of 4 in
    4..416, Umax <= 255); targets [B, Umax], logit_lengths [B], target_lengths [B], blank (-1: V - 1), clamp and reduction as for
    rnnt_loss.  Returns float32 costs, [B] or reduced.

    CUDA tensors: the forward runs rnnt_joint_loss_forward on torch's current stream (the lattice kernel keeps a cell's vocabulary row
    in registers and leaves two picked log-probabilities and lse per cell; the f64 recursions follow) and computes no gradient.  It
    saves the four inputs and one `state` tensor of 16 bytes per cell plus the lengths and targets.  The backward runs
    rnnt_joint_loss_backward with the incoming gradient [B] as the per-row scale: the logits are recomputed in registers (bf16x3
    MFMAs), g = clamp(d nll_b / d logits) * grad_out[b] is formed there and contracted at once.  Bit-for-bit repeatable.
    The recomputed logits differ from the forward's in summation order only.

    CPU tensors run rnnt_joint_loss_host, which composes the float64 host sides of the joint forward, rnnt_transducer_loss_host, the
    scaling and rnnt_joint_lattice_backward_host with nothing rounded between them (forward and backward each run it): on the CPU the
    lattice and its gradient DO exist, in float64, inside that call.

    Any dtype but float32: TypeError.  A refused call (shapes, V, a length or label out of range, the blank inside a transcript,
    Umax > 255, ...) raises RnntError with the library's status code."""
    for name, t in (("enc_proj", enc_proj), ("pred_proj", pred_proj), ("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"transducer_joint_loss: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"transducer_joint_loss: reduction must be one of {REDUCTIONS}, got {reduction!r}")
    D = rlib.JOINT_D
    if enc_proj.dim() != 3 or pred_proj.dim() != 3 or weight.dim() != 2 or bias.dim() != 1 or enc_proj.size(2) != D or pred_proj.size(2) != D or \
            weight.size(1) != D or pred_proj.size(0) != enc_proj.size(0) or bias.size(0) != weight.size(0):
        raise RnntError(f"transducer_joint_loss: want enc_proj [B, T, {D}], pred_proj [B, U1, {D}], weight [V, {D}], bias [V]; got "
                        f"{tuple(enc_proj.shape)}, {tuple(pred_proj.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}", rlib.ERR_ARG)
    if len({t.device for t in (enc_proj, pred_proj, weight, bias)}) != 1:
        raise RnntError("transducer_joint_loss: the four tensors must be on one device", rlib.ERR_ARG)
    if targets is None or logit_lengths is None or target_lengths is None:
        raise RnntError("transducer_joint_loss: targets, logit_lengths and target_lengths are required", rlib.ERR_ARG)
    V = weight.size(0)
    costs = _TransducerJointLoss.apply(enc_proj, pred_proj, weight, bias, targets, logit_lengths, target_lengths, V - 1 if blank == -1 else int(blank),
                                       float(clamp))
    return costs if reduction == "none" else (costs.mean() if reduction == "mean" else costs.sum())


class TransducerJoint(torch.nn.Module):
    """The reference's TransducerJoint (model/component/joint.py) in its one trained configuration -- prejoin linear, add, tanh, no
    postjoin linear -- with the reference's parameter names (enc_ffn, pred_ffn, ffn_out), so its `joint.*` checkpoint entries load.
    The two small projections are nn.Linear (torch autograd); the lattice and its backward are transducer_joint; `loss` is the lattice
    and the transducer loss in one, transducer_joint_loss."""

    def __init__(self, vocab_size, enc_output_size, pred_output_size, join_dim=256):
        super().__init__()
        if join_dim != rlib.JOINT_D:
            raise RnntError(f"TransducerJoint: the lattice kernels are built for join_dim {rlib.JOINT_D}, got {join_dim}", rlib.ERR_SHAPE)
        self.enc_ffn = torch.nn.Linear(enc_output_size, join_dim)
        self.pred_ffn = torch.nn.Linear(pred_output_size, join_dim)
        self.ffn_out = torch.nn.Linear(join_dim, vocab_size)

    def forward(self, enc_out, pred_out, logit_lengths=None, target_lengths=None):
        return transducer_joint(self.enc_ffn(enc_out), self.pred_ffn(pred_out), self.ffn_out.weight, self.ffn_out.bias, logit_lengths, target_lengths)

    def loss(self, enc_out, pred_out, targets, logit_lengths, target_lengths, **kw):
        """The transducer loss of this joint's lattice without the lattice: the two projections, then transducer_joint_loss (blank, clamp
        and reduction as keywords)."""
        return transducer_joint_loss(self.enc_ffn(enc_out), self.pred_ffn(pred_out), self.ffn_out.weight, self.ffn_out.bias, targets, logit_lengths,
                                     target_lengths, **kw)


# ---- the CTC loss with gradients (rnnt_ctc_loss): torch.nn.functional.ctc_loss's signature ----------------------------------------
def _ctc_strides(x):
    """(stride_b, stride_t) in elements of a [T, B, V] tensor whose frames rnnt_ctc_loss can address as they lie, else None"""
    T, B, V = x.shape
    st, sb, sv = x.stride()
    if B == 1:
        sb = max(sb, T * st) if T > 1 else V
    if T == 1:
        st = B * sb
    if (V > 1 and sv != 1) or sb < V or st < V or not (sb >= T * st or st >= B * sb):
        return None
    return None if x.data_ptr() % 16 else (sb, st)


class _CtcLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, tg, il, tl, blank, fused_log_softmax):
        x = log_probs.detach()
        T, B, V = x.shape
        if x.is_cuda:
            strides = _ctc_strides(x)
            if strides is None:
                x = _aligned(x)
                strides = (V, B * V)
            sb, st = strides
            with torch.cuda.device(x.device):
                nbytes = rlib.ctc_loss_workspace(B, T, tg.shape[1])
                work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                nll = torch.empty(B, dtype=torch.float64, device=x.device)
                grad = torch.empty_strided((T, B, V), (st, sb, 1), dtype=x.dtype, device=x.device)
                rlib.ctc_loss_device(x.data_ptr(), (B, T, V), (sb, st), tg, il, tl, blank, fused_log_softmax, nll.data_ptr(), grad.data_ptr(),
                                     work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream,
                                     elem=None if x.dtype == torch.float32 else ELEMS[x.dtype])
        else:                                                      # 16-bit input widens exactly; the f64 gradient is rounded f32 -> E
            nll_np, grad_np = rlib.ctc_loss_host(x.float().transpose(0, 1).numpy(), tg, il, tl, blank, fused_log_softmax)
            nll, grad = torch.from_numpy(nll_np), torch.from_numpy(grad_np.astype(np.float32)).transpose(0, 1).to(x.dtype)
        ctx.save_for_backward(grad)
        return nll.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        if grad.dtype == torch.float32:
            return grad * grad_out.to(grad.dtype).view(1, -1, 1), None, None, None, None, None
        # 16 bits: the product is formed in float32 per element and rounded once; the scale itself is never rounded to 16 bits
        return torch.mul(grad, grad_out.to(torch.float32).view(1, -1, 1), out=torch.empty_like(grad)), None, None, None, None, None


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction="mean", zero_infinity=False, fused_log_softmax=False):
    """The CTC loss of torch.nn.functional.ctc_loss, with its signature and argument conventions.

    log_probs [T, B, V] float32, bfloat16 or float16; targets [B, Lmax] padded integer labels, or 1-D: the rows' labels one after the
    other (unpacked on the host); input_lengths [B] (frames per row, 1..T); target_lengths [B] (labels per row, 0..Lmax <= 255).
    reduction: "none" ([B]), "sum", or "mean" = mean_b(nll_b / max(L_b, 1)), torch's definition.  Returns a FLOAT32 tensor on
    log_probs' device whatever their dtype; `.backward()` gives log_probs.grad in log_probs' dtype.

    fused_log_softmax=True: `log_probs` holds LOGITS; the function takes the log-softmax itself (float32, max-subtracted) and returns
    the gradient with respect to the logits, p_k - occupancy, so a trainer's separate log-softmax forward and backward over [T, B, V]
    disappear.  False (torch's meaning): the input holds log-probabilities and is differentiated as it stands.

    Any batch and frame strides with unit stride over V run without a copy: a contiguous [T, B, V] tensor, and the transposed view of
    a contiguous [B, T, V] one (what the reference passes).  Anything else (or a base that is not 16-byte aligned) is made
    contiguous.  A 16-bit input is read and its gradient written in 16 bits, each gradient element rounded once, to nearest even.

    A row whose frames cannot hold its transcript has loss +inf -- 0 with zero_infinity=True -- and a gradient of EXACTLY 0 either
    way: a deliberate departure from torch, which writes NaN into such a row unless zero_infinity is set.  Frames t >= T_b and
    targets beyond a row's length are never read; the gradient of such frames is exactly 0.

    The forward computes d nll_b / d input eagerly and saves it; the backward scales it per row.  CUDA tensors run rnnt_ctc_loss /
    rnnt_ctc_loss_elem on torch's current stream; CPU tensors run rnnt_ctc_loss_host, the float64 C++ twin.  Any other dtype: TypeError.
    A refused call (a length or label out of range, the blank inside a transcript, Lmax > 255, ...) raises RnntError with the
    library's status code."""
    if not isinstance(log_probs, torch.Tensor) or log_probs.dtype not in ELEMS:
        raise TypeError(f"ctc_loss: log_probs must be a float32, bfloat16 or float16 tensor, got {getattr(log_probs, 'dtype', type(log_probs))}")
    if log_probs.dim() != 3:
        raise RnntError(f"ctc_loss: log_probs must be [T, B, V], got {tuple(log_probs.shape)}", rlib.ERR_ARG)
    if reduction not in REDUCTIONS:
        raise ValueError(f"ctc_loss: reduction must be one of {REDUCTIONS}, got {reduction!r}")
    B = log_probs.size(1)
    il, tl = _lens_np(input_lengths).reshape(-1), _lens_np(target_lengths).reshape(-1)
    tg = _lens_np(targets)
    if il.shape != (B,) or tl.shape != (B,):
        raise RnntError(f"ctc_loss: {B} rows, but lengths of shapes {il.shape} and {tl.shape}", rlib.ERR_ARG)
    if tg.ndim == 1:                                               # concatenated: row b is the next L_b labels
        if (tl < 0).any() or int(tl.sum()) != tg.size:
            raise RnntError(f"ctc_loss: {tg.size} concatenated targets, but target_lengths sum to {int(tl.sum())}", rlib.ERR_ARG)
        flat, tg, at = tg, np.zeros((B, int(tl.max()) if B else 0), np.int32), 0
        for b in range(B):
            tg[b, :tl[b]] = flat[at:at + tl[b]]
            at += tl[b]
    elif tg.ndim != 2 or tg.shape[0] != B:
        raise RnntError(f"ctc_loss: targets must be [{B}, Lmax] or 1-D, got {tg.shape}", rlib.ERR_ARG)
    costs = _CtcLoss.apply(log_probs, np.ascontiguousarray(tg), il, tl, int(blank), bool(fused_log_softmax))
    if zero_infinity:
        costs = torch.where(torch.isinf(costs), torch.zeros_like(costs), costs)
    if reduction == "none":
        return costs
    if reduction == "sum":
        return costs.sum()
    return (costs / torch.from_numpy(np.maximum(tl, 1)).to(device=costs.device, dtype=costs.dtype)).mean()


class CTCHead(torch.nn.Module):
    """The reference's OnlineCTC (model/online_rnnt_model.py) with its parameter name, ctc_lo, so `ctc_head.ctc_lo.*` checkpoint
    entries load.  The projection is nn.Linear (torch autograd, the split TransducerJoint makes too); the log-softmax, the loss and
    their backward are ctc_loss with fused_log_softmax=True over the transposed view of the logits: no [T, B, V] copy, no separate
    log-softmax pass."""

    def __init__(self, vocab_size, encoder_output_size, dropout_rate=0.0, blank_id=0):
        super().__init__()
        self.ctc_lo = torch.nn.Linear(encoder_output_size, vocab_size)
        self.dropout_rate = dropout_rate
        self.blank_id = blank_id

    def forward(self, hs_pad, hlens, ys_pad, ys_lens, return_log_probs=False):
        """hs_pad [B, T, D], hlens [B], ys_pad [B, Lmax] (anything beyond a row's length, e.g. -1), ys_lens [B] -> (loss, ys_hat): the
        reference's loss (reduction "mean", zero_infinity) and, only when asked for, its [B, T, V] log-probabilities (else None)."""
        logits = self.ctc_lo(torch.nn.functional.dropout(hs_pad, p=self.dropout_rate))
        loss = ctc_loss(logits.transpose(0, 1), ys_pad, hlens, ys_lens, blank=self.blank_id, reduction="mean", zero_infinity=True,
                        fused_log_softmax=True)
        return loss, (logits.log_softmax(2) if return_log_probs else None)

    def log_softmax(self, hs_pad):
        return torch.nn.functional.log_softmax(self.ctc_lo(hs_pad), dim=2)

    def argmax(self, hs_pad):
        return torch.argmax(self.ctc_lo(hs_pad), dim=2)


# ---- the predictor's LSTM over a whole label sequence with gradients (rnnt_lstm_forward / _backward) ------------------------------
class _LstmPredictor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0, lengths):
        B, U1, D = x.shape
        xa, wia, wha, bia, bha = (_aligned(t) for t in (x, w_ih, w_hh, b_ih, b_hh))
        h0a, c0a = (None if t is None else _aligned(t) for t in (h0, c0))
        lens = _lens_np(lengths)
        ptr = lambda t: None if t is None else t.data_ptr()
        if xa.is_cuda:
            with torch.cuda.device(xa.device):
                wbytes, sbytes = rlib.lstm_workspace(B, U1)
                work = torch.empty(wbytes, dtype=torch.uint8, device=xa.device)
                state = torch.empty(sbytes, dtype=torch.uint8, device=xa.device)
                out = torch.empty(B, U1, D, dtype=torch.float32, device=xa.device)
                hn, cn = torch.empty(B, D, dtype=torch.float32, device=xa.device), torch.empty(B, D, dtype=torch.float32, device=xa.device)
                rlib.lstm_forward_device(xa.data_ptr(), wia.data_ptr(), wha.data_ptr(), bia.data_ptr(), bha.data_ptr(), ptr(h0a), ptr(c0a), lens, (B, U1),
                                         out.data_ptr(), hn.data_ptr(), cn.data_ptr(), state.data_ptr(), sbytes, work.data_ptr(), wbytes,
                                         torch.cuda.current_stream().cuda_stream)
        else:                                                      # the float64 host twin, rounded once; it saves nothing: the backward runs it again
            npy = lambda t: None if t is None else t.numpy()
            out, hn, cn = (torch.from_numpy(a.astype(np.float32)) for a in
                           rlib.lstm_host(xa.numpy(), wia.numpy(), wha.numpy(), bia.numpy(), bha.numpy(), npy(h0a), npy(c0a), lens))
            state = torch.empty(0, dtype=torch.uint8)
        ctx.has = (h0 is not None, c0 is not None)
        ctx.lens = lens
        ctx.save_for_backward(x, w_ih, w_hh, b_ih, b_hh, *(t for t in (h0, c0) if t is not None), out, state)
        ctx.mark_non_differentiable(hn, cn)
        return out, hn, cn

    @staticmethod
    def backward(ctx, dout, _dhn, _dcn):
        saved = list(ctx.saved_tensors)
        x, w_ih, w_hh, b_ih, b_hh = saved[:5]
        state, out = saved.pop(), saved.pop()
        rest = saved[5:]
        h0 = rest.pop(0) if ctx.has[0] else None
        c0 = rest.pop(0) if ctx.has[1] else None
        B, U1, D = x.shape
        xa, wia, wha, da = (_aligned(t) for t in (x, w_ih, w_hh, dout.to(torch.float32)))
        h0a, c0a = (None if t is None else _aligned(t) for t in (h0, c0))
        ptr = lambda t: None if t is None else t.data_ptr()
        if xa.is_cuda:
            with torch.cuda.device(xa.device):
                wbytes, sbytes = rlib.lstm_workspace(B, U1)
                work = torch.empty(wbytes, dtype=torch.uint8, device=xa.device)
                new = lambda *s: torch.empty(*s, dtype=torch.float32, device=xa.device)
                dx, dwi, dwh, db, dh0, dc0 = new(B, U1, D), new(4 * D, D), new(4 * D, D), new(4 * D), new(B, D), new(B, D)
                rlib.lstm_backward_device(xa.data_ptr(), wia.data_ptr(), wha.data_ptr(), ptr(h0a), ptr(c0a), _aligned(out).data_ptr(), state.data_ptr(), sbytes,
                                          da.data_ptr(), ctx.lens, (B, U1), dx.data_ptr(), dwi.data_ptr(), dwh.data_ptr(), db.data_ptr(), dh0.data_ptr(),
                                          dc0.data_ptr(), work.data_ptr(), wbytes, torch.cuda.current_stream().cuda_stream)
        else:
            npy = lambda t: None if t is None else t.numpy()
            dx, dwi, dwh, db, dh0, dc0 = (torch.from_numpy(a.astype(np.float32)) for a in
                                          rlib.lstm_host(xa.numpy(), wia.numpy(), wha.numpy(), b_ih.detach().numpy(), b_hh.detach().numpy(), npy(h0a), npy(c0a), ctx.lens,
                                                         dout=da.numpy())[3:])
        return dx, dwi, dwh, db, db.clone(), dh0 if ctx.has[0] else None, dc0 if ctx.has[1] else None, None


def lstm_predictor(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, lengths=None):
    """The predictor's LSTM layer -- torch.nn.LSTM(256, 256, one layer, batch_first) -- over a whole label sequence, differentiable:
    (out [B, U1, 256], hN [B, 256], cN [B, 256]).

    x [B, U1, 256]; w_ih, w_hh [1024, 256] and b_ih, b_hh [1024] in torch.nn.LSTM's layout (gate order i, f, g, o); h0, c0 [B, 256] or
    None (zeros); lengths [B] (valid steps per row, 1..U1; the transducer caller passes target_lengths + 1) or None.  All float32 on one
    device.  `out` is differentiable with respect to x, the four weights, h0 and c0; hN and cN are the state after each row's last
    valid step and are returned non-differentiable.  With lengths, x and the incoming gradient beyond a row's length are never read,
    and out and x.grad there are exactly 0.

    CUDA tensors run rnnt_lstm_forward and, in .backward(), rnnt_lstm_backward on torch's current stream: one recurrence launch each
    whatever U1 is, float32 throughout with the inference predictor's activations, bit-for-bit repeatable.  Saved for the backward:
    the inputs, out and one state tensor (the activated gates and c of every step, 5120 bytes per row and step).  CPU tensors run
    rnnt_lstm_host, the float64 C++ twin (the backward runs it again instead of saving a state).

    Any dtype but float32: TypeError.  Shape or device disagreements, or a length out of range: RnntError(ERR_ARG); U1 > 256:
    RnntError(ERR_SHAPE)."""
    named = (("x", x), ("w_ih", w_ih), ("w_hh", w_hh), ("b_ih", b_ih), ("b_hh", b_hh), ("h0", h0), ("c0", c0))
    for name, t in named:
        if (t is not None or name not in ("h0", "c0")) and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise TypeError(f"lstm_predictor: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    D = rlib.LSTM_D
    B = x.size(0) if x.dim() == 3 else -1
    if x.dim() != 3 or x.size(2) != D or tuple(w_ih.shape) != (4 * D, D) or tuple(w_hh.shape) != (4 * D, D) or tuple(b_ih.shape) != (4 * D,) or \
            tuple(b_hh.shape) != (4 * D,) or any(t is not None and tuple(t.shape) != (B, D) for t in (h0, c0)):
        raise RnntError(f"lstm_predictor: want x [B, U1, {D}], w_ih and w_hh [{4 * D}, {D}], b_ih and b_hh [{4 * D}], h0 and c0 [B, {D}]; got "
                        + ", ".join(f"{n} {tuple(t.shape)}" for n, t in named if t is not None), rlib.ERR_ARG)
    if len({t.device for _, t in named if t is not None}) != 1:
        raise RnntError("lstm_predictor: every tensor must be on one device", rlib.ERR_ARG)
    if lengths is not None:
        a = _lens_np(lengths)
        if a.shape != (B,) or (a < 1).any() or (a > x.size(1)).any():
            raise RnntError(f"lstm_predictor: lengths must be [{B}] values in 1..{x.size(1)}, got {a.tolist()}", rlib.ERR_ARG)
    return _LstmPredictor.apply(x, w_ih, w_hh, b_ih, b_hh, h0, c0, lengths)


class _LstmParams(torch.nn.Module):
    """the four parameters of a one-layer torch.nn.LSTM under its names, initialised as torch does (uniform in +-1 / sqrt(hidden))"""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        k = hidden_size ** -0.5
        for name, shape in (("weight_ih_l0", (4 * hidden_size, input_size)), ("weight_hh_l0", (4 * hidden_size, hidden_size)),
                            ("bias_ih_l0", (4 * hidden_size,)), ("bias_hh_l0", (4 * hidden_size,))):
            setattr(self, name, torch.nn.Parameter(torch.empty(shape).uniform_(-k, k)))


class RNNPredictor(torch.nn.Module):
    """The reference's RNNPredictor (model/component/predictor.py) in its one trained configuration -- embedding 256, one LSTM layer of
    256, projection to 256 -- with the reference's parameter names (embed.weight, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0,
    rnn.bias_hh_l0, projection.weight, projection.bias), so the `predictor.*` entries of a checkpoint load with strict=True.  The
    embedding, its dropout and the projection are torch modules (the split TransducerJoint and CTCHead make too); the LSTM is
    lstm_predictor."""

    def __init__(self, voca_size, embed_size, output_size, embed_dropout, hidden_size, num_layers, bias=True, rnn_type="lstm", dropout=0.1):
        super().__init__()
        D = rlib.LSTM_D
        if (embed_size, output_size, hidden_size, num_layers, bool(bias), rnn_type) != (D, D, D, 1, True, "lstm"):
            raise RnntError(f"RNNPredictor: the LSTM kernels are built for embed / output / hidden {D}, one lstm layer with bias; got embed_size={embed_size} "
                            f"output_size={output_size} hidden_size={hidden_size} num_layers={num_layers} bias={bias} rnn_type={rnn_type!r}", rlib.ERR_SHAPE)
        self.n_layers = num_layers
        self.hidden_size = hidden_size
        self._output_size = output_size
        self.embed = torch.nn.Embedding(voca_size, embed_size)
        self.dropout = torch.nn.Dropout(embed_dropout)
        self.rnn = _LstmParams(embed_size, hidden_size)
        self.projection = torch.nn.Linear(hidden_size, output_size)

    def output_size(self):
        return self._output_size

    def init_state(self, batch_size, device, method="zero"):
        assert batch_size > 0
        return [torch.zeros(self.n_layers, batch_size, self.hidden_size, device=device) for _ in range(2)]

    def lstm(self, input_tensor, cache=None, lengths=None):
        """(out [B, U1, 256] before the projection, hN, cN [1, B, 256]) -- the reference's self.rnn(embed, states)"""
        embed = self.dropout(self.embed(input_tensor))
        h0, c0 = (None, None) if cache is None else (cache[0][0], cache[1][0])
        r = self.rnn
        out, hn, cn = lstm_predictor(embed, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, h0, c0, lengths)
        return out, hn.unsqueeze(0), cn.unsqueeze(0)

    def forward(self, input_tensor, cache=None, lengths=None):
        """input_tensor [B, U1] token ids (add_blank(texts)); cache None (the zero state) or [h, c], each [1, B, 256]; lengths [B] valid
        steps per row or None -> [B, U1, 256]."""
        return self.projection(self.lstm(input_tensor, cache, lengths)[0])


# ---- an encoder layer's attention core with gradients (rnnt_rel_attention_forward / _backward) -----------------------------------------
class _RelAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, p, u, vb, lengths, chunk_size, num_left_chunks):
        B, T, D = q.shape
        qa, ka, va, pa, ua, vba = (_aligned(t) for t in (q, k, v, p, u, vb))
        lens = _lens_np(lengths)
        if qa.is_cuda:
            with torch.cuda.device(qa.device):
                wbytes, sbytes = rlib.rel_attention_workspace(B, T)
                work = torch.empty(wbytes, dtype=torch.uint8, device=qa.device)
                state = torch.empty(sbytes, dtype=torch.uint8, device=qa.device)
                out = torch.empty(B, T, D, dtype=torch.float32, device=qa.device)
                rlib.rel_attention_forward_device(qa.data_ptr(), ka.data_ptr(), va.data_ptr(), pa.data_ptr(), ua.data_ptr(), vba.data_ptr(), lens, (B, T),
                                                  chunk_size, num_left_chunks, out.data_ptr(), state.data_ptr(), sbytes, work.data_ptr(), wbytes,
                                                  torch.cuda.current_stream().cuda_stream)
        else:                                                      # the float64 host twin, rounded once; it saves nothing: the backward runs it again
            (out64,) = rlib.rel_attention_host(qa.numpy(), ka.numpy(), va.numpy(), pa.numpy(), ua.numpy(), vba.numpy(), lens, chunk_size, num_left_chunks)
            out = torch.from_numpy(out64.astype(np.float32))
            state = torch.empty(0, dtype=torch.uint8)
        ctx.mask = (lens, chunk_size, num_left_chunks)
        ctx.save_for_backward(q, k, v, p, u, vb, out, state)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, u, vb, out, state = ctx.saved_tensors
        lens, chunk_size, num_left_chunks = ctx.mask
        B, T, D = q.shape
        qa, ka, va, pa, ua, vba, da = (_aligned(t) for t in (q, k, v, p, u, vb, dout.to(torch.float32)))
        if qa.is_cuda:
            with torch.cuda.device(qa.device):
                wbytes, sbytes = rlib.rel_attention_workspace(B, T)
                work = torch.empty(wbytes, dtype=torch.uint8, device=qa.device)
                new = lambda *s: torch.empty(*s, dtype=torch.float32, device=qa.device)
                dq, dk, dv, dp, du, dvb = new(B, T, D), new(B, T, D), new(B, T, D), new(T, D), new(*u.shape), new(*vb.shape)
                rlib.rel_attention_backward_device(qa.data_ptr(), ka.data_ptr(), va.data_ptr(), pa.data_ptr(), ua.data_ptr(), vba.data_ptr(),
                                                   _aligned(out).data_ptr(), state.data_ptr(), sbytes, da.data_ptr(), lens, (B, T), chunk_size,
                                                   num_left_chunks, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dp.data_ptr(), du.data_ptr(), dvb.data_ptr(),
                                                   work.data_ptr(), wbytes, torch.cuda.current_stream().cuda_stream)
        else:
            dq, dk, dv, dp, du, dvb = (torch.from_numpy(a.astype(np.float32)) for a in
                                       rlib.rel_attention_host(qa.numpy(), ka.numpy(), va.numpy(), pa.numpy(), ua.numpy(), vba.numpy(), lens, chunk_size,
                                                               num_left_chunks, dout=da.numpy())[1:])
        return dq, dk, dv, dp, du, dvb, None, None, None


def rel_attention(q, k, v, p, pos_bias_u, pos_bias_v, lengths=None, chunk_size=0, num_left_chunks=-1):
    """The attention core of the reference's encoder layer (RelPositionMultiHeadedAttention between its Linears,
    wenet/transformer/attention.py:364-420, with the mask of add_optional_chunk_mask), differentiable: out [B, T, 256].

        s[b,h,i,j] = ((q[b,i,h] + u[h]) . k[b,j,h] + (q[b,i,h] + vb[h]) . p[j,h]) / 8,   a = softmax of s over the visible j,   out = a v
        visible(b,i,j) = j < lengths[b] and (chunk_size <= 0 or j < min(T, (i // chunk_size + 1) chunk_size))
                         and (chunk_size <= 0 or num_left_chunks < 0 or j >= (i // chunk_size - num_left_chunks) chunk_size)

    q, k, v [B, T, 256] as linear_q / _k / _v write them (head h at columns 64 h ..); p [T, 256] = linear_pos(pos_emb[0]); pos_bias_u,
    pos_bias_v [4, 64]; lengths [B] (keys per row, 1..T) or None.  All float32 on one device.  Only keys are masked: every query row is
    live and its gradient flows to the visible keys; a row with no visible key gives zeros and no gradient.  k and v at j >= lengths[b]
    are never read, and dk, dv there are exactly 0.

    CUDA tensors run rnnt_rel_attention_forward and, in .backward(), rnnt_rel_attention_backward on torch's current stream: no
    [T, T] tensor reaches memory, exact-float32 MFMA contractions with a float32 online softmax, bit-for-bit repeatable.  Saved for
    the backward: the six inputs, out and one log-sum-exp per (b, h, i) (16 B T bytes).  CPU tensors run rnnt_rel_attention_host, the
    float64 C++ twin (the backward runs it again instead of saving a state).

    Any dtype but float32: TypeError.  Shape or device disagreements, a length out of range, or num_left_chunks >= 0 without a
    chunk_size: RnntError(ERR_ARG); T > lib.ATTN_TMAX (4096): RnntError(ERR_SHAPE)."""
    named = (("q", q), ("k", k), ("v", v), ("p", p), ("pos_bias_u", pos_bias_u), ("pos_bias_v", pos_bias_v))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"rel_attention: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    D, hb = rlib.ATTN_D, (rlib.ATTN_H, rlib.ATTN_DK)
    if q.dim() != 3 or q.size(2) != D or k.shape != q.shape or v.shape != q.shape or tuple(p.shape) != (q.size(1), D) or tuple(pos_bias_u.shape) != hb or \
            tuple(pos_bias_v.shape) != hb:
        raise RnntError(f"rel_attention: want q, k, v [B, T, {D}], p [T, {D}], pos_bias_u and pos_bias_v [{hb[0]}, {hb[1]}]; got "
                        + ", ".join(f"{n} {tuple(t.shape)}" for n, t in named), rlib.ERR_ARG)
    if len({t.device for _, t in named}) != 1:
        raise RnntError("rel_attention: every tensor must be on one device", rlib.ERR_ARG)
    B, T = q.shape[:2]
    if lengths is not None:
        a = _lens_np(lengths)
        if a.shape != (B,) or (a < 1).any() or (a > T).any():
            raise RnntError(f"rel_attention: lengths must be [{B}] values in 1..{T}, got {a.tolist()}", rlib.ERR_ARG)
    chunk_size, num_left_chunks = int(chunk_size), int(num_left_chunks)
    if num_left_chunks >= 0 and chunk_size <= 0:
        raise RnntError(f"rel_attention: num_left_chunks={num_left_chunks} counts chunks, but chunk_size={chunk_size}", rlib.ERR_ARG)
    return _RelAttention.apply(q, k, v, p, pos_bias_u, pos_bias_v, lengths, chunk_size, num_left_chunks)


class RelPositionMultiHeadedAttention(torch.nn.Module):
    """The reference's RelPositionMultiHeadedAttention (wenet/transformer/attention.py) in its one trained configuration -- 4 heads over
    256 features -- as self-attention without a cache, with the reference's parameter names (linear_q / _k / _v / _out with bias,
    linear_pos without, pos_bias_u, pos_bias_v), so a layer's `self_attn.*` checkpoint entries load with strict=True.  The five
    Linears are torch modules under torch autograd (the split TransducerJoint and RNNPredictor make too); what lies between them is
    rel_attention.  The mask is (lengths, chunk_size, num_left_chunks) instead of a [B, T, T] tensor.  Dropout on the attention
    weights is not built: dropout_rate must be 0."""

    def __init__(self, n_head, n_feat, dropout_rate=0.0):
        super().__init__()
        if (n_head, n_feat) != (rlib.ATTN_H, rlib.ATTN_D) or dropout_rate != 0:
            raise RnntError(f"RelPositionMultiHeadedAttention: the attention kernels are built for {rlib.ATTN_H} heads over {rlib.ATTN_D} features without "
                            f"dropout on the weights; got n_head={n_head} n_feat={n_feat} dropout_rate={dropout_rate}", rlib.ERR_SHAPE)
        self.h, self.d_k = n_head, n_feat // n_head
        self.linear_q = torch.nn.Linear(n_feat, n_feat)
        self.linear_k = torch.nn.Linear(n_feat, n_feat)
        self.linear_v = torch.nn.Linear(n_feat, n_feat)
        self.linear_out = torch.nn.Linear(n_feat, n_feat)
        self.linear_pos = torch.nn.Linear(n_feat, n_feat, bias=False)
        self.pos_bias_u = torch.nn.Parameter(torch.empty(self.h, self.d_k))
        self.pos_bias_v = torch.nn.Parameter(torch.empty(self.h, self.d_k))
        torch.nn.init.xavier_uniform_(self.pos_bias_u)
        torch.nn.init.xavier_uniform_(self.pos_bias_v)

    def forward(self, x, pos_emb, lengths=None, chunk_size=0, num_left_chunks=-1):
        """x [B, T, 256] (query = key = value); pos_emb [1, T, 256]; lengths [B] keys per row or None -> [B, T, 256]"""
        if pos_emb.dim() != 3 or pos_emb.size(0) != 1 or pos_emb.size(1) != x.size(1):
            raise RnntError(f"RelPositionMultiHeadedAttention: pos_emb must be [1, T, {rlib.ATTN_D}] for x {tuple(x.shape)}, got {tuple(pos_emb.shape)}",
                            rlib.ERR_ARG)
        out = rel_attention(self.linear_q(x), self.linear_k(x), self.linear_v(x), self.linear_pos(pos_emb[0]), self.pos_bias_u, self.pos_bias_v, lengths,
                            chunk_size, num_left_chunks)
        return self.linear_out(out)
