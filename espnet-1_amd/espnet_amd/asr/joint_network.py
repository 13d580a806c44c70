"""JointNetwork and RNNTLoss — the transducer objective of ESPnetASRModel (espnet2/asr_transducer/
joint_network.py, warprnnt_pytorch.RNNTLoss as espnet2/asr/espnet_model.py:115-123 builds it).

The reference computes lin_out(tanh(lin_enc(enc) + lin_dec(dec))) into a (B, T, U+1, V) tensor and hands
it to the loss.  Here lin_enc and lin_dec are ordinary Linear nodes, and tanh + lin_out + the loss are
ONE autograd node, RNNTJointLossFn, over csrc/transducer.hip: the logits are never stored.

    forward    ea_rnnt_joint_lse   lse, lp_blank, lp_label per lattice node
               ea_rnnt_lattice     alpha, beta (f64), the loss, and gamma / kappa_blank / kappa_label per node
    backward   in chunks of whole (b, t) rows, each chunk:
               ea_rnnt_joint_dlogits   recomputes the logits, stores dlogits and the rounded h of the chunk
               ea_gemm                 dh = dlogits . W_out;  lin_out.weight.grad += dlogits^T . h
               ea_colsum               lin_out.bias.grad += column sums of the stored dlogits
               ea_rnnt_joint_dact      dpre = dh (1 - h^2); dE = sum_u, dD = sum_t

Four f32 per node live from forward to backward (lse and the three coefficients).  Under amp h, W_out and
the stored dlogits are bf16; E, D and every sum are f32, the lattice recurrences f64.  The chunk count depends on the
shapes only and nothing synchronises with the host, so a training step stays capturable as one graph.

Decoding: E = project_enc(enc_out) once per utterance, D = project_dec(dec_out) per new
label sequence, and step(E, frame, D, k) over csrc/transducer_step.hip for n <= 64 hypotheses at once:
    ea_rnnt_step_logits   tanh + lin_out with the vocabulary split over the grid; the (n, V) logits and a
                          (max, sum exp) pair per vocabulary slice and row
    ea_rnnt_step_select   lse, lp_blank, the top k non-blank log-probabilities and ids per row
"""
from __future__ import annotations

import torch

from typing import NamedTuple, Optional

from .. import hip_ops as ops
from .._lib import (RNNT_MAX_JOINT, RNNT_MAX_U1, RNNT_STEP_MAX_K, RNNT_STEP_MAX_ROWS,  # noqa: F401
                    RNNT_STEP_SW, dt, lib)  # (bound from the header's enums)
from ..layers.common import Bound, rup


class JointStep(NamedTuple):
    """JointNetwork.step's outputs, views of one device buffer (`packed`)."""
    lse: torch.Tensor
    lp_blank: torch.Tensor
    top_value: torch.Tensor
    top_id: torch.Tensor
    logp: Optional[torch.Tensor]
    packed: torch.Tensor

    def host(self):
        """One device-to-host copy -> (lp_blank (n), top values (n, k), top ids (n, k)) as lists."""
        (n, k), p = self.top_id.shape, self.packed.cpu()
        return (p[n:2 * n].tolist(), p[2 * n:2 * n + n * k].view(n, k).tolist(),
                p[2 * n + n * k:].view(torch.int32).view(n, k).tolist())


def check_step(n: int, k: int, V: int):
    """The joint-step kernels' limits (include/espnet_amd.h), refused by name."""
    if not 1 <= n <= RNNT_STEP_MAX_ROWS:
        raise ValueError(f"JointNetwork.step: n={n} rows; the joint-step kernel takes 1 .. {RNNT_STEP_MAX_ROWS} "
                         "(EA_RNNT_STEP_MAX_ROWS)")
    if not 1 <= k <= min(RNNT_STEP_MAX_K, V - 1):
        raise ValueError(f"JointNetwork.step: k={k} with vocabulary {V}; the selection takes 1 .. "
                         f"min({RNNT_STEP_MAX_K}, V - 1) (EA_RNNT_STEP_MAX_K)")


def f32c(t: torch.Tensor) -> torch.Tensor:
    """An f32 tensor with unit inner stride (lm/rnn_train.py's rule; that package imports the model,
    which imports this module)."""
    if t.dtype != torch.float32:
        raise RuntimeError("activations and gradients between the transducer's nodes are float32")
    return t if t.stride(-1) == 1 else t.contiguous()


class JointLinearFn(torch.autograd.Function):
    """A Linear of the joint network: (rows, in) f32 -> (rows, out) f32; lin = (weight Parameter, bias
    Parameter or None, the weight in the compute dtype)."""

    @staticmethod
    def forward(ctx, x, lin):
        weight, bias, w = lin
        xc = ops.cast(x, w.dtype)
        y = torch.empty(xc.shape[0], w.shape[0], device=x.device)
        ops.linear(xc, w, y, epi=ops.make_epi(bias=None if bias is None else bias.detach()))
        ctx.save = (xc, lin)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, (weight, bias, w) = ctx.save
        ctx.save = None
        dy = f32c(dy)
        dyc = ops.cast(dy, w.dtype)
        dx = torch.empty(xc.shape[0], w.shape[1], device=dy.device)
        ops.linear_dx(dyc, w, dx)
        ops.linear_dw(dyc, xc, weight.grad, accumulate=True)
        if bias is not None:
            ops.colsum(dy, bias.grad, accumulate=True)
        return dx, None


def chunk_rows(BT: int, U1: int, V: int, esize: int, cap_bytes: int) -> int:
    """(b, t) rows per backward chunk: the dlogits workspace (rows * U1 node rows of V rounded up to 8
    elements) stays under cap_bytes; one (b, t) row at the least."""
    return max(1, min(BT, cap_bytes // (U1 * rup(V) * esize)))


class RNNTJointLossFn(torch.autograd.Function):
    """(E (B, T, J), D (B, U1, J) f32, y (B, U1 - 1), t_len, u_len (B) int32 on the device) -> the
    batch-mean RNN-T loss with blank 0.  lin_out: (weight, bias, weight in the compute dtype)."""

    @staticmethod
    def forward(ctx, E, D, y, t_len, u_len, lin_out, cap_bytes):
        weight, bias, w = lin_out
        E, D = f32c(E).contiguous(), f32c(D).contiguous()
        (B, T, J), U1, V = E.shape, D.shape[1], w.shape[0]
        if J % 8 or J > RNNT_MAX_JOINT:
            raise NotImplementedError(f"joint_space_size={J}: the joint kernel keeps its tanh tile in LDS and takes "
                                      f"a multiple of 8 up to {RNNT_MAX_JOINT}")
        if U1 > RNNT_MAX_U1:
            raise NotImplementedError(f"{U1 - 1} labels: the lattice kernel holds two diagonals of at most "
                                      f"{RNNT_MAX_U1} nodes in LDS")
        if D.shape != (B, U1, J) or y.shape != (B, U1 - 1) or any(v.dtype != torch.int32 for v in (y, t_len, u_len)):
            raise ValueError(f"E {tuple(E.shape)}, D {tuple(D.shape)}, y {tuple(y.shape)} {y.dtype}")
        dev, st = E.device, ops.stream()
        keep = torch.empty(4, B, T, U1, device=dev)  # lse, gamma, kappa_blank, kappa_label
        tmp = torch.empty(2, B, T, U1, device=dev)   # lp_blank, lp_label
        ab = torch.empty(2, B, T, U1, dtype=torch.float64, device=dev)  # alpha, beta
        ll, loss = torch.empty(B, dtype=torch.float64, device=dev), torch.empty((), device=dev)
        y = y.contiguous()
        lib.ea_rnnt_joint_lse(dt(w), B, T, U1, V, J, E.data_ptr(), D.data_ptr(), w.data_ptr(), w.stride(0),
                              bias.data_ptr(), y.data_ptr(), t_len.data_ptr(), u_len.data_ptr(), keep[0].data_ptr(),
                              tmp[0].data_ptr(), tmp[1].data_ptr(), st)
        lib.ea_rnnt_lattice(B, T, U1, tmp[0].data_ptr(), tmp[1].data_ptr(), t_len.data_ptr(), u_len.data_ptr(),
                            ab[0].data_ptr(), ab[1].data_ptr(), ll.data_ptr(), keep[1].data_ptr(),
                            keep[2].data_ptr(), keep[3].data_ptr(), loss.data_ptr(), st)
        ctx.save = (E, D, y, t_len, u_len, lin_out, keep, cap_bytes)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        E, D, y, t_len, u_len, (weight, bias, w), keep, cap_bytes = ctx.save
        ctx.save = None
        g = gloss.contiguous()
        if g.dtype != torch.float32:
            raise RuntimeError("loss gradients must be float32")
        (B, T, J), U1, V = E.shape, D.shape[1], w.shape[0]
        dev, st, cd, Vp = E.device, ops.stream(), w.dtype, rup(V)
        nbt_max = chunk_rows(B * T, U1, V, w.element_size(), cap_bytes)
        dl = torch.empty(nbt_max * U1, Vp, dtype=cd, device=dev)
        h = torch.empty(nbt_max * U1, J, dtype=cd, device=dev)
        dh = torch.empty(nbt_max * U1, J, device=dev)
        dE, dD = torch.empty(B, T, J, device=dev), torch.empty(B, U1, J, device=dev)
        for bt0 in range(0, B * T, nbt_max):
            nbt = min(nbt_max, B * T - bt0)
            rows = nbt * U1
            lib.ea_rnnt_joint_dlogits(dt(w), B, T, U1, V, J, E.data_ptr(), D.data_ptr(), w.data_ptr(), w.stride(0),
                                      bias.data_ptr(), y.data_ptr(), t_len.data_ptr(), u_len.data_ptr(),
                                      keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                                      g.data_ptr(), bt0, nbt, dl.data_ptr(), Vp, h.data_ptr(), st)
            # launched here, not queued with the pass's weight gradients: the next chunk reuses dl and h
            ops.gemm(dl, w, dh, M=rows, N=J, K=V, a_kmajor=1, b_kmajor=0, lda=Vp, ldb=w.stride(0), ldc=J, splitk=False)
            ops.gemm(dl, h, weight.grad, M=V, N=J, K=rows, a_kmajor=0, b_kmajor=0, lda=Vp, ldb=J, ldc=J,
                     epi=ops.make_epi(beta=1.0), splitk=False)
            ops.colsum(dl[:rows, :V], bias.grad, accumulate=True, defer=False)
            lib.ea_rnnt_joint_dact(B, T, U1, J, E.data_ptr(), D.data_ptr(), t_len.data_ptr(), u_len.data_ptr(), bt0, nbt,
                                   dh.data_ptr(), dE.data_ptr(), dD.data_ptr(), st)
        return dE, dD, None, None, None, None, None


class RNNTLoss(torch.nn.Module):
    """warprnnt_pytorch.RNNTLoss(blank=0, fastemit_lambda=0.0, reduction="mean": the sum over the batch
    divided by the batch size), taken together with the joint network's tanh and lin_out.

    chunk_bytes caps the backward's dlogits workspace; the backward runs in chunks of whole (b, t) rows
    sized under it.  The default, 1 GiB, is a guess nobody has measured."""

    def __init__(self, blank: int = 0, fastemit_lambda: float = 0.0, reduction: str = "mean",
                 chunk_bytes: int = 1 << 30):
        super().__init__()
        if blank != 0:
            raise NotImplementedError(f"RNNTLoss blank={blank}: the kernels use blank = 0")
        if fastemit_lambda != 0.0:
            raise NotImplementedError(f"RNNTLoss fastemit_lambda={fastemit_lambda}: FastEmit is not built")
        if reduction != "mean":
            raise NotImplementedError(f"RNNTLoss reduction={reduction!r}: only 'mean'")
        self.chunk_bytes = int(chunk_bytes)

    def forward(self, joint_network, enc_out, dec_out, target, t_len, u_len):
        """enc_out (B, T, D_enc), dec_out (B, U1, D_dec) f32; target (B, U1 - 1), t_len, u_len (B) int32."""
        E, D = joint_network.project(enc_out, dec_out)
        return RNNTJointLossFn.apply(E, D, target, t_len, u_len, joint_network.lin_out_handle(), self.chunk_bytes)


class JointNetwork(torch.nn.Module):
    """espnet2/asr_transducer/joint_network.py: same constructor, attributes and state_dict keys."""

    def __init__(self, output_size: int, encoder_size: int, decoder_size: int, joint_space_size: int = 256,
                 joint_activation_type: str = "tanh", **activation_parameters):
        if joint_activation_type != "tanh":
            raise NotImplementedError(f"espnet_amd JointNetwork: joint_activation_type={joint_activation_type!r} is "
                                      "not built (only 'tanh')")
        if joint_space_size % 8 or joint_space_size > RNNT_MAX_JOINT:
            raise NotImplementedError(f"espnet_amd JointNetwork: joint_space_size={joint_space_size} is not built "
                                      f"(a multiple of 8 up to {RNNT_MAX_JOINT})")
        super().__init__()
        self.lin_enc = torch.nn.Linear(encoder_size, joint_space_size)
        self.lin_dec = torch.nn.Linear(decoder_size, joint_space_size, bias=False)
        self.lin_out = torch.nn.Linear(joint_space_size, output_size)
        self.joint_space_size = joint_space_size
        self._b = None

    def arena_groups(self, prefix=""):
        return []

    def bind(self, arena, prefix, cd):
        self._b = Bound(arena, prefix, cd)

    def _lin(self, name):
        if self._b is None:
            raise RuntimeError("JointNetwork: bind(arena, prefix, cd) first (ESPnetASRModel.prepare)")
        m = getattr(self, name)
        return m.weight, m.bias, self._b.w(f"{name}.weight")

    def lin_out_handle(self):
        return self._lin("lin_out")

    def project(self, enc_out, dec_out):
        """-> (lin_enc(enc_out) (B, T, J), lin_dec(dec_out) (B, U1, J)) f32."""
        (B, T, _), U1, J = enc_out.shape, dec_out.shape[1], self.joint_space_size
        E = JointLinearFn.apply(enc_out.reshape(B * T, -1), self._lin("lin_enc"))
        D = JointLinearFn.apply(dec_out.reshape(B * U1, -1), self._lin("lin_dec"))
        return E.view(B, T, J), D.view(B, U1, J)

    # ------------------------------------------------------------------ decoding (csrc/transducer_step.hip)
    def project_enc(self, enc_out):
        """(T, D_enc) -> E = lin_enc(enc_out) (T, J) f32: one GEMM per utterance."""
        with torch.no_grad():
            return JointLinearFn.apply(enc_out, self._lin("lin_enc"))

    def project_dec(self, dec_out):
        """(n, D_dec) -> D = lin_dec(dec_out) (n, J) f32: the few-row GEMM."""
        with torch.no_grad():
            return JointLinearFn.apply(dec_out, self._lin("lin_dec"))

    def _step_logits(self, E, frame, D):
        """Launch A: -> (the (n, V) f32 logits of row i at frame[i], the slices' (max, sum exp) pairs)."""
        _, bias, w = self._lin("lin_out")
        (n, J), V = D.shape, w.shape[0]
        if E.dim() != 2 or E.shape[1] != J or J != self.joint_space_size or frame.shape != (n,) \
                or frame.dtype != torch.int32 or not frame.is_contiguous():
            raise ValueError(f"E {tuple(E.shape)}, D {tuple(D.shape)}, frame {tuple(frame.shape)} {frame.dtype}")
        E, D = f32c(E), f32c(D)
        logits = torch.empty(n, V, device=D.device)
        part = torch.empty(2 * n * -(-V // RNNT_STEP_SW), device=D.device)
        lib.ea_rnnt_step_logits(dt(w), n, V, J, E.data_ptr(), E.stride(0), E.shape[0], frame.data_ptr(), D.data_ptr(),
                                D.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr(), logits.data_ptr(), V,
                                part.data_ptr(), ops.stream())
        return logits, part

    def step(self, E, frame, D, k, want_logp=False):
        """One joint step of n rows: row i is a hypothesis with D[i] = lin_dec(its decoder output) at frame
        frame[i] (int32, on the device) of E (rows of lin_enc outputs).  -> JointStep: lse, lp_blank (n), the
        top k of the non-blank log-probabilities (n, k) with their ids in 1 .. V-1 (descending, ties to the
        lower id) and, with want_logp, the (n, V) log-probabilities.  Two launches, nothing synchronises."""
        check_step(D.shape[0], k, self.lin_out.out_features)
        with torch.no_grad():
            logits, part = self._step_logits(E, frame, D)
            n, V = logits.shape
            packed = torch.empty(2 * n + 2 * n * k, device=D.device)  # lse | lp_blank | top values | top ids
            ids = packed[2 * n + n * k:].view(torch.int32)
            lib.ea_rnnt_step_select(n, V, k, logits.data_ptr(), V, part.data_ptr(), packed.data_ptr(),
                                    packed[n:].data_ptr(), packed[2 * n:].data_ptr(), ids.data_ptr(), int(want_logp),
                                    ops.stream())
        return JointStep(packed[:n], packed[n:2 * n], packed[2 * n:2 * n + n * k].view(n, k), ids.view(n, k),
                         logits if want_logp else None, packed)

    def forward(self, enc_out, dec_out):
        """joint_network.py:43-59 at decoding time: enc_out_t (D_enc), dec_out (D_dec) -> the (V) logits."""
        if enc_out.dim() != 1 or dec_out.dim() != 1 or torch.is_grad_enabled():
            raise NotImplementedError("espnet_amd JointNetwork: the (B, T, U, V) joint output is never built; the "
                                      "loss takes the network itself (RNNTLoss.forward); forward serves decoding: "
                                      "1-D enc_out_t and dec_out under torch.no_grad()")
        frame = torch.zeros(1, dtype=torch.int32, device=dec_out.device)
        return self._step_logits(self.project_enc(enc_out[None]), frame, self.project_dec(dec_out[None]))[0][0]
