"""Sublayers shared by the encoder blocks: the position-wise feed-forward sublayer (Conformer,
E-Branchformer and Transformer blocks) and the rel-pos multi-head attention core (Conformer and
E-Branchformer blocks).

Plain functions called from inside a block's autograd Function: the forward half launches the
sublayer's HIP kernels and returns what its backward half needs; the backward half writes the
parameter gradients into the arena.  `b` is the block's `Bound`; parameters are named relative
to it (`pre` / `A` select the holder).  A block's kernel launch order is the order of these calls.
"""
from __future__ import annotations

from .common import (EPI_ACT, EPI_DACT, EPI_RESID, REL_LEGACY, attn_bwd, attn_dmask, attn_fused_bwd, attn_fwd,
                     dbd_layout, empty, fused_attn_ok, lib, ln_bwd, ln_fwd, math, ops, rup, site_dv)


# ----------------------------------------------------------------------------- feed-forward
def ffn_fwd(b, x_in, pre, ln_name, *, act, p_in, p_out, rscale, seed_in, seed_out):
    """x_in + rscale * dropout(w_2(dropout(act(w_1(ln(x_in)))))) on the f32 residual stream
    (positionwise_feed_forward.py:22-32 inside a pre-norm residual).  p_in / seed_in: the dropout
    behind the activation; p_out / seed_out: the sublayer's output dropout."""
    cd = b.cd
    N, d = x_in.shape
    w1 = b.w(pre + ".w_1.weight")
    Fh = w1.shape[0]
    xn, mu, rs = ln_fwd(x_in, b, ln_name, cd)
    h = empty(N, Fh, dtype=cd, device=x_in.device)
    a = empty(N, Fh, dtype=cd, device=x_in.device)
    ops.linear(xn, w1, a,
               epi=ops.make_epi(EPI_ACT, bias=b.f(pre + ".w_1.bias"), act=act, aux=h,
                                drop_p=p_in, seed=seed_in))
    x_out = empty(N, d, device=x_in.device)
    ops.linear(a, b.w(pre + ".w_2.weight"), x_out,
               epi=ops.make_epi(EPI_RESID, bias=b.f(pre + ".w_2.bias"), resid=x_in,
                                rscale=rscale, drop_p=p_out, seed=seed_out))
    return x_out, (xn, mu, rs, h, a)


def ffn_bwd(b, dx, x_in, saved, pre, ln_name, *, act, p_in, p_out, rscale, seed_in, seed_out,
            dv_in=None, next_drop=None):
    """dx: f32 (N,d) grad of the sub-block output; updated in place to grad of x_in.  dv_in: this
    site's dv when already written; next_drop: the following site's (dv, scale, p, seed) for the
    LayerNorm backward to write."""
    cd = b.cd
    xn, mu, rs, h, a = saved
    N, d = dx.shape
    dv = site_dv(dx, dv_in, b.g(pre + ".w_2.bias"), rscale, p_out, seed_out, cd)
    with ops.wgrad(dv, a):
        ops.linear_dw(dv, a, b.g(pre + ".w_2.weight"), accumulate=True)
    dh = empty(*h.shape, dtype=cd, device=dx.device)
    ops.linear_dx(dv, b.w(pre + ".w_2.weight"), dh,
                  epi=ops.make_epi(EPI_DACT, act=act, aux=h, drop_p=p_in, seed=seed_in))
    with ops.wgrad(dh, xn):
        ops.linear_dw(dh, xn, b.g(pre + ".w_1.weight"), accumulate=True,
                      db=b.g(pre + ".w_1.bias"))
    dxn = empty(N, d, dtype=cd, device=dx.device)
    ops.linear_dx(dh, b.w(pre + ".w_1.weight"), dxn)
    ln_bwd(dxn, x_in, b, ln_name, mu, rs, dx, accumulate=True, drop=next_drop)


# ----------------------------------------------------------------------------- rel-pos attention
def rel_attn_fwd(b, A, xn, pos, olens, *, B, T, H, rel_mode, pa, seed):
    """Rel-pos MHSA core (attention.py:262-305; REL_LEGACY: attention.py:114-206) on the parameters
    under prefix `A`: xn (N, d) cd -> O (N, d) cd, before linear_out.  pa / seed: the dropout on
    the attention probabilities."""
    cd = b.cd
    N, d = xn.shape
    dev = xn.device
    dk = d // H
    P2 = 2 * T - 1
    qkv = empty(N, 3 * d, dtype=cd, device=dev)
    ops.linear(xn, b.w(A + "linear_q.weight", A + "linear_k.weight", A + "linear_v.weight",
                       shape=(3 * d, d)), qkv,
               epi=ops.make_epi(bias=b.f(A + "linear_q.bias", A + "linear_k.bias",
                                         A + "linear_v.bias", shape=(3 * d,))))
    fused = fused_attn_ok(cd, dk, T, T)
    if rel_mode == REL_LEGACY and fused:
        # the fused backward's d(q+v) GEMM runs over every physical column of the shifted band
        # layout: `shift` zero rows in front of the table
        shift = dbd_layout(T)[0]
        pp_full = empty(shift + P2, d, dtype=cd, device=dev)
        pp_full[:shift].zero_()
        pp = pp_full[shift:]
    else:
        pp_full = None
        pp = empty(P2, d, dtype=cd, device=dev)
    if rel_mode == REL_LEGACY:
        # pos has T rows; the band is taken against Pext = [p; 0; p[:T-2]] (2T-1 rows)
        assert pos.shape[0] == T
        pT = empty(T, d, dtype=cd, device=dev)
        ops.linear(pos, b.w(A + "linear_pos.weight"), pT)
        lib.ea_legacy_pext(T, d, pT.data_ptr(), d, pp.data_ptr(), d, ops.dt(pp), ops.stream())
    else:
        ops.linear(pos, b.w(A + "linear_pos.weight"), pp)
    scale = 1.0 / math.sqrt(dk)
    if fused:
        # one kernel: (q+u)k^T + rel_shift((q+v)p^T), mask, softmax, dropout, @v
        O = empty(N, d, dtype=cd, device=dev)
        lse = empty(B * H * T, device=dev)
        dmask, ldm = attn_dmask(B * H * T, T, pa, dev)
        lib.ea_attn_fused_fwd2_mode(B, H, T, T, dk, qkv.data_ptr(), 3 * d, qkv[:, d:].data_ptr(), 3 * d,
                                    qkv[:, 2 * d:].data_ptr(), 3 * d, b.f(A + "pos_bias_u").data_ptr(),
                                    b.f(A + "pos_bias_v").data_ptr(), pp.data_ptr(), d, olens.data_ptr(), 0,
                                    scale, float(pa), seed, O.data_ptr(), d, lse.data_ptr(), ops.ptr(dmask), ldm,
                                    rel_mode, ops.stream())
        ldT = 0
        s_core = ("fused", lse, dmask, ldm, pp_full)
    else:
        qu = empty(N, d, dtype=cd, device=dev)
        qv = empty(N, d, dtype=cd, device=dev)
        lib.ea_add_pos_bias(N, H, dk, qkv.data_ptr(), 3 * d, b.f(A + "pos_bias_u").data_ptr(),
                            b.f(A + "pos_bias_v").data_ptr(), qu.data_ptr(), qv.data_ptr(),
                            ops.dt(qu), ops.stream())
        ldbd = rup(P2, 8)
        bd = empty(H * B * T * ldbd, device=dev)
        ops.gemm(qv, pp, bd, M=T, N=P2, K=dk, a_kmajor=1, b_kmajor=1, lda=d, ldb=d, ldc=ldbd,
                 batch=B, nh=H, sA=(T * d, dk), sB=(0, dk), sC=(T * ldbd, B * T * ldbd), splitk=False)
        O, P, Pd, ldT = attn_fwd(qu, qkv[:, d:], qkv[:, 2 * d:], B=B, H=H, T1=T, T2=T, dk=dk,
                                 ldq=d, ldk=3 * d, ldv=3 * d, klen=olens, causal=False, scale=scale,
                                 p=pa, seed=seed, cd=cd, bd=bd, ldbd=ldbd, rel_mode=rel_mode)
        del bd
        s_core = ("unfused", qu, qv, P, Pd)
    return O, (qkv, pp, s_core, scale, ldT)


def rel_attn_bwd(b, A, dO, xn, O, saved, pos, olens, *, B, T, H, rel_mode, pa, seed):
    """Backward of rel_attn_fwd: parameter gradients of linear_q/k/v, linear_pos, pos_bias_u/v into
    the arena; returns dxn (N, d) cd."""
    cd = b.cd
    N, d = xn.shape
    dev = dO.device
    dk = d // H
    P2 = 2 * T - 1
    qkv, pp, s_core, scale, ldT = saved
    legacy = rel_mode == REL_LEGACY
    dqkv = empty(N, 3 * d, dtype=cd, device=dev)
    ldbd, shift = rup(P2, 8), 0
    if s_core[0] == "fused":
        # dbd rows written in full, in the pipelined dQ pass's shifted layout (logical column r
        # at r + shift); pos_bias_u / pos_bias_v gradients from per-block column sums of the dq
        # terms.  Latest: dq includes the q+v path (dBD.p, in-kernel).  Legacy: the passes
        # recompute the legacy scores and emit the band with the latest placement,
        # ea_attn_legacy_band moves it onto the legacy rows, and d(q+v) is one batched GEMM
        # over that band (the form of the unfused path below)
        _, lse, dmask, ldm, pp_full = s_core
        shift, ldbd = dbd_layout(T)
        dbd = empty(H * B * T * ldbd, dtype=cd, device=dev)
        qv = empty(N, d, dtype=cd, device=dev)  # q + v, for the linear_pos weight gradient
        nqb = (T + 63) // 64
        part = empty(2 * B * nqb * d, device=dev)
        attn_fused_bwd(B=B, H=H, T1=T, T2=T, q=qkv, ldq=3 * d, k=qkv[:, d:], ldk=3 * d, v=qkv[:, 2 * d:],
                       ldv=3 * d, bu=b.f(A + "pos_bias_u"), bv=b.f(A + "pos_bias_v"), pp=pp, ldp=d,
                       klen=olens, causal=False, scale=scale, p=pa, seed=seed, O=O, ldo=d, lse=lse, dO=dO,
                       lddo=d, dq=dqkv, lddq=3 * d, dk=dqkv[:, d:], lddk=3 * d, dv=dqkv[:, 2 * d:],
                       lddv=3 * d, dbd=dbd, ldbd=ldbd, part=part, ldpart=d, qv_out=qv, ldqv=d, dmask=dmask,
                       ldm=ldm, flags=2 if legacy else 1 | 2, rel_mode=rel_mode)
        ops.reduce_rows(part[:B * nqb * d], B * nqb, d, d, b.g(A + "pos_bias_u", shape=(d,)))
        if legacy:
            raw = dbd
            dbd = empty(H * B * T * ldbd, dtype=cd, device=dev)
            lib.ea_attn_legacy_band(H * B, T, raw.data_ptr(), dbd.data_ptr(), ldbd, ops.stream())
            del raw
            dqv = empty(N, d, dtype=cd, device=dev)
            ops.gemm(dbd, pp_full, dqv, M=T, N=dk, K=shift + P2, a_kmajor=1, b_kmajor=0, lda=ldbd, ldb=d, ldc=d,
                     batch=B, nh=H, sA=(T * ldbd, B * T * ldbd), sB=(0, dk), sC=(T * d, dk), splitk=False)
            ops.colsum(dqv, b.g(A + "pos_bias_v", shape=(d,)))
            lib.ea_add_2d(N, d, dqv.data_ptr(), ops.dt(dqv), d, dqkv.data_ptr(), ops.dt(dqkv), 3 * d, 1.0,
                          ops.stream())
        else:
            ops.reduce_rows(part[B * nqb * d:], B * nqb, d, d, b.g(A + "pos_bias_v", shape=(d,)))
    else:
        _, qu, qv, P, Pd = s_core
        dbd = empty(H * B * T * ldbd, dtype=cd, device=dev)
        attn_bwd(dO, qu, qkv[:, d:], qkv[:, 2 * d:], P, Pd, ldT, B=B, H=H, T1=T, T2=T, dk=dk,
                 ldq=d, ldk=3 * d, ldv=3 * d, scale=scale, p=pa, seed=seed, cd=cd,
                 dq=dqkv, lddq=3 * d, dk_=dqkv[:, d:], lddk=3 * d, dv=dqkv[:, 2 * d:], lddv=3 * d,
                 dbd=dbd, ldbd=ldbd, rel_mode=rel_mode)
        # q_u = q + u: du = sum dq_u ; q_v = q + v path: dq_v = dBD . p_h, dv_bias = sum dq_v
        dqv = empty(N, d, dtype=cd, device=dev)
        ops.gemm(dbd, pp, dqv, M=T, N=dk, K=P2, a_kmajor=1, b_kmajor=0, lda=ldbd, ldb=d, ldc=d,
                 batch=B, nh=H, sA=(T * ldbd, B * T * ldbd), sB=(0, dk), sC=(T * d, dk), splitk=False)
        # not deferred: dqkv[:, :d] receives dqv in place right below
        ops.colsum(dqkv[:, :d], b.g(A + "pos_bias_u", shape=(d,)), defer=False)
        ops.colsum(dqv, b.g(A + "pos_bias_v", shape=(d,)))
        lib.ea_add_2d(N, d, dqv.data_ptr(), ops.dt(dqv), d, dqkv.data_ptr(), ops.dt(dqkv), 3 * d, 1.0,
                      ops.stream())
    qkv_w = b.w(A + "linear_q.weight", A + "linear_k.weight", A + "linear_v.weight", shape=(3 * d, d))
    # linear_pos: dp[h] = sum_b dBD[h][b]^T qv[b, :, h]  (K = B*T), dWpos = dp^T pos; with the
    # shifted layout the GEMM runs over every physical column and rows [shift, shift + P2) of
    # its output are dp

    def dpp_wgrad(after=None):
        with ops.wgrad(dbd, qv, pos, after=after, launches=True):
            Mp = P2 + shift if shift else P2
            dpp_full = empty(Mp, d, dtype=cd, device=dev)
            ops.gemm(dbd, qv, dpp_full, M=Mp, N=dk, K=B * T, a_kmajor=0, b_kmajor=0, lda=ldbd, ldb=d, ldc=d,
                     batch=1, nh=H, sA=(0, B * T * ldbd), sB=(0, dk), sC=(0, dk))
            dpp = dpp_full[shift:]
            if legacy:  # dp[k] = dPext[k] + dPext[T+1+k] over pos's T rows
                dpp = empty(T, d, dtype=cd, device=dev)
                lib.ea_legacy_pext_fold(T, d, dpp_full[shift:].data_ptr(), d, dpp.data_ptr(), d, ops.dt(dpp),
                                        ops.stream())
            ops.linear_dw(dpp, pos, b.g(A + "linear_pos.weight"), accumulate=True)

    fork = ops.fork_event()
    if fork is None:
        dpp_wgrad()
    with ops.wgrad(dqkv, xn):
        ops.linear_dw(dqkv, xn, b.g(A + "linear_q.weight", A + "linear_k.weight", A + "linear_v.weight",
                                    shape=(3 * d, d)), accumulate=True,
                      db=b.g(A + "linear_q.bias", A + "linear_k.bias", A + "linear_v.bias", shape=(3 * d,)))
    dxn = empty(N, d, dtype=cd, device=dev)
    ops.linear_dx(dqkv, qkv_w, dxn)
    if fork is not None:  # the side GEMM issued after the main chain's next kernel (fork_event)
        dpp_wgrad(after=fork)
    return dxn
