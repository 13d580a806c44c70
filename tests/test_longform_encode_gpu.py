"""Past 2048 subsampled frames in f32 (head dim 8): encode() of one-block Conformers (rel_pos_type latest
and legacy) and a Transformer encoder at T' = 2049 (B = 2, the second utterance shorter), and the decoder's
scoring over a 2049-frame memory, against the float64 oracle on the same weights; the legacy Conformer is
the oracle's with its attention replaced by the restatement below.  Before csrc/attn_stream.hip each of
these failed in ea_attn_softmax_fwd (bad argument).  Tolerance: atol = rtol = 1e-4, the fp32 bound of
encoder outputs and logits in tests/test_model_gpu.py.  A training forward at this length is refused by name."""
import numpy as np
import pytest
import torch

from goldens import perturb_norms
from legacy_relpos_goldens import legacy_shift
from test_model_build import build

pytestmark = pytest.mark.gpu
T, F, D, HEADS, V = 8199, 20, 32, 4, 20  # ((T - 1) // 2 - 1) // 2 = 2049
ZERO = dict(dropout_rate=0.0, positional_dropout_rate=0.0)
DEC = dict(attention_heads=HEADS, linear_units=64, num_blocks=1, self_attention_dropout_rate=0.0,
           src_attention_dropout_rate=0.0, **ZERO)
CONFORMER = dict(macaron_style=True, pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn",
                 activation_type="swish", use_cnn_module=True, cnn_module_kernel=15)


def _models(kind):
    from oracle.asr_oracle import OracleASR
    enc = dict(output_size=D, attention_heads=HEADS, linear_units=64, num_blocks=1, attention_dropout_rate=0.0,
               input_layer="conv2d", normalize_before=True, **ZERO)
    if kind != "transformer":
        enc.update(CONFORMER, rel_pos_type=kind)
    cfg = dict(encoder="transformer" if kind == "transformer" else "conformer", input_size=F, vocab_size=V,
               encoder_conf=enc, decoder="transformer", decoder_conf=DEC,
               model_conf=dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False))
    torch.manual_seed(5)
    m = build(cfg)
    perturb_norms(m, torch.Generator().manual_seed(6))
    ora = OracleASR(cfg, {k: v.clone() for k, v in m.state_dict().items()}, dtype=torch.float64)
    return m.prepare("cuda", amp=False), ora


def _legacy_rel_mha(P, name, x, pos_emb, mask, h, p_drop, training):
    """attention.py:114-206 over the first T' rows of the reversed 5000-row table (embedding.py:220-257)."""
    from espnet_amd.layers.subsampling import legacy_rel_pos_table
    from oracle import asr_oracle as O
    B, Tp, d = x.shape
    q = O.linear(P, name + ".linear_q", x).view(B, Tp, h, d // h)
    k, v = (O.split_heads(O.linear(P, name + n, x), h) for n in (".linear_k", ".linear_v"))
    pos = legacy_rel_pos_table(5000, d)[:Tp].to(x.dtype)
    p = O.linear(P, name + ".linear_pos", pos, bias=False).view(1, Tp, h, d // h).transpose(1, 2)
    qu, qv = ((q + P[name + b]).transpose(1, 2) for b in (".pos_bias_u", ".pos_bias_v"))
    o = O.mha_core(qu, k, v, legacy_shift(qv @ p.transpose(-2, -1)), mask, 0.0, False, d // h)
    return O.linear(P, name + ".linear_out", O.merge_heads(o))


@pytest.mark.parametrize("kind", ["latest", "legacy", "transformer"])
def test_encode_2049_frames_matches_f64_oracle(kind, monkeypatch):
    from oracle import asr_oracle as O
    m, ora = _models(kind)
    speech, lens = torch.randn(2, T, F, generator=torch.Generator().manual_seed(9)), torch.tensor([T, 4999])
    m.eval()
    with torch.no_grad():
        enc, olens = m.encode(speech, lens)
        feats = O.utterance_mvn(speech.double(), lens)
        if kind == "transformer":
            ref, rlens = O.transformer_encoder(ora.params, feats, lens, ora.cfg["encoder_conf"], False)
        else:
            if kind == "legacy":
                monkeypatch.setattr(O, "rel_mha", _legacy_rel_mha)
            ref, rlens = O.conformer_encoder(ora.params, feats, lens, ora.cfg["encoder_conf"], ora.bufs, False)
    assert olens.cpu().tolist() == rlens.tolist() == [2049, 1250]
    print(f"{kind}: encode() at T' = 2049, max |err| vs float64 {float((enc.cpu().double() - ref).abs().max()):.3g}")
    np.testing.assert_allclose(enc.cpu().numpy(), ref.numpy(), atol=1e-4, rtol=1e-4)
    m.train()  # the same forward with a graph to build: refused, with the limit named
    with pytest.raises(NotImplementedError, match="2048 keys.*inference is served"):
        m(speech, lens, torch.randint(1, V - 1, (2, 3)), torch.tensor([3, 2]))


def test_decoder_steps_over_a_2049_frame_memory_match_f64_oracle():
    """batch_score from <sos> (captured steps) and forward_one_step on the prefix (the eager step)."""
    from oracle import asr_oracle as O
    m, ora = _models("transformer")
    g = torch.Generator().manual_seed(3)
    mem, ys = torch.randn(2, 2049, D, generator=g), torch.randint(1, V - 1, (2, 3), generator=g)
    ys[:, 0] = m.sos
    m.eval()
    with torch.no_grad():
        states = [None, None]
        for L in (1, 2, 3):
            logp, states = m.decoder.batch_score(ys[:, :L].cuda(), states, mem.cuda())
        eager, _ = m.decoder.forward_one_step(ys.cuda(), None, mem.cuda())
        logits = O.transformer_decoder(ora.params, mem.double(), torch.tensor([2049, 2049]), ys, torch.tensor([3, 3]),
                                       ora.cfg["decoder_conf"], False)
    ref = torch.log_softmax(logits[:, -1], -1)
    for what, got in (("batch_score", logp), ("forward_one_step", eager)):
        print(f"{what}: max |err| vs float64 {float((got.cpu().double() - ref).abs().max()):.3g}")
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=1e-4, rtol=1e-4)
