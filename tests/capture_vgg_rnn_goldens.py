"""Capture the VGG2L + BLSTM(P) encoder fixtures from the REFERENCE implementation
(espnet2/asr/encoder/vgg_rnn_encoder.py VGGRNNEncoder over VGG2L / RNNP / RNN of
espnet/nets/pytorch_backend/rnn/encoders.py, dropout 0).  Test infrastructure: not collected by
pytest, never imported by the package.

It reuses oracle/make_goldens.py (reference import path and stubs) and the helpers of
tests/capture_rnn_encoder_goldens.py, and writes, readable by tests/vgg_rnn_goldens.py:

    vgg_rnn_tiny.npz    B 2, T 13, F 10, ilens 13 7, RNNP 2 x 8 -> 8
    vgg_rnn_noproj.npz  the same with use_projection false (RNN 2 x 8, l_last -> 8)
    vgg_rnn_f83.npz     B 2, T 9, F 83, ilens 9 5, RNNP 2 x 8 -> 8
    vgg_rnn_build.npz   no arrays but cfg: for four configurations (the defaults; use_projection
                        false; bidirectional false; the encoder_conf of
                        tests/golden/train_asr_rnn_aishell.yaml) at input_size 83 the state_dict keys,
                        shapes, the parameter count, output_size and, built under cfg.seed, the f64
                        sum of every tensor; and the parameter count of the aishell recipe's model

each of the first three with out.y, out.olens, of every parameter gradient under the cotangent a
strided sample (gsamp.*) and its f64 norm (gnorm.*), and wsum.* (weights are regenerated from
cfg.seed; inputs from tests/vgg_rnn_goldens.py make_inputs, junk in the padded frames).

Yardstick: the same module is run in float64; err.<array> is max |f32 - f64| of the reference
itself, and the tests allow MARGIN x that or MARGIN f32 ulps at the array's magnitude.

Decisions.  cfg.seed is the first seed for which, in the float64 run, no convolution output lies
within MARGIN x (that array's max |f32 - f64|) of zero and no pooling window's two largest ReLU
outputs lie that close to each other (asserted here): every ReLU and argmax decision of an f32
computation within the tolerance is then the float64 one; and for which the bf16 caps below hold.

bf16.  Decisions near a tie cannot be pinned end to end: a bf16 operand that lands on the other side
of a rounding boundary moves later pre-activations by about 1e-3.  tests/vgg_rnn_goldens.py restate
with bf=True is the float64 restatement on bf16-rounded operands with GIVEN decisions; the test
feeds it the kernels' own.  Checked here: with bf=False and its own decisions it is the reference
(float64 rounding), and fed its own decisions it returns the same arrays bit for bit.  bf.err.* is,
with the decisions held fixed at the restatement's own, the largest deviation from it of the same
restatement in f32 and of the float64 one with every rounding decision taken on operand x
(1 +- cfg.bf_nudge); cfg.bf_nudge is MARGIN x the reference's largest relative f32 error over the
recorded arrays (as for rnn_enc_*).  cfg.bands: per convolution MARGIN x the largest deviation of its
output among those runs; a kernel decision must equal the restatement's own wherever the
restatement's |pre-activation| (or top-two gap) exceeds the band.  The share of a layer's elements
(windows) inside its band is a condition on the seed, asserted here: at most 5 % per ReLU layer and
20 % per pool layer (cfg.band_shares).

vgg_rnn_tiny.npz also records hyb.*: ESPnetASRModel with this encoder, decoder: rnn and ctc_weight
0.5 built under cfg.hyb.seed (hyb.wsum.*), four steps of torch.optim.Adam(lr 1e-3) with
clip_grad_norm_(5) (hyb.loss / loss_att / loss_ctc / acc from the float64 run, err.hyb.* =
max |f32 - f64|) and the n-best hypotheses of BeamSearch (beam 3, ctc_weight 0 and 0.3).

Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_vgg_rnn_goldens.py
"""
from __future__ import annotations

import copy
import json
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402  (puts the reference and its stubs on sys.path)
from capture_rnn_encoder_goldens import (BEAM_CASES, HYB_CLIP, HYB_LR, HYB_STEPS, _err,  # noqa: E402
                                         _hybrid_steps, _save)
from vgg_rnn_goldens import (CONVS, MARGIN, bands, decision_room, encoder_kwargs, in_band, make_inputs,  # noqa: E402
                             restate)

GSAMPLE = 4096
RELU_CAP, POOL_CAP = 0.05, 0.20  # the largest share of a layer's decisions that may lie inside its band
AISHELL = "train_asr_rnn_aishell.yaml"


def _run(enc, inp, dtype):
    """Output, lengths, parameter gradients and the four convolution outputs in `dtype`."""
    enc = copy.deepcopy(enc).to(dtype)
    enc.train()
    pre = {}
    hooks = [getattr(enc.enc[0], n).register_forward_hook(lambda m, i, o, n=n: pre.__setitem__(n, o.detach()))
             for n in CONVS]
    y, olens, _ = enc(inp["xs_pad"].detach().clone().to(dtype), inp["ilens"])
    (y * inp["cot"].to(dtype)).sum().backward()
    for h in hooks:
        h.remove()
    g = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for k, p in enc.named_parameters()}
    return y.detach(), torch.as_tensor(olens).long(), g, pre


def bf16_yardstick(enc, cfg, inp, y, y64, g, g64):
    """The bf16 yardstick of one candidate seed (module docstring, "bf16").
    -> (record entries, cfg entries, largest in-band share of a ReLU layer, of a pool layer)."""
    sd = enc.state_dict()
    by, _, bg, bpre, D0 = restate(sd, cfg, inp, torch.float64, bf=True)
    # feeding the restatement its own decisions changes nothing
    sy, _, sg, _, _ = restate(sd, cfg, inp, torch.float64, bf=True, decisions=D0)
    assert torch.equal(sy, by) and all(torch.equal(sg[k], bg[k]) for k in bg)
    rel = max([float(_err(y, y64)) / float(y64.abs().max())]
              + [float(_err(g[k], g64[k])) / float(g64[k].abs().max()) for k in g64 if float(g64[k].abs().max()) > 0])
    nudge = MARGIN * rel
    alts = [restate(sd, cfg, inp, torch.float32, bf=True, decisions=D0)]
    alts += [restate(sd, cfg, inp, torch.float64, bf=True, decisions=D0, nudge=s * nudge) for s in (1.0, -1.0)]
    rec = {"bf.err.y": np.array(max(float(_err(a[0], by)) for a in alts))}
    for k in bg:
        rec[f"bf.err.grad.{k}"] = np.array(max(float(_err(a[2][k], bg[k])) for a in alts))
    band = bands(bpre, [a[3] for a in alts])
    relu_in, pool_in = in_band(bpre, band)
    shares = {f"relu{i}": float(m.double().mean()) for i, m in relu_in.items()}
    shares.update({f"pool{j}": float(m.double().mean()) for j, m in pool_in.items()})
    return (rec, dict(bf_nudge=nudge, bands=band, band_shares=shares),
            max(shares[f"relu{i}"] for i in range(4)), max(shares[f"pool{j}"] for j in range(2)))


def capture(name, cfg):
    from espnet2.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
    ok = False
    for seed in range(64):
        cfg = dict(cfg, seed=seed)
        torch.manual_seed(seed)
        enc = VGGRNNEncoder(**encoder_kwargs(cfg))
        inp = make_inputs(cfg)
        y, olens, g, pre = _run(enc, inp, torch.float32)
        y64, olens64, g64, pre64 = _run(enc, inp, torch.float64)
        room = decision_room(pre, pre64)
        if room <= 1.0:
            continue
        bf_rec, bf_cfg, relu_share, pool_share = bf16_yardstick(enc, cfg, inp, y, y64, g, g64)
        if relu_share <= RELU_CAP and pool_share <= POOL_CAP:
            ok = True
            break
    assert ok and room > 1.0, "no seed clears the decision guard and the in-band caps"
    assert relu_share <= RELU_CAP and pool_share <= POOL_CAP
    assert torch.equal(olens, olens64)
    # the restatement (tests/vgg_rnn_goldens.py restate) with bf=False and its own decisions is the
    # reference's module: within float64 rounding
    ry, rl, rg, _, _ = restate(enc.state_dict(), cfg, inp, torch.float64)
    assert ry.shape == y64.shape and torch.equal(rl, olens64) and float((ry - y64).abs().max()) < 1e-12
    for k in g64:
        assert float((rg[k] - g64[k]).abs().max()) <= 1e-10 * max(1.0, float(g64[k].abs().max())), k
    rec = {f"wsum.{k}": np.array(v.double().sum().item()) for k, v in enc.state_dict().items()}
    rec["out.y"], rec["err.y"], rec["out.olens"] = mg.np32(y), _err(y, y64), olens.numpy()
    rec.update(bf_rec)
    gstride = {}
    for k in g:
        s = max(1, -(-g[k].numel() // GSAMPLE))
        while s > 1 and math.gcd(s, 6) != 1:  # coprime to the 9 taps and to the channel counts: the
            s += 1                            # sample walks through every tap and every channel
        gstride[k] = s
        rec[f"err.grad.{k}"] = _err(g[k], g64[k])
        rec[f"gsamp.{k}"] = mg.np32(g[k].reshape(-1)[::s])
        rec[f"gnorm.{k}"] = np.array(float(g64[k].norm()))
    cfg = dict(cfg, margin=MARGIN, gstride=gstride, guard_room=room, **bf_cfg)
    if name == "vgg_rnn_tiny":
        cfg["hyb"] = hybrid(rec, cfg)
    rec["cfg"] = np.array(json.dumps(cfg))
    print(f"{name}: seed {cfg['seed']} (guard room {room:.2f}), y err {float(rec['err.y']):.1e} (bf16 "
          f"{float(rec['bf.err.y']):.1e}), worst grad err {max(float(rec[f'err.grad.{k}']) for k in g):.1e} (bf16 "
          f"{max(float(rec[f'bf.err.grad.{k}']) for k in g):.1e}), in-band shares relu {relu_share:.3f} pool "
          f"{pool_share:.3f}, {_save(name, rec)} bytes")


def _hybrid_model(hcfg):
    from espnet2.asr.ctc import CTC
    from espnet2.asr.decoder.rnn_decoder import RNNDecoder
    from espnet2.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
    from espnet2.asr.espnet_model import ESPnetASRModel
    from espnet2.layers.utterance_mvn import UtteranceMVN
    V = hcfg["vocab_size"]
    encoder = VGGRNNEncoder(input_size=hcfg["input_size"], **hcfg["encoder_conf"])
    decoder = RNNDecoder(vocab_size=V, encoder_output_size=encoder.output_size(), **hcfg["decoder_conf"])
    ctc = CTC(odim=V, encoder_output_size=encoder.output_size())
    return ESPnetASRModel(vocab_size=V, token_list=mg.token_list(V), frontend=None, specaug=None,
                          normalize=UtteranceMVN(), preencoder=None, encoder=encoder, postencoder=None,
                          decoder=decoder, ctc=ctc, joint_network=None, **hcfg["model_conf"])


def hybrid(rec, cfg):
    from espnet.nets.beam_search import BeamSearch
    from espnet.nets.scorers.ctc import CTCPrefixScorer
    from espnet.nets.scorers.length_bonus import LengthBonus
    kw = encoder_kwargs(cfg)
    kw.pop("input_size")
    hcfg = dict(seed=7, input_size=cfg["F"], vocab_size=11, encoder_conf=kw,
                decoder_conf=dict(rnn_type="lstm", num_layers=1, hidden_size=16,
                                  att_conf=dict(adim=14, aconv_chans=3, aconv_filts=5)),
                model_conf=dict(ctc_weight=0.5, lsm_weight=0.0, length_normalized_loss=False),
                speech_lengths=[36, 25, 13], text_lengths=[4, 3, 2],
                steps=HYB_STEPS, lr=HYB_LR, grad_clip=HYB_CLIP, beam_cases=BEAM_CASES)
    torch.manual_seed(hcfg["seed"])
    model = _hybrid_model(hcfg)
    rec.update({f"hyb.wsum.{k}": np.array(v.double().sum().item()) for k, v in model.state_dict().items()})
    batch = mg.make_batch(hcfg, torch.Generator().manual_seed(21))
    rec.update({f"hyb.in.{k}": v.numpy() for k, v in batch.items()})
    s32, s64 = _hybrid_steps(model, batch, torch.float32), _hybrid_steps(model, batch, torch.float64)
    for k in s64:
        rec[f"hyb.{k}"], rec[f"err.hyb.{k}"] = s64[k].numpy(), _err(s32[k], s64[k])
    model.eval()
    V = model.vocab_size
    nbest_meta = []
    with torch.no_grad():
        for ci, (beam, cw) in enumerate(BEAM_CASES):
            bs = BeamSearch(scorers={"decoder": model.decoder, "ctc": CTCPrefixScorer(model.ctc, model.eos),
                                     "length_bonus": LengthBonus(V)},
                            weights={"decoder": 1.0 - cw, "ctc": cw, "length_bonus": 0.0}, beam_size=beam,
                            vocab_size=V, sos=model.sos, eos=model.eos, token_list=None, pre_beam_score_key="full")
            for u in range(batch["speech"].shape[0]):
                le = int(batch["speech_lengths"][u])
                enc, _ = model.encode(batch["speech"][u:u + 1, :le], batch["speech_lengths"][u:u + 1])
                nbest = bs(x=enc[0], maxlenratio=0.0, minlenratio=0.0)
                for r, h in enumerate(nbest):
                    rec[f"hyb.beam.c{ci}.u{u}.h{r}.yseq"] = h.yseq.numpy().astype(np.int64)
                    rec[f"hyb.beam.c{ci}.u{u}.h{r}.score"] = np.float64(float(h.score))
                nbest_meta.append({"case": ci, "utt": u, "n": len(nbest)})
    hcfg["nbest"] = nbest_meta
    print(f"hybrid: losses {s64['loss'].tolist()} (f32-f64 {float(rec['err.hyb.loss']):.1e})")
    return hcfg


def capture_build(name="vgg_rnn_build", seed=11, input_size=83):
    from espnet2.asr.encoder.vgg_rnn_encoder import VGGRNNEncoder
    with open(os.path.join(mg.OUT, AISHELL)) as f:
        recipe = yaml.safe_load(f)
    confs = {"defaults": {}, "noproj": dict(use_projection=False), "uni": dict(bidirectional=False),
             "aishell": recipe["encoder_conf"]}
    out = {}
    for key, conf in confs.items():
        torch.manual_seed(seed)
        enc = VGGRNNEncoder(input_size=input_size, **conf)
        sd = enc.state_dict()
        out[key] = dict(conf=conf, keys=list(sd), shapes=[list(v.shape) for v in sd.values()],
                        nparams=sum(p.numel() for p in enc.parameters()),
                        wsum=[v.double().sum().item() for v in sd.values()], output_size=enc.output_size())
    V = 50
    model = _hybrid_model(dict(vocab_size=V, input_size=input_size, encoder_conf=recipe["encoder_conf"],
                               decoder_conf=recipe["decoder_conf"], model_conf=recipe["model_conf"]))
    cfg = dict(seed=seed, input_size=input_size, aishell_yaml=AISHELL, confs=out, recipe_vocab=V,
               recipe_nparams=sum(p.numel() for p in model.parameters()))
    rec = {"cfg": np.array(json.dumps(cfg))}
    print(f"{name}: {[(k, v['nparams']) for k, v in out.items()]}, recipe {cfg['recipe_nparams']}, "
          f"{_save(name, rec)} bytes")


if __name__ == "__main__":
    base = dict(F=10, H=8, proj=8, layers=2, bidirectional=True, use_projection=True, ilens=[13, 7])
    capture("vgg_rnn_tiny", base)
    capture("vgg_rnn_noproj", dict(base, use_projection=False))
    capture("vgg_rnn_f83", dict(base, F=83, ilens=[9, 5]))
    capture_build()
