"""Transducer decoding on the GPU: BeamSearchTransducer (greedy, default beam search) and transducer_decode
over TransducerDecoder + JointNetwork against a restatement of the reference's two searches
(espnet2/asr/transducer/beam_search_transducer.py:221-354) in plain torch on the same weights, run in float64
(the reference) and in float32 (its own error: the tolerance rule of tests/lstm_train_goldens.py, margin 4).
bf16 rounds what the kernels round: every product's operands (rd of tests/test_rnnt_kernels_gpu.py).  lin_out
is scaled up and the blank bias set so that the greedy search both emits and skips (asserted)."""
import functools

import pytest
import torch

from lstm_train_goldens import tolerance
from test_rnnt_kernels_gpu import DT, rd

pytestmark = pytest.mark.gpu
V, ENC, H, J, T, MARGIN = 23, 24, 32, 40, 12, 4
OUT_SCALE, BLANK_BIAS = 8.0, 3.0
MODES = {"greedy": (1, 1, True), "beam3": (3, 3, True), "beam3_nonorm": (3, 3, False)}  # beam, nbest, score_norm


@functools.lru_cache(maxsize=None)
def weights(layers):
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.joint_network import JointNetwork
    torch.manual_seed(11 + layers)
    pair = torch.nn.Module()
    pair.decoder = TransducerDecoder(V, num_layers=layers, hidden_size=H)
    pair.joint_network = JointNetwork(V, ENC, H, joint_space_size=J)
    with torch.no_grad():
        pair.joint_network.lin_out.weight.mul_(OUT_SCALE)
        pair.joint_network.lin_out.bias[0] = BLANK_BIAS
    sd = {k: v.detach().clone() for k, v in pair.state_dict().items()}
    return sd, torch.randn(3, T, ENC, generator=torch.Generator().manual_seed(7))


@functools.lru_cache(maxsize=None)
def gpu_pair(layers, cd):
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.joint_network import JointNetwork
    pair = torch.nn.Module()
    pair.decoder = TransducerDecoder(V, num_layers=layers, hidden_size=H)
    pair.joint_network = JointNetwork(V, ENC, H, joint_space_size=J)
    pair.load_state_dict(weights(layers)[0])
    arena = ParamArena(pair, "cuda", [], shadow_dtype=None if DT[cd] == torch.float32 else DT[cd])
    pair.decoder.bind(arena, "decoder.", DT[cd])
    pair.joint_network.bind(arena, "joint_network.", DT[cd])
    pair.use_transducer_decoder, pair.encode = True, lambda speech, lens: (speech, lens)  # the encoder: identity
    return pair.eval()


@functools.lru_cache(maxsize=None)
def restate(layers, amp, dtype, mode):
    """-> [(yseq with the leading blank, score)]: the reference's searches over enc_out[0]."""
    beam, nbest, score_norm = MODES[mode]
    sd, enc = weights(layers)
    p = {k: v.to(dtype) for k, v in sd.items()}
    mm = lambda x, w: rd(x, amp) @ rd(p[w], amp).t()  # noqa: E731
    E = mm(enc[0].to(dtype), "joint_network.lin_enc.weight") + p["joint_network.lin_enc.bias"]
    cache = {}

    def score(yseq, state):  # decoder.score: (dec_out, the new state) per label sequence
        if tuple(yseq) not in cache:
            x, hs, cs = p["decoder.embed.weight"][yseq[-1]], [], []
            for k in range(layers):
                q = f"decoder.decoder.{k}."
                g = mm(x, q + "weight_ih_l0") + mm(state[0][k], q + "weight_hh_l0") + p[q + "bias_ih_l0"] + p[q + "bias_hh_l0"]
                gi, gf, gg, go = g.chunk(4)
                c = torch.sigmoid(gf) * state[1][k] + torch.sigmoid(gi) * torch.tanh(gg)
                x = torch.sigmoid(go) * torch.tanh(c)
                hs.append(x)
                cs.append(c)
            cache[tuple(yseq)] = (x, (hs, cs))
        return cache[tuple(yseq)]

    def logp(e, dec_out):
        hj = torch.tanh(e + mm(dec_out, "joint_network.lin_dec.weight"))
        return torch.log_softmax(mm(hj, "joint_network.lin_out.weight") + p["joint_network.lin_out.bias"], dim=-1)

    zero = ([torch.zeros(H, dtype=dtype)] * layers,) * 2
    if beam <= 1:
        yseq, total, state = [0], 0.0, zero
        dec_out, new = score(yseq, state)
        for e in E:
            top, pred = torch.max(logp(e, dec_out), dim=-1)
            if pred != 0:
                yseq.append(int(pred))
                total += float(top)
                state = new
                dec_out, new = score(yseq, state)
        return [(yseq, total)]
    kept = [(0.0, [0], zero)]
    for e in E:
        hyps, kept = kept, []
        while True:
            mx = hyps.pop(max(range(len(hyps)), key=lambda i: hyps[i][0]))
            dec_out, new = score(mx[1], mx[2])
            lp = logp(e, dec_out)
            kept.append((mx[0] + float(lp[0]), mx[1], mx[2]))
            for v, i in zip(*lp[1:].topk(min(beam, V - 1))):
                hyps.append((mx[0] + float(v), mx[1] + [int(i) + 1], new))
            hyps_max = max(h[0] for h in hyps)
            best = sorted([h for h in kept if h[0] > hyps_max], key=lambda h: h[0])
            if len(best) >= beam:
                kept = best
                break
    kept.sort(key=(lambda h: h[0] / len(h[1])) if score_norm else (lambda h: h[0]), reverse=True)
    return [(h[1], h[0]) for h in kept[:nbest]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cd", DT)
@pytest.mark.parametrize("layers", [1, 2])
def test_search_against_float64(layers, cd, mode):
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    beam, nbest, score_norm = MODES[mode]
    ref, r32 = (restate(layers, cd == "bf16", d, mode) for d in (torch.float64, torch.float32))
    assert [y for y, _ in ref] == [y for y, _ in r32] and len(ref) == nbest  # preconditions, on the CPU
    assert mode != "greedy" or 3 <= len(ref[0][0]) - 1 < T
    pair = gpu_pair(layers, cd)
    search = BeamSearchTransducer(pair.decoder, pair.joint_network, beam, nbest=nbest, score_norm=score_norm)
    got = search(weights(layers)[1][0].cuda())
    assert [h.yseq for h in got] == [y for y, _ in ref]
    want, s32 = (torch.tensor([s for _, s in r], dtype=torch.float64) for r in (ref, r32))
    tol = tolerance(want, float((s32 - want).abs().max()), MARGIN)
    dev = float((torch.tensor([h.score for h in got], dtype=torch.float64) - want).abs().max())
    print(f"scores {want.tolist()}: dev {dev:.3e} tol {tol:.3e}")
    assert dev <= tol


@pytest.mark.parametrize("cd", DT)
@pytest.mark.parametrize("layers", [1, 2])
def test_batched_greedy_equals_per_utterance_greedy(layers, cd):
    from espnet_amd.asr.inference import transducer_decode
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    pair, enc, lens = gpu_pair(layers, cd), weights(layers)[1].cuda(), [T, 7, 9]
    search = BeamSearchTransducer(pair.decoder, pair.joint_network, 1)
    one = [search(enc[i, :n])[0].yseq[1:] for i, n in enumerate(lens)]
    got = transducer_decode(pair, enc, torch.tensor(lens))
    assert [r[0][0] for r in got] == one and len({len(y) for y in one}) > 1 and pair.training is False
