"""decoder: transducer on the GPU.  TransducerDecoder + JointNetwork + RNNTLoss over a given encoder
output against a float64 restatement (two layers, dropout 0; tests/test_rnnt_kernels_gpu.py's loss, rd,
GradRound and tolerance).  bf16 rounds what the nodes round: every product's operands, and the gradients
the backward casts (dgates, lin_enc / lin_dec's output gradients, dlogits).  Then dropout, and training
steps of a tiny ESPnetASRModel with ctc_weight 0.3: captured equal to eager, the reference's stats keys."""
import pytest
import torch

from test_rnnt_kernels_gpu import DT, GradRound, close, rd, rnnt_loss
from test_transducer_build_cpu import ENCODER_CONF, TOK

pytestmark = pytest.mark.gpu
V, ENC, H, J, B, T, U, T_LEN, U_LEN = len(TOK), 24, 16, 40, 3, 6, 4, [6, 4, 5], [4, 0, 2]


def batch():
    g = torch.Generator().manual_seed(9)
    enc, y = torch.randn(B, T, ENC, generator=g), torch.randint(1, V, (B, U), generator=g)
    for i, n in enumerate(U_LEN):
        y[i, n:] = 0
    return enc, y, torch.cat([torch.zeros(B, 1, dtype=torch.long), y], dim=1)


def run_hip(cd, dropout=0.0, seeds=(0,)):  # -> (CPU state_dict, per seed the loss and every gradient)
    from espnet_amd.arena import ParamArena
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.joint_network import JointNetwork, RNNTLoss
    torch.manual_seed(5)
    pair = torch.nn.Module()
    pair.decoder = TransducerDecoder(V, num_layers=2, hidden_size=H, dropout=dropout, dropout_embed=dropout)
    pair.joint_network = JointNetwork(V, ENC, H, joint_space_size=J)
    sd = {k: v.detach().clone() for k, v in pair.state_dict().items()}
    arena = ParamArena(pair, "cuda", [], shadow_dtype=None if cd == torch.float32 else cd)
    pair.decoder.bind(arena, "decoder.", cd)
    pair.joint_network.bind(arena, "joint_network.", cd)
    enc, y, dec_in = batch()
    tl, ul = (torch.tensor(v, dtype=torch.int32).cuda() for v in (T_LEN, U_LEN))
    outs = []
    for seed in seeds:
        e = enc.cuda().requires_grad_(True)
        arena.zero_grad()
        loss = RNNTLoss()(pair.joint_network, e, pair.decoder(dec_in.cuda(), seed=seed), y.to(torch.int32).cuda(), tl, ul)
        loss.backward()
        torch.cuda.synchronize()
        outs.append(dict({k: p.grad.cpu().clone() for k, p in pair.named_parameters()}, loss=loss.detach().cpu(),
                         enc=e.grad.cpu()))
    return sd, outs


def restate(sd, enc, y, dec_in, dtype, amp):
    p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    enc = enc.to(dtype).requires_grad_(True)

    def mm(x, w):  # a product on rounded operands whose output gradient is cast to bf16
        return GradRound.apply(rd(x, amp) @ rd(p[w], amp).t(), amp)

    x = torch.nn.functional.embedding(dec_in, p["decoder.embed.weight"], padding_idx=0)
    for k in range(2):
        q = f"decoder.decoder.{k}."
        h, c, outs = x.new_zeros(B, H), x.new_zeros(B, H), []
        for s in range(U + 1):
            g = GradRound.apply(rd(x[:, s], amp) @ rd(p[q + "weight_ih_l0"], amp).t() +
                                rd(h, amp) @ rd(p[q + "weight_hh_l0"], amp).t(), amp) + p[q + "bias_ih_l0"] + p[q + "bias_hh_l0"]
            gi, gf, gg, go = g.chunk(4, dim=1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            outs.append(h)
        x = torch.stack(outs, dim=1)
    q = "joint_network."
    hj = torch.tanh((mm(enc, q + "lin_enc.weight") + p[q + "lin_enc.bias"])[:, :, None] + mm(x, q + "lin_dec.weight")[:, None])
    logits = GradRound.apply(rd(hj, amp) @ rd(p[q + "lin_out.weight"], amp).t() + p[q + "lin_out.bias"], amp)
    loss = rnnt_loss(logits, y, T_LEN, U_LEN)[0]
    loss.backward()
    out = {k: v.grad.detach() for k, v in p.items()}
    out.update(loss=loss.detach(), enc=enc.grad)
    return out


@pytest.mark.parametrize("cd", DT)
def test_decoder_joint_loss_against_float64(cd):
    sd, (got,) = run_hip(DT[cd])
    ref, r32 = (restate(sd, *batch(), d, cd == "bf16") for d in (torch.float64, torch.float32))
    assert not got["decoder.embed.weight"][0].any()  # the padding row
    for k, g in got.items():
        close(k, g, ref[k], r32[k])


def test_dropout_runs_and_differs_between_steps():
    _, (a, b) = run_hip(torch.float32, dropout=0.3, seeds=(1, 2))
    assert torch.isfinite(a["loss"]) and torch.isfinite(b["loss"]) and a["loss"] != b["loss"]


def _setup(amp):
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.tasks.asr import build_model
    torch.manual_seed(3)
    m = build_model(dict(token_list=TOK, input_size=20, encoder="conformer", encoder_conf=ENCODER_CONF,
                         decoder="transducer", decoder_conf=dict(num_layers=1, hidden_size=H, dropout=0.1),
                         joint_net_conf=dict(joint_space_size=640),  # > 64 KiB of LDS, under capture too
                         model_conf=dict(ctc_weight=0.3, report_cer=False, report_wer=False)))
    m.prepare("cuda:0", amp=amp, seed=3)
    m.train()
    g = torch.Generator().manual_seed(4)
    b1 = dict(speech=torch.randn(2, 50, 20, generator=g), speech_lengths=torch.tensor([50, 41]),
              text=torch.tensor([[3, 4, 5, 6], [7, 8, -1, -1]]), text_lengths=torch.tensor([4, 2]))
    b2 = dict(b1, speech_lengths=torch.tensor([37, 50]), text=torch.tensor([[3, -1, -1, -1], [7, 8, 9, 4]]),
              text_lengths=torch.tensor([1, 4]))
    return m, ArenaAdam(m, lr=1e-3), [b1, b2, b1, b2]


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
def test_captured_step_equals_eager_and_stats_are_the_references(amp):
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    KEYS = ("loss", "loss_ctc", "loss_transducer")
    m1, o1, seq = _setup(amp)
    eager = []
    for b in seq:
        loss, stats, _, _ = Trainer.train_one_step(m1, b, o1, None, grad_clip=5.0)
        eager.append([float(stats[k]) for k in KEYS])
    want = eager[0][2] + 0.3 * eager[0][1]
    assert all(v == v for e in eager for v in e) and abs(eager[0][0] - want) <= 4e-7 * abs(want) and eager[0] != eager[1]
    m2, o2, seq = _setup(amp)
    run = CapturedTrainStep(m2, o2, None, grad_clip=5.0, warmup=1)
    graph = []
    for b in seq:
        stats = run(b)[1]
        graph.append([float(stats[k]) for k in KEYS])
    torch.cuda.synchronize()
    assert len(run.graphs) == 1 and run.mode == "graph"
    assert eager == graph
    for (k, p1), p2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(p1, p2), k
    _, stats, weight = m1(**seq[0])  # the model's own stats: the reference's keys, cer / wer None in training
    assert {"cer_ctc", "cer_transducer", "wer_transducer"} <= set(stats) and int(weight) == 2
    assert stats["cer_transducer"] is None and stats["wer_transducer"] is None
