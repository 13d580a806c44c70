"""ConformerEncoder / TransformerEncoder with input_layer conv2d6 and conv2d2 on the MI355X: `embed`'s
output, the lengths and the gradients of its parameters against a float64 restatement in plain torch.nn
modules loaded from the same state_dict; the short-utterance limit; captured steps == eager steps.
d 16, 2 heads, 1 block, dropout 0, B 3 ragged, T 38, F 20: x1 is 18x9 (conv2d6: an uncovered row and column).

Tolerance: tests/test_conv_sub_strided_kernels_gpu.py's rule on the whole restatement.  bf16: the
restatement rounds to bf16 what the HIP path keeps in bf16: the features and weights as GEMM operands,
x1, x2 and the gradients dv, dx2, dx1; every checked array is f32."""
import math

import pytest
import torch
from torch import nn

from goldens import load, section
from rnn_encoder_goldens import prepare_encoder
from test_conv_sub_strided_kernels_gpu import _check

pytestmark = pytest.mark.gpu
KS = {"conv2d6": (5, 3, 11), "conv2d2": (3, 1, 7)}  # kernel, stride of conv.2; check_short_utt's limit
B, T, FD, D = 3, 38, 20, 16
ILENS = [38, 27, 16]


def _encoder(kind, layer, idim=FD):
    from espnet_amd.asr.encoder.conformer_encoder import ConformerEncoder
    from espnet_amd.asr.encoder.transformer_encoder import TransformerEncoder
    kw = dict(input_size=idim, output_size=D, attention_heads=2, linear_units=32, num_blocks=1, dropout_rate=0.0,
              positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer=layer)
    if kind == "transformer":
        return TransformerEncoder(**kw)
    return ConformerEncoder(rel_pos_type=kind, cnn_module_kernel=7, **kw)


def _bf(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


class _Stored(torch.autograd.Function):
    """An activation the bf16 path stores in bf16 (fwd) whose gradient it stores in bf16 too."""

    @staticmethod
    def forward(ctx, x, fwd):
        return _bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return _bf(g), None


def _restate(sd, layer, xs, cot, absolute, dtype, amp):
    """-> (embed's output (B, T', D), {embed parameter: gradient}) in `dtype` on the CPU."""
    k, s, _ = KS[layer]
    stored = (lambda t, fwd=True: _Stored.apply(t, fwd)) if amp else (lambda t, fwd=True: t)
    conv1, conv2 = nn.Conv2d(1, D, 3, 2), nn.Conv2d(D, D, k, s)
    lin = nn.Linear(sd["embed.out.0.weight"].shape[1], D)
    mods = {"conv.0": conv1, "conv.2": conv2, "out.0": lin}
    for name, m in mods.items():
        w, b = sd[f"embed.{name}.weight"].detach().cpu(), sd[f"embed.{name}.bias"].detach().cpu()
        m.load_state_dict(dict(weight=_bf(w) if amp else w, bias=b))
        m.to(dtype)
    x = (_bf(xs) if amp else xs).to(dtype).unsqueeze(1)
    x = stored(torch.relu(conv1(x)))
    x = stored(torch.relu(conv2(x)))
    b_, c, t, f = x.shape
    y = stored(lin(x.transpose(1, 2).reshape(b_, t, c * f)), False) * math.sqrt(D)
    if absolute:  # embedding.py:58-92
        pos = torch.arange(t, dtype=dtype).unsqueeze(1)
        div = torch.exp(torch.arange(0, D, 2, dtype=dtype) * -(math.log(10000.0) / D))
        pe = torch.zeros(t, D, dtype=dtype)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
        y = y + pe
    y.backward(cot.to(dtype))
    grads = {f"{n}.{p}": getattr(m, p).grad for n, m in mods.items() for p in ("weight", "bias")}
    return y.detach(), grads


@pytest.mark.parametrize("amp", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer", list(KS))
@pytest.mark.parametrize("kind", ["latest", "legacy", "transformer"])
def test_embed_output_lengths_and_gradients(kind, layer, amp):
    k, s, _ = KS[layer]
    torch.manual_seed(3)
    enc = _encoder(kind, layer)
    sd = {n: v.clone() for n, v in enc.state_dict().items()}
    arena = prepare_encoder(enc, amp)  # noqa: F841  (keeps the arena alive)
    gen = torch.Generator().manual_seed(11)
    xs = torch.randn(B, T, FD, generator=gen)
    ilens = torch.tensor(ILENS)
    enc.train()
    for p in enc.parameters():
        p.grad.zero_()
    x, olens = enc.front(xs.cuda(), ilens.cuda(), 0)
    cot = torch.randn(x.shape, generator=gen)
    x.backward(cot.cuda())
    torch.cuda.synchronize()
    assert x.dtype == torch.float32
    mask = (torch.arange(T)[None, :] < ilens[:, None]).unsqueeze(1)
    assert olens.cpu().tolist() == mask[:, :, :-2:2][:, :, :-(k - 1):s].sum(-1).squeeze(1).tolist()
    assert x.shape[1] == int(olens.max())
    (y64, g64), (y32, g32) = (_restate(sd, layer, xs, cot, kind == "transformer", dt, amp)
                              for dt in (torch.float64, torch.float32))
    _check(x.detach().cpu(), y64, y32, "embed output")
    for n in g64:
        mod, leaf = n.rsplit(".", 1)
        _check(getattr(enc.embed.get_submodule(mod), leaf).grad.cpu(), g64[n], g32[n], n + " gradient")


@pytest.mark.parametrize("layer", list(KS))
def test_one_frame_below_the_limit_is_too_short(layer):
    from espnet_amd.asr.encoder.abs_encoder import TooShortUttError
    limit = KS[layer][2]
    enc = _encoder("latest", layer)
    arena = prepare_encoder(enc)  # noqa: F841
    with pytest.raises(TooShortUttError) as e:
        enc(torch.zeros(2, limit - 1, FD, device="cuda"), torch.tensor([limit - 1, 3], device="cuda"))
    assert (e.value.actual_size, e.value.limit) == (limit - 1, limit)
    x, olens = enc.front(torch.zeros(2, limit, FD, device="cuda"), torch.tensor([limit, 3], device="cuda"), 0)
    assert x.shape == (2, 1, D) and olens.tolist() == [1, 1]  # the limit itself gives one frame


def _hybrid():
    from espnet_amd.optim.adam import ArenaAdam
    from espnet_amd.tasks.asr import build_model
    cfg, d = load("tiny_hybrid")
    V = cfg["vocab_size"]
    tok = ["<blank>", "<unk>"] + [f"t{i}" for i in range(V - 3)] + ["<sos/eos>"]
    torch.manual_seed(5)
    m = build_model(dict(token_list=tok, input_size=cfg["input_size"], encoder="conformer",
                         encoder_conf=dict(cfg["encoder_conf"], input_layer="conv2d6"), decoder="transformer",
                         decoder_conf=cfg["decoder_conf"], model_conf=cfg["model_conf"]))
    m.prepare("cuda:0", amp=False, seed=9)
    m.train()
    batch = {k: torch.from_numpy(v) for k, v in section(d, "in").items()}
    noise = torch.randn(batch["speech"].shape, generator=torch.Generator().manual_seed(1))
    return m, ArenaAdam(m, lr=0.002), [batch, dict(batch, speech=batch["speech"] + noise)]


def test_captured_steps_equal_eager_steps():
    """Two training steps of a tiny hybrid model with input_layer conv2d6 through CapturedTrainStep
    (warm-up, then capture and replay) equal two eager steps bit for bit."""
    from espnet_amd.train.graph import CapturedTrainStep
    from espnet_amd.train.trainer import Trainer
    torch.cuda.set_device(0)
    m1, o1, batches = _hybrid()
    eager = [float(Trainer.train_one_step(m1, b, o1, None, grad_clip=5.0)[0]) for b in batches]
    m2, o2, batches = _hybrid()
    run = CapturedTrainStep(m2, o2, None, grad_clip=5.0, warmup=1)
    graph = [float(run(b)[0]) for b in batches]
    torch.cuda.synchronize()
    assert run.mode == "graph" and len(run.graphs) == 1
    assert eager == graph and eager[0] != eager[1]
