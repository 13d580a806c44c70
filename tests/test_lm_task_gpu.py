"""lm_train end to end on the GPU: a generated text_int corpus (240 short lines over the tiny
hybrid model's 50-token vocabulary, so that the trained LM can be fused with it), 2 epochs,
batch_type folded; the files the task writes, a falling train loss, --resume, and the saved
model loading through build_lm into attention_beam_search."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

V = 50


def _corpus(d, n, seed):
    """Sentences that follow one fixed successor rule from a random start: learnable in an epoch."""
    d.mkdir()
    g = torch.Generator().manual_seed(seed)
    text, shape = [], []
    for i in range(n):
        ln = int(torch.randint(2, 10, (1,), generator=g))
        tok = [int(torch.randint(2, V - 1, (1,), generator=g))]
        for _ in range(ln - 1):
            tok.append((tok[-1] * 3 + 1) % (V - 3) + 2)
        text.append(f"utt{i:03d} " + " ".join(map(str, tok)))
        shape.append(f"utt{i:03d} {ln}")
    (d / "text").write_text("\n".join(text) + "\n")
    (d / "shape").write_text("\n".join(shape) + "\n")
    return d


def test_lm_train_end_to_end_resume_and_fusion(tmp_path):
    import yaml
    from espnet_amd.asr.inference import attention_beam_search
    from espnet_amd.bin import lm_train
    from espnet_amd.lm import build_lm, lm_state_dict
    from test_inference_gpu import _setup

    tr, dv = _corpus(tmp_path / "tr", 240, 0), _corpus(tmp_path / "dv", 40, 1)
    (tmp_path / "tokens.txt").write_text("\n".join(["<blank>", "<unk>"] + [f"c{i}" for i in range(V - 3)]
                                                   + ["<sos/eos>"]) + "\n")
    lm_conf = dict(unit=32, nlayers=2, dropout_rate=0.1)
    conf = dict(lm="seq_rnn", lm_conf=lm_conf, optim="adam", optim_conf=dict(lr=0.01), batch_type="folded",
                batch_size=16, fold_length=[150], max_epoch=2, num_workers=0, keep_nbest_models=[2],
                best_model_criterion=[["valid", "loss", "min"]], grad_clip=5.0)
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(conf))
    out = tmp_path / "exp"
    cmd = ["--config", str(tmp_path / "c.yaml"), "--output_dir", str(out), "--ngpu", "1",
           "--token_list", str(tmp_path / "tokens.txt"),
           "--train_data_path_and_name_and_type", f"{tr}/text,text,text_int", "--train_shape_file", f"{tr}/shape",
           "--valid_data_path_and_name_and_type", f"{dv}/text,text,text_int", "--valid_shape_file", f"{dv}/shape"]
    lm_train.main(cmd)
    files = {p.name for p in out.iterdir()}
    assert {"config.yaml", "checkpoint.pth", "latest.pth", "1epoch.pth", "2epoch.pth", "valid.loss.best.pth",
            "valid.loss.ave.pth", "valid.loss.ave_2best.pth"} <= files, files
    saved = yaml.safe_load((out / "config.yaml").read_text())
    assert saved["lm"] == "seq_rnn" and len(saved["token_list"]) == V and saved["lm_conf"]["unit"] == 32
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=True)
    stats = ck["reporter"]["stats"]
    assert ck["reporter"]["epoch"] == 2 and stats[2]["train"]["total_count"] == 2 * 15
    for k in ("loss", "iter_time", "forward_time", "backward_time", "optim_step_time", "train_time", "optim0_lr0"):
        assert math.isfinite(stats[2]["train"][k]), k
    assert stats[2]["train"]["loss"] < stats[1]["train"]["loss"] < math.log(V)
    assert stats[2]["valid"]["loss"] < stats[1]["valid"]["loss"]
    assert all(k.startswith("lm.") for k in ck["model"])

    # --resume continues from the checkpoint
    lm_train.main(cmd + ["--resume", "true", "--max_epoch", "3"])
    ck3 = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=True)
    assert ck3["reporter"]["epoch"] == 3 and int(ck3["optimizers"][0]["state"][0]["step"]) == 3 * 15
    assert ck3["reporter"]["stats"][3]["train"]["loss"] < stats[2]["train"]["loss"]

    # the saved models load through build_lm and fuse in the beam search
    m, _, inp = _setup()
    assert m.vocab_size == V
    nbests = []
    for fn in ("valid.loss.best.pth", "checkpoint.pth"):
        lm = build_lm(saved["lm"], saved["lm_conf"], V)
        lm.load_state_dict(lm_state_dict(out / fn))
        lm.prepare("cuda").eval()
        nbests.append(attention_beam_search(m, inp["speech"][:1], inp["speech_lengths"][:1], 3, 0.0, 0.0,
                                            ctc_weight=0.3, lm=lm, lm_weight=0.3)[0])
    for nbest in nbests:
        assert len(nbest) >= 1 and int(nbest[0].yseq[0]) == m.sos and int(nbest[0].yseq[-1]) == m.eos
        assert math.isfinite(float(nbest[0].score)) and float(nbest[0].scores["lm"]) < 0
    # the trained LM has learnt something of the successor rule: the rule's next token is more
    # likely than under the uniform distribution it started from
    nxt = lambda t: (t * 3 + 1) % (V - 3) + 2  # noqa: E731
    with torch.no_grad():
        logits, _ = lm(torch.tensor([[V - 1, 7, nxt(7)]]), None)
    logp = torch.log_softmax(logits[0, -1].float(), dim=-1)
    assert float(logp[nxt(nxt(7))]) > -math.log(V)
