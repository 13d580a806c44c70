"""decoder: transducer without a GPU: the librispeech recipe's blocks (small sizes) build through ASRTask with the
state_dict layout tests/capture_transducer_goldens.py recorded from the reference; the rest is refused by name."""
import pytest

from goldens import load

TOK = ["<blank>", "<unk>"] + [f"t{i}" for i in range(20)] + ["<sos/eos>"]
ENCODER_CONF = dict(output_size=64, attention_heads=4, linear_units=128, num_blocks=2, dropout_rate=0.1,
                    positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d",
                    normalize_before=True, pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn",
                    activation_type="swish", macaron_style=True, use_cnn_module=True, cnn_module_kernel=15)


def _build(**over):
    from espnet_amd.tasks.asr import ASRTask
    conf = load("transducer_build")[0]["conf"]
    a = dict(token_list=TOK, input_size=80, encoder="conformer", encoder_conf=ENCODER_CONF, decoder="transducer",
             decoder_conf=conf["decoder_conf"], joint_net_conf=conf["joint_net_conf"],
             model_conf=dict(ctc_weight=0.3, report_cer=False, report_wer=False))
    return ASRTask.build_model(dict(a, **over))


def test_recipe_blocks_build_with_the_references_layout():
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.tasks.asr import decoder_choices
    cfg, _ = load("transducer_build")
    assert decoder_choices.get_class("transducer") is TransducerDecoder
    assert len(TOK) == cfg["vocab_size"] and ENCODER_CONF["output_size"] == cfg["encoder_output_size"]
    m = _build()
    assert m.use_transducer_decoder and m.ctc is not None and m.criterion_transducer.chunk_bytes == 1 << 30
    for name in ("decoder", "joint_network"):
        sd = getattr(m, name).state_dict()
        assert list(sd) == cfg[name]["keys"]
        assert [list(v.shape) for v in sd.values()] == cfg[name]["shapes"]


@pytest.mark.parametrize("over,match", [
    (dict(decoder_conf=dict(rnn_type="gru")), r"TransducerDecoder: rnn_type='gru' is not built"),
    (dict(joint_net_conf=dict(joint_activation_type="relu")), r"joint_activation_type='relu' is not built"),
    (dict(joint_net_conf=dict(joint_space_size=1024)), r"joint_space_size=1024 is not built"),
    (dict(model_conf=dict(ctc_weight=0.3)), r"report_cer=True / report_wer=True with a transducer decoder"),
    (dict(model_conf=dict(ctc_weight=1.0, report_cer=False, report_wer=False)), r"ctc_weight=1.0 with a transducer"),
    (None, "decoder: transducer"),
])
def test_refused_by_name(over, match):
    from espnet_amd.asr.inference import attention_beam_search
    with pytest.raises(NotImplementedError, match=match):
        _build(**over) if over is not None else attention_beam_search(_build(), None, None, beam_size=2)
