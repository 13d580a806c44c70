"""Capture tests/golden/transducer_build.npz from the REFERENCE's TransducerDecoder and JointNetwork: cfg
only (the small-size substitutes of the librispeech recipe's decoder_conf / joint_net_conf, the sizes, per
module the state_dict keys and shapes).  Test infrastructure, not collected by pytest.
Run:  PYTHONDONTWRITEBYTECODE=1 python -B tests/capture_transducer_goldens.py"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import numpy as np  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402

VOCAB, ENC = 23, 64
CONF = dict(decoder_conf=dict(rnn_type="lstm", num_layers=2, hidden_size=48, dropout=0.1, dropout_embed=0.2),
            joint_net_conf=dict(joint_space_size=40))

if __name__ == "__main__":
    from espnet2.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet2.asr_transducer.joint_network import JointNetwork
    dec = TransducerDecoder(VOCAB, embed_pad=0, **CONF["decoder_conf"])
    mods = dict(decoder=dec, joint_network=JointNetwork(VOCAB, ENC, dec.dunits, **CONF["joint_net_conf"]))
    cfg = dict(vocab_size=VOCAB, encoder_output_size=ENC, conf=CONF)
    for name, m in mods.items():
        sd = m.state_dict()
        cfg[name] = dict(keys=list(sd), shapes=[list(v.shape) for v in sd.values()])
    np.savez_compressed(os.path.join(mg.OUT, "transducer_build.npz"), cfg=np.array(json.dumps(cfg)))
