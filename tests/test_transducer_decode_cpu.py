"""Transducer decoding without a GPU: what the search and the joint step do not build is refused by name."""
import pytest
import torch

V, H = 23, 32


def _pair():
    from espnet_amd.asr.decoder.transducer_decoder import TransducerDecoder
    from espnet_amd.asr.joint_network import JointNetwork
    return TransducerDecoder(V, hidden_size=H), JointNetwork(V, 24, H, joint_space_size=40)


@pytest.mark.parametrize("kw,match", [
    (dict(beam_size=2, search_type="tsd"), r"search_type='tsd' is not built"),
    (dict(beam_size=2, search_type="alsd"), r"search_type='alsd' is not built"),
    (dict(beam_size=2, search_type="nsc"), r"search_type='nsc' is not built"),
    (dict(beam_size=2, search_type="maes"), r"search_type='maes' is not built"),
    (dict(beam_size=2, lm=torch.nn.Identity()), r"lm is not built"),
    (dict(beam_size=17), r"beam_size=17 is not built"),
])
def test_search_refuses_by_name(kw, match):
    from espnet_amd.asr.transducer.beam_search_transducer import BeamSearchTransducer
    with pytest.raises(NotImplementedError, match=match):
        BeamSearchTransducer(*_pair(), **kw)
    BeamSearchTransducer(*_pair(), beam_size=16)  # the widest beam that is built


@pytest.mark.parametrize("n,k,match", [(0, 1, "n=0 rows"), (65, 1, "n=65 rows"), (1, 0, "k=0"), (1, 17, "k=17"),
                                       (1, V, f"k={V} with vocabulary {V}")])
def test_joint_step_limits_by_name(n, k, match):
    jn = _pair()[1]
    with pytest.raises(ValueError, match=match):
        jn.step(torch.zeros(4, 40), torch.zeros(n, dtype=torch.int32), torch.zeros(n, 40), k)
