"""CPU suite: the pieces of voice conversion that need no GPU - the glowtts_flow_encode symbol (declared, bound, exported), the `--convert`
list format, and the Vanilla-mode refusal, which comes before any device work."""
import ctypes
import os
import re

import pytest
import torch

from helpers import tiny_hp_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_encode_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "glowtts_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+glowtts_flow_encode\s*\(\s*const glowtts_flow_dims \*d,\s*const glowtts_flow_params \*p,\s*const glowtts_flow_acts \*a,"
                     r"\s*void \*stream\)", header)
    from glow_tts_amd import abi
    restype, argtypes = abi.SIGNATURES["glowtts_flow_encode"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 4
    so = os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(so)
    assert hasattr(L, "glowtts_flow_encode")
    assert L.glowtts_abi_version() == 7


def test_convert_list_parses(tmp_path):
    from glow_tts_amd.inferencer import read_convert_list
    p = tmp_path / "convert.tsv"
    p.write_text("Label\tSource\tSource_Speaker\tTarget_Speaker\tTarget_Reference\n"
                 "a\t/x/a.npy\t3\t7\t/x/ref.wav\n"
                 "\n"
                 "b\t/x/b.wav\t1\t1\n"
                 "c\t/x/c.npy\t\t\t\n")
    recs = read_convert_list(str(p))
    assert recs == [
        {"label": "a", "source": "/x/a.npy", "source_speaker": 3, "target_speaker": 7, "target_reference": "/x/ref.wav"},
        {"label": "b", "source": "/x/b.wav", "source_speaker": 1, "target_speaker": 1, "target_reference": None},
        {"label": "c", "source": "/x/c.npy", "source_speaker": None, "target_speaker": None, "target_reference": None},
    ]
    q = tmp_path / "noheader.tsv"
    q.write_text("x\t/x/x.npy\t0\t2\n")
    assert read_convert_list(str(q))[0]["target_speaker"] == 2
    bad = tmp_path / "bad.tsv"
    bad.write_text("x\t/x/x.npy\n")
    with pytest.raises(ValueError):
        read_convert_list(str(bad))


def test_vanilla_voice_conversion_raises_before_device_work():
    from glow_tts_amd.hparams import Recursive_Parse
    from glow_tts_amd.modules import GlowTTS
    model = GlowTTS(Recursive_Parse(tiny_hp_dict("Vanilla"))).eval()
    mels, lengths = torch.zeros(2, 12, 20), torch.tensor([20, 15])
    with pytest.raises(ValueError, match="conditioned"):
        model.voice_conversion(mels, lengths)
    assert all(p.device.type == "cpu" for p in model.parameters())
