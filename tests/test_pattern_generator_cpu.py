"""CPU suite of the pattern generator and the host side of the analysis front end: the new C symbols, the sparse filterbank, `Pattern_Generator.py --host`
through the LJ / VCTK / list layouts (paths, keys, dtypes, bit-equality with `audio.pattern_from_wav`, Token.yaml, both metadata pickles, the eval split,
idempotence) and the geometry errors of `frontend.Analyzer`."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import frontend_cases as C  # noqa: E402

NEW_SYMBOLS = ["glowtts_mel_analysis_f32", "glowtts_yin_f32"]


def test_new_symbols_are_declared_and_exported_with_abi_7():
    header = open(os.path.join(REPO, "include", "glowtts_hip.h")).read()
    assert re.search(r"#define GLOWTTS_ABI_VERSION\s+7\b", header)
    so = os.path.join(REPO, "glow_tts_amd", "libglowtts_hip.so")
    if not os.path.exists(so):
        sys.path.insert(0, REPO)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(so)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header), f"{n} not declared"
        assert hasattr(L, n), f"{n} not exported"
    assert L.glowtts_abi_version() == 7


@pytest.mark.parametrize("geo", ["full", "tiny"])
def test_sparse_filterbank_reconstructs_the_dense_one(geo):
    from glow_tts_amd import audio, frontend
    (n_fft, _, _), n_mel = C.GEOS[geo]
    fb = audio.mel_filterbank(C.SR, n_fft, n_mel, 125, 7600)
    index, weights = frontend.sparse_filterbank(fb)
    assert index.dtype == np.int32 and index.shape == (n_mel, 3) and weights.dtype == np.float32
    assert np.array_equal(frontend.dense_filterbank(index, weights, n_fft // 2 + 1), fb)
    assert int((fb > 0).sum(axis=0).max()) <= 2                    # a bin lies under at most two triangles
    assert (index[:, 0] >= 0).all() and (index[:, 0] + index[:, 1] <= n_fft // 2 + 1).all()
    assert np.array_equal(index[:, 2], np.concatenate([[0], np.cumsum(index[:-1, 1])])) and index[:, 1].sum() == weights.size
    assert weights.size <= 2 * (n_fft // 2 + 1)                    # the point of the sparse form


def _mtimes(root):
    return {p: os.stat(os.path.join(root, p)).st_mtime_ns for p in C.load_patterns(root)}


def test_lj_layout_through_the_host_path(tmp_path, capsys):
    import yaml
    from glow_tts_amd import audio, data, pattern_generator
    corpus, out = str(tmp_path / "LJSpeech-1.1"), str(tmp_path / "out")
    os.makedirs(out)
    names = C.make_lj_tree(corpus)
    yml, hp = C.write_hp(out)
    argv = ["-hp", yml, "-lj", corpus, "-text", "--host", "-evalr", "0.4", "-evalm", "1", "-mw", "2"]
    res = pattern_generator.main(argv)
    assert res["written"] == 3 and res["failed"] == 0 and (res["train"], res["eval"]) == (2, 1)      # max(1, int(3 * 0.4)) = 1
    assert "LJ001-0003" in capsys.readouterr().out                 # the rejected text is reported
    train, evals = C.load_patterns(hp.Train.Train_Pattern.Path), C.load_patterns(hp.Train.Eval_Pattern.Path)
    assert len(train) == 2 and len(evals) == 1
    both = dict(train, **evals)
    kept = [n for n in names if n != "LJ001-0003"]
    assert sorted(both) == ["LJ/LJ/LJ.{}.PICKLE".format(n) for n in kept]
    texts = {n: data.text_filtering(t) for n, t in C.LJ_TEXTS}
    for n in kept:
        pat = both["LJ/LJ/LJ.{}.PICKLE".format(n)]
        assert set(pat) == {"Audio", "Mel", "Pitch", "Speaker_ID", "Speaker", "Dataset", "Text"}
        assert pat["Audio"].dtype == pat["Mel"].dtype == pat["Pitch"].dtype == np.float32
        assert (pat["Speaker_ID"], pat["Speaker"], pat["Dataset"], pat["Text"]) == (0, "LJ", "LJ", texts[n])
        T = 1 + len(pat["Audio"]) // 256
        assert pat["Audio"].ndim == 1 and pat["Mel"].shape == (T, 80) and pat["Pitch"].shape == (T,) and T > 20
        mel, pitch = audio.pattern_from_wav(os.path.join(corpus, "wavs", n + ".wav"), hp, top_db=60, with_pitch=True)
        assert np.array_equal(pat["Mel"], mel) and np.array_equal(pat["Pitch"], pitch)
    with open(hp.Token_Path) as f:
        assert yaml.safe_load(f) == data.make_token_dict([texts[n] for n in kept])
    tokens = data.load_token_dict(hp.Token_Path)
    for pattern, n in ((hp.Train.Train_Pattern, 2), (hp.Train.Eval_Pattern, 1)):
        ds = data.PatternDataset(pattern.Path, pattern.Metadata_File, tokens)
        assert len(ds) == n
        tok, mel, spk, pit = ds[0]
        assert mel.shape[0] == pit.shape[0] and spk == 0 and tok[0] == tokens["<S>"] and tok[-1] == tokens["<E>"]
        with open(os.path.join(pattern.Path, pattern.Metadata_File), "rb") as f:
            assert pickle.load(f)["Frame_Shift"] == 256
    # a second run finds every pattern and writes none
    before = (_mtimes(hp.Train.Train_Pattern.Path), _mtimes(hp.Train.Eval_Pattern.Path))
    res = pattern_generator.main(argv)
    assert res["written"] == 0 and res["failed"] == 0
    assert before == (_mtimes(hp.Train.Train_Pattern.Path), _mtimes(hp.Train.Eval_Pattern.Path))
    # the minimum wins over the ratio
    assert [len(x) for x in pattern_generator.split_eval([{"path": str(i)} for i in range(10)], 0.001, 3)] == [7, 3]
    assert [len(x) for x in pattern_generator.split_eval([{"path": str(i)} for i in range(10)], 0.5, 1)] == [5, 5]


def test_vctk_layout_speakers_and_the_p315_rule(tmp_path):
    from glow_tts_amd import audio, data, pattern_generator
    corpus = str(tmp_path / "VCTK-Corpus")
    C.make_vctk_tree(corpus)
    out = str(tmp_path / "text")
    os.makedirs(out)
    yml, hp = C.write_hp(out)
    res = pattern_generator.main(["-hp", yml, "-vctk", corpus, "-text", "--host", "-evalm", "1", "-mw", "2"])
    assert res["written"] == 3 and res["failed"] == 0 and res["eval"] == 1
    both = dict(C.load_patterns(hp.Train.Train_Pattern.Path), **C.load_patterns(hp.Train.Eval_Pattern.Path))
    assert sorted(both) == ["VCTK/VCTK.P225/VCTK.P225.P225_001.PICKLE", "VCTK/VCTK.P225/VCTK.P225.P225_002.PICKLE", "VCTK/VCTK.P226/VCTK.P226.P226_001.PICKLE"]
    for rel, pat in both.items():                                  # p315 has no transcripts: with text it is left out, ids run over the sorted rest
        assert pat["Speaker_ID"] == {"VCTK.P225": 0, "VCTK.P226": 1}[pat["Speaker"]] and pat["Dataset"] == "VCTK"
        spk, name = [(s, n) for s, n, _ in C.VCTK_FILES if n.upper() in rel][0]
        assert pat["Text"] == data.text_filtering([t for _, n, t in C.VCTK_FILES if n == name][0])
        mel, pitch = audio.pattern_from_wav(os.path.join(corpus, "wav48", spk, name + ".wav"), hp, top_db=15, with_pitch=True)      # resampled 48 -> 24 kHz
        assert np.array_equal(pat["Mel"], mel) and np.array_equal(pat["Pitch"], pitch) and mel.shape[0] == pitch.shape[0] > 10
    # without text every speaker is in, none of the patterns carries a text, and the metadata has no text lengths
    out = str(tmp_path / "notext")
    os.makedirs(out)
    yml, hp = C.write_hp(out)
    res = pattern_generator.main(["-hp", yml, "-vctk", corpus, "--host", "-evalm", "1"])
    assert res["written"] == 4
    both = dict(C.load_patterns(hp.Train.Train_Pattern.Path), **C.load_patterns(hp.Train.Eval_Pattern.Path))
    assert {p["Speaker"]: p["Speaker_ID"] for p in both.values()} == {"VCTK.P225": 0, "VCTK.P226": 1, "VCTK.P315": 2}
    assert all("Text" not in p for p in both.values()) and not os.path.exists(hp.Token_Path)
    with open(os.path.join(hp.Train.Train_Pattern.Path, "METADATA.PICKLE"), "rb") as f:
        meta = pickle.load(f)
    assert "Text_Length_Dict" not in meta and len(meta["File_List"]) == 3
    # the optional list of utterances to keep
    with open(os.path.join(corpus, "VCTK.NonOutlier.txt"), "w") as f:
        f.write("p225_001.wav\np226_001\n")
    assert [os.path.basename(x["path"]) for x in pattern_generator.walk_corpus("VCTK", corpus, True)] == ["p225_001.wav", "p226_001.wav"]


def test_generic_list_with_its_own_trim_level(tmp_path):
    from glow_tts_amd import audio, pattern_generator
    corpus = str(tmp_path / "LJ")
    C.make_lj_tree(corpus)
    out = str(tmp_path / "out")
    os.makedirs(out)
    yml, hp = C.write_hp(out)
    lst = str(tmp_path / "LJ" / "corpus.tsv")
    with open(lst, "w") as f:
        f.write("wavs/LJ001-0001.wav\tMY\tBeta\tHello there.\n")
        f.write("\n")
        f.write("{}\tMY\tAlpha\tGeneral Kenobi!\t20\n".format(os.path.join(corpus, "wavs", "LJ001-0002.wav")))
        f.write("wavs/LJ001-0004.wav\tMY\tBeta\tnumber 4 is rejected\n")                                  # rejected text
        f.write("wavs/missing.wav\tMY\tBeta\tThis file does not exist.\n")                    # reported, skipped, the run goes on
    res = pattern_generator.main(["-hp", yml, "--list", lst, "-text", "--host", "-evalm", "1"])
    assert res["written"] == 2 and res["failed"] == 1
    both = dict(C.load_patterns(hp.Train.Train_Pattern.Path), **C.load_patterns(hp.Train.Eval_Pattern.Path))
    assert sorted(both) == ["MY/Alpha/MY.ALPHA.LJ001-0002.PICKLE", "MY/Beta/MY.BETA.LJ001-0001.PICKLE"]
    a, b = both["MY/Alpha/MY.ALPHA.LJ001-0002.PICKLE"], both["MY/Beta/MY.BETA.LJ001-0001.PICKLE"]
    assert (a["Speaker_ID"], a["Text"], b["Speaker_ID"], b["Text"]) == (0, "GENERAL KENOBI!", 1, "HELLO THERE.")
    for pat, name, top_db in ((a, "LJ001-0002", 20), (b, "LJ001-0001", 60)):
        mel, pitch = audio.pattern_from_wav(os.path.join(corpus, "wavs", name + ".wav"), hp, top_db=top_db, with_pitch=True)
        assert np.array_equal(pat["Mel"], mel) and np.array_equal(pat["Pitch"], pitch)
    assert len(a["Audio"]) < len(audio.audio_prep(os.path.join(corpus, "wavs", "LJ001-0002.wav"), C.SR, 60))      # the fifth column took effect
    with pytest.raises(ValueError):
        with open(lst, "w") as f:
            f.write("only\ttwo\n")
        pattern_generator.read_list(lst)


def test_analyzer_refuses_geometries_by_their_yaml_keys_without_a_device():
    from glow_tts_amd import frontend
    assert frontend.geometry(C.hp()) == (2048, 1024, 256)
    assert frontend.geometry(C.hp("tiny"), with_pitch=False) == (256, 256, 64)
    assert frontend.geometry(C.hp(Frame_Length=1000)) == (2048, 1000, 256)                    # no Frame_Length % Frame_Shift condition here
    cases = [(dict(Spectrogram_Dim=1001), True, ["Sound.Spectrogram_Dim"]),
             (dict(Spectrogram_Dim=65, Frame_Length=64), True, ["Sound.Spectrogram_Dim"]),
             (dict(Spectrogram_Dim=4097), True, ["Sound.Spectrogram_Dim"]),
             (dict(Spectrogram_Dim=257, Frame_Length=1024), True, ["Sound.Frame_Length"]),
             (dict(Frame_Shift=0), False, ["Sound.Frame_Shift"]),
             (dict(Frame_Shift=200), True, ["Sound.Frame_Shift"]),
             (dict(Spectrogram_Dim=129, Frame_Length=256, Frame_Shift=64), True, ["Sound.Frame_Shift"])]
    for sound, with_pitch, keys in cases:
        with pytest.raises(ValueError) as e:
            frontend.Analyzer(C.hp(**sound), "cuda:0", with_pitch=with_pitch)                 # raised before anything touches a device
        for k in keys:
            assert k in str(e.value), (sound, str(e.value))
    assert frontend.yin_frames(0) == 0
    for n in (1, 255, 256, 257, 700, 2148, 16391, 72000):
        from glow_tts_amd import audio
        assert frontend.yin_frames(n) == 1 + n // 256 or n < 2
        if n > 1:
            assert frontend.yin_frames(n) == len(audio.yin_pitch(np.zeros(n), C.SR, 0.4))
            assert frontend.yin_frames(n, 256, 64) == len(audio.yin_pitch(np.zeros(n), C.SR, 0.4, w_len=256, w_step=64))
