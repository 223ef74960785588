"""FLAC frames encoded on the GPU (csrc/flac_out.hip through ace355.audio_out.flac_encode_device and AudioSaver(flac_on_gpu=True)): the
bytes equal the host encoder's (ace355.audio_out.flac_encode_pcm16) exactly, on the inputs of tests/_flac_out_cases.py, whose coverage of
the encoder's choices tests/test_flac_out_cpu.py asserts on the host encoder.  Then the three readers, the saver end to end, the fallback and
the flag-off path.  There is no tolerance anywhere.  The host encoder's stream of each case is computed once (K.host_bytes)."""
import hashlib

import numpy as np
import pytest
import torch

import _flac_out_cases as K

pytestmark = pytest.mark.gpu

CASES = [(n, 48000) for n in K.ORIGINAL + K.ADDED + ("blocks129", "blocks2049_mono", "empty")] + [("rates", sr) for sr in K.RATES + (700001,)]


def _device(dev, name, sr=48000, md5=True):
    from ace355 import audio_out
    return audio_out.flac_encode_device(torch.from_numpy(K.pcm_of(name)).to(dev), sr, md5=md5)


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"{len(a)} bytes vs {len(b)}, first difference at byte {int(d[0]) if d.size else n}"


@pytest.mark.parametrize("name, sr", CASES, ids=[f"{n}-{sr}" for n, sr in CASES])
def test_bytes_equal_the_host_encoder(gpu_device, name, sr):
    got, = _device(gpu_device, name, sr)
    want = K.host_bytes(name, sr)
    assert got == want, _first_difference(got, want)


def test_batch_of_three(gpu_device):
    """Three items of different content in one call, twice: each item is its own host stream, and the two runs give the same bytes."""
    from ace355 import audio_out
    x = torch.from_numpy(np.stack([K.pcm_of(n) for n in K.BATCH3])).to(gpu_device)
    a = audio_out.flac_encode_device(x, 48000)
    b = audio_out.flac_encode_device(x, 48000)
    assert a == b and len(a) == 3
    for got, name in zip(a, K.BATCH3):
        assert got == K.host_bytes(name), name + ": " + _first_difference(got, K.host_bytes(name))


@pytest.mark.parametrize("name", K.ADDED + ("mono_sine", "tiny_tail", "blocks129"))
def test_without_md5_and_the_three_readers(gpu_device, name):
    """md5=False: the host's bytes but for 16 zero bytes in STREAMINFO.  The oracle reader, the native host decoder and the GPU decoder of
    csrc/flac_in.hip all return the PCM that went in, from the stream with the hash and from the one without."""
    from ace355 import audio_in, audio_out
    from oracle import audio_out as o_audio
    pcm, want = K.pcm_of(name), K.host_bytes(name)
    bare, = _device(gpu_device, name, md5=False)
    assert bare[:26] == want[:26] and bare[26:42] == bytes(16) and bare[42:] == want[42:]
    full, = _device(gpu_device, name)
    assert full[26:42] == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    for data in (full, bare):
        if pcm.shape[0] <= K.N:   # (the pure-Python reader takes seconds per 100k samples)
            got, info = o_audio.flac_decode(data)
            assert np.array_equal(got, pcm.astype(np.int64)) and info["frames"] == pcm.shape[0]
        got, sr = audio_out.flac_decode_pcm16(data)   # every CRC, and the MD5 where there is one
        assert sr == 48000 and np.array_equal(got, pcm)
        buf, pinfo, report = audio_in.decode_flac(data, gpu_device)   # both codecs on the device
        assert report["path"] == "gpu" and report["reason"] is None, report
        raw = np.frombuffer(buf.cpu().numpy().tobytes()[:2 * pinfo.channels * pinfo.frames], dtype="<i2").reshape(pinfo.frames, pinfo.channels)
        assert np.array_equal(raw, pcm)


def _wav_batch(dev):
    """[3, 2, S] float32 in [-1, 1]: what the saver quantises back to the three PCM items."""
    pcm = np.stack([K.pcm_of(n) for n in K.BATCH3]).astype(np.float32) / np.float32(32767.0)
    return torch.from_numpy(pcm).permute(0, 2, 1).contiguous().to(dev)


def test_saver_writes_the_same_files(gpu_device, tmp_path):
    from ace355 import audio_out
    wav = _wav_batch(gpu_device)
    names = lambda tag, ext: [tmp_path / f"{tag}_{i}.{ext}" for i in range(3)]  # noqa: E731
    off = audio_out.AudioSaver(flac_on_gpu=False)
    off.save_paths(wav, names("off", "flac"), 48000, "flac")
    assert off.last_flac_report["path"] == "host"
    want = [p.read_bytes() for p in names("off", "flac")]
    on = audio_out.AudioSaver(flac_on_gpu=True)
    on.save_paths(wav, names("on", "flac"), 48000, "flac")
    assert on.last_flac_report["path"] == "gpu" and on.last_flac_report["sizes"] == [len(w) for w in want], on.last_flac_report
    assert [p.read_bytes() for p in names("on", "flac")] == want
    bare = audio_out.AudioSaver(flac_on_gpu=True, flac_md5=False)
    bare.save_paths(wav, names("bare", "flac"), 48000, "flac")
    assert bare.last_flac_report["path"] == "gpu" and "left zero" in bare.last_flac_report["reason"]
    assert [p.read_bytes() for p in names("bare", "flac")] == [w[:26] + bytes(16) + w[42:] for w in want]
    # WAV ignores the flags, and leaves the FLAC report alone
    off.save_paths(wav, names("off", "wav"), 48000, "wav")
    on.last_flac_report = None
    on.save_paths(wav, names("on", "wav"), 48000, "wav")
    assert [p.read_bytes() for p in names("on", "wav")] == [p.read_bytes() for p in names("off", "wav")] and on.last_flac_report is None
    # a single item through save_audio, mono
    mono = wav[0, :1]
    assert on.save_audio(mono, tmp_path / "m_on.flac") and off.save_audio(mono, tmp_path / "m_off.flac")
    assert (tmp_path / "m_on.flac").read_bytes() == (tmp_path / "m_off.flac").read_bytes() and on.last_flac_report["path"] == "gpu"


def test_refused_request_is_encoded_by_the_host(gpu_device, tmp_path, monkeypatch):
    """A request the plan refuses yields the host's files and a report that says why.  The plan's own ceiling is 2^21 (item, block) pairs
    per call - 34 GB of float32 - so the test lowers it with ACE355_FLAC_OUT_MAX_UNITS, the saver's bound on its scratch, which the plan
    takes as its ceiling; the text reported is the plan's."""
    from ace355 import audio_out, native
    wav = _wav_batch(gpu_device)
    with pytest.raises(RuntimeError, match="n_items x blocks"):
        native.flac_out_plan(4096, 513 * 4096, 1)
    monkeypatch.setenv("ACE355_FLAC_OUT_MAX_UNITS", "8")   # 3 items x 3 blocks = 9 units
    on = audio_out.AudioSaver(flac_on_gpu=True)
    paths = [tmp_path / f"r_{i}.flac" for i in range(3)]
    on.save_paths(wav, paths, 48000, "flac")
    assert on.last_flac_report["path"] == "host" and "n_items x blocks" in on.last_flac_report["reason"], on.last_flac_report
    assert [p.read_bytes() for p in paths] == [K.host_bytes(n) for n in K.BATCH3]
    monkeypatch.setenv("ACE355_FLAC_OUT_MAX_UNITS", "9")
    on.save_paths(wav, paths, 48000, "flac")
    assert on.last_flac_report["path"] == "gpu" and [p.read_bytes() for p in paths] == [K.host_bytes(n) for n in K.BATCH3]


def test_flag_off_calls_no_new_entry_point(gpu_device, tmp_path, monkeypatch):
    from ace355 import audio_out, native
    real = native.lib()

    class Guard:
        def __getattr__(self, name):
            assert name not in ("ace355_save_audio_batch_ex", "ace355_flac_out_encode", "ace355_flac_out_plan", "ace355_flac_streaminfo"), name
            return getattr(real, name)
    monkeypatch.setattr(native, "_LIB", Guard())
    s = audio_out.AudioSaver(flac_on_gpu=False)
    p = tmp_path / "off.flac"
    s.save_paths(_wav_batch(gpu_device)[:1], [p], 48000, "flac")
    assert s.last_flac_report == {"path": "host", "reason": "flac_on_gpu is off", "sizes": None}
    assert p.read_bytes() == K.host_bytes(K.BATCH3[0])
