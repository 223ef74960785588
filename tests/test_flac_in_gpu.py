"""FLAC frames decoded on the GPU (csrc/flac_in.hip through ace355.audio_in.decode_flac): the decoded integers equal the oracle reader's
(oracle.audio_out.flac_decode) exactly on streams the test-side writer (tests/_flac_streams.py) makes for every subframe form at 16, 20
and 24 bits; then the loader end to end, the fallback ladder on a corrupted frame and on a false sync, and the handler seam.  There is
no tolerance anywhere.  Small streams: a few seconds in all, most of it the pure-Python writer and reader."""
import numpy as np
import pytest
import torch

import _flac_streams as S

pytestmark = pytest.mark.gpu

CRC16 = 5   # ACE355_FLAC_CRC16


def _ints(buf, info, bps):
    """The payload decode_flac returns, back as integers [frames, channels]."""
    raw = buf.cpu().numpy().tobytes()
    if info.format == "s16":
        assert bps == 16
        return np.frombuffer(raw[:2 * info.channels * info.frames], dtype="<i2").astype(np.int64).reshape(info.frames, info.channels)
    assert info.format == "s32" and bps > 16
    v = np.frombuffer(raw, dtype="<i4").astype(np.int64).reshape(info.frames, info.channels)
    assert not (v & ((1 << (32 - bps)) - 1)).any(), "left-justified"
    return v >> (32 - bps)


def _check(dev, name):
    from ace355 import audio_in
    data, rep, pcm, info = S.stream(name)
    buf, pinfo, report = audio_in.decode_flac(data, dev)
    assert report["path"] == "gpu" and report["reason"] is None and report["frames"] == len(rep["blocks"]), report
    assert (pinfo.channels, pinfo.sample_rate, pinfo.frames, pinfo.offset) == (info["channels"], info["sample_rate"], info["frames"], 0)
    assert buf.dtype == torch.uint8 and buf.numel() % 4 == 0
    got = _ints(buf, pinfo, info["bps"])
    assert np.array_equal(got, pcm), f"{name}: first difference at sample {int(np.argwhere(got != pcm)[0][0])}"
    return rep, pcm


# ---------------------------------------------------------------------------------------------------- exact decode
@pytest.mark.parametrize("name", S.ONE_FRAME)
def test_one_frame(gpu_device, name):
    """One frame of 16 samples, mono: each subframe kind in turn."""
    rep, _pcm = _check(gpu_device, name)
    assert rep["blocks"] == [16]


def test_wave_boundary(gpu_device):
    """70 frames of 192 stereo samples: past a 64-lane wave whatever the plan's lanes, the four channel assignments cycling."""
    rep, _pcm = _check(gpu_device, "wave_boundary")
    assert rep["blocks"] == [192] * 70


def test_many_frames(gpu_device):
    """2100 frames of 16 samples: more frames than wave slots (3 live lanes per wave), frame numbers coded in 1, 2 and 3 bytes; then the
    same samples with sample-number headers and blocks of 16 / 32 / 64."""
    from ace355 import native
    rep, pcm = _check(gpu_device, "many_frames")
    data = S.stream("many_frames")[0]
    assert len(rep["blocks"]) == 2100 and native.flac_in_plan(2100, 1, 16, 16, 33600)["entropy_lanes"] == 3
    assert [data[rep["offsets"][f] + 4] >> 4 for f in (127, 128, 2047, 2048)] == [0x7, 0xC, 0xD, 0xE]   # 1-, 2-, 2- and 3-byte numbers
    rep2, pcm2 = _check(gpu_device, "many_frames_variable")
    assert np.array_equal(pcm, pcm2) and rep2["blocks"][:3] == [16, 32, 64] and S.stream("many_frames_variable")[0][rep2["offsets"][0] + 1] == 0xF9


def test_block_size_codes(gpu_device):
    """The named sizes 192, 576, 1152, 4096 and 4608, and a last short block through the 8-bit and through the 16-bit header field."""
    rep, _pcm = _check(gpu_device, "block_codes")
    data = S.stream("block_codes")[0]
    assert [data[o + 2] >> 4 for o in rep["offsets"]] == [1, 2, 3, 12, 5, 6] and rep["blocks"][-1] == 100
    rep, _pcm = _check(gpu_device, "short_last_16bit_field")
    data = S.stream("short_last_16bit_field")[0]
    assert [data[o + 2] >> 4 for o in rep["offsets"]] == [12, 12, 7] and rep["blocks"][-1] == 1000


@pytest.mark.parametrize("name", ["fixed_orders", "lpc", "rice", "partitions", "wasted", "bps20"])
def test_subframe_forms(gpu_device, name):
    """fixed_orders: orders 0-4.  lpc: orders 1, 8, 12, 32; precision 15 with shift 0 and shift 14.  rice: k = 0, k = 14, Rice2 with
    k = 15 and 17.  partitions: order 0 and the largest a block allows, escaped partitions with 0 raw bits.  wasted: 1 and 7 bits.
    bps20: one 20-bit stream."""
    _check(gpu_device, name)


def test_escape_at_full_width(gpu_device):
    """24 bits, left/side: the side channel's escaped partition carries 25 raw bits, both extremes included."""
    _rep, pcm = _check(gpu_device, "escape_25_bits")
    side = pcm[:, 0] - pcm[:, 1]
    assert side.min() == -(1 << 24) + 1 and side.max() == (1 << 24) - 1


def test_24_bit_mid_side_needs_int64_sums(gpu_device):
    """Full-scale noise, mid/side, LPC order 32 at precision 15: the writer reports a prediction sum beyond 2^31 in magnitude, so an int32
    accumulator would not decode this."""
    rep, _pcm = _check(gpu_device, "ms24")
    assert rep["max_pred_sum"] > (1 << 31)


# ---------------------------------------------------------------------------------------------------- the loader
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", ["e2e_44k", "e2e_48k"])
def test_loader_16_bit_equals_the_host_path(gpu_device, name):
    from ace355 import audio_in
    data = S.stream(name)[0]
    want, want_peak = audio_in.load_stereo_48k(data, gpu_device)
    got, peak = audio_in.load_stereo_48k(data, gpu_device, flac_on_gpu=True)
    assert got.shape == want.shape and got.device == want.device and torch.equal(_bits(got), _bits(want)) and peak == want_peak and peak > 0.1


def test_loader_24_bit_equals_the_s24_wav_payload(gpu_device):
    """v << 8 as int32 over 2^31 and v as packed int24 over 2^23 are the same fp32 number, and the taps are the same: bit for bit."""
    from ace355 import audio_in
    data, _rep, pcm, info = S.stream("e2e24_44k")
    got, peak = audio_in.load_stereo_48k(data, gpu_device, flac_on_gpu=True)
    raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in pcm.reshape(-1))
    want, want_peak = audio_in.resample_payload(audio_in.upload(np.frombuffer(raw, dtype=np.uint8), gpu_device), 0, "s24", 2, len(pcm), info["sample_rate"])
    assert torch.equal(_bits(got), _bits(want)) and peak == float(want_peak.item()) and peak > 0.1
    with pytest.raises(NotImplementedError, match="24 bits per sample"):
        audio_in.load_stereo_48k(data, gpu_device)


# ---------------------------------------------------------------------------------------------------- the fallback ladder
def _flip(name, frame=1, byte=12):
    data, rep, pcm, _info = S.stream(name)
    bad = bytearray(data)
    bad[rep["offsets"][frame] + byte] ^= 0x10   # inside the first verbatim subframe: valid memory, same structure, another CRC-16
    return bytes(bad), rep, pcm


def test_corrupted_frame_16_bit(gpu_device):
    """One flipped bit inside frame 1: the device names the frame and the CRC code, its samples are zeros and every other frame's are the
    oracle's; the call then raises what the host decoder raises today."""
    from ace355 import audio_in
    bad, rep, pcm = _flip("verbatim16")
    with pytest.raises(RuntimeError, match="CRC-16") as host:
        audio_in.load_stereo_48k(bad, gpu_device)
    for call in (lambda: audio_in.decode_flac(bad, gpu_device), lambda: audio_in.load_stereo_48k(bad, gpu_device, flac_on_gpu=True)):
        with pytest.raises(RuntimeError, match="CRC-16") as exc:
            call()
        report = exc.value.flac_report
        assert str(exc.value) == str(host.value)
        assert report["path"] == "host" and report["frame"] == 1 and report["code"] == CRC16 and "frame 1: CRC-16 mismatch" in report["reason"], report
    buf, pinfo, report = audio_in.decode_flac(bad, gpu_device, sync=False)
    assert report["words"].cpu()[1:].tolist() == [1, CRC16]
    got, lo, hi = _ints(buf, pinfo, 16), rep["blocks"][0], rep["blocks"][0] + rep["blocks"][1]
    assert not got[lo:hi].any() and np.array_equal(got[:lo], pcm[:lo]) and np.array_equal(got[hi:], pcm[hi:])


def test_corrupted_frame_24_bit(gpu_device):
    """The same at 24 bits: there is no host decoder to fall back to, so the host path's NotImplementedError surfaces."""
    from ace355 import audio_in
    bad, _rep, _pcm = _flip("verbatim24")
    for call in (lambda: audio_in.decode_flac(bad, gpu_device), lambda: audio_in.load_stereo_48k(bad, gpu_device, flac_on_gpu=True)):
        with pytest.raises(NotImplementedError, match="24 bits per sample") as exc:
            call()
        report = exc.value.flac_report
        assert report["path"] == "host" and report["frame"] == 1 and report["code"] == CRC16, report


def test_fake_header_falls_back(gpu_device):
    """The index splits frame 1 at the header its verbatim subframe spells; the device rejects the piece, and the host decoder's samples
    come back."""
    from ace355 import audio_in
    data, _rep, pcm, _info = S.stream("fake_header")
    buf, pinfo, report = audio_in.decode_flac(data, gpu_device)
    assert report["path"] == "host" and report["frame"] == 1 and report["code"] != 0 and report["reason"].startswith("frame 1: "), report
    assert np.array_equal(_ints(buf, pinfo, 16), pcm)
    want, want_peak = audio_in.load_stereo_48k(data, gpu_device)
    got, peak = audio_in.load_stereo_48k(data, gpu_device, flac_on_gpu=True)
    assert torch.equal(_bits(got), _bits(want)) and peak == want_peak


def test_index_refusal_falls_back(gpu_device):
    """A stream the index refuses (here: a STREAMINFO max block it does not take) is the host decoder's, and the report says why."""
    from ace355 import audio_in
    x = np.arange(-24, 24, dtype=np.int64).reshape(48, 1) * 100
    data = S.write_stream([dict(samples=x[i:i + 16], subframes={"kind": "fixed", "order": 1}, bs_code=6) for i in (0, 16, 32)], 1, 16, max_block=32768)[0]
    buf, pinfo, report = audio_in.decode_flac(data, gpu_device)
    assert report["path"] == "host" and "max block 32768" in report["reason"] and report["frame"] is None
    assert np.array_equal(_ints(buf, pinfo, 16), x)


# ---------------------------------------------------------------------------------------------------- the handler seam
def test_handler(gpu_device, tmp_path):
    from ace355 import audio_in
    from ace355.backend import NativeHandler
    paths = {}
    for name in ("e2e_44k", "e2e24_44k"):
        paths[name] = str(tmp_path / f"{name}.flac")
        with open(paths[name], "wb") as f:
            f.write(S.stream(name)[0])
    h = NativeHandler()
    h.device, h.use_native_audio_in = str(gpu_device), True
    h.native_flac_decode = False
    want16 = h.process_src_audio(paths["e2e_44k"])
    assert h.process_src_audio(paths["e2e24_44k"]) is None    # as before: not read natively, and this handler has no host loader
    h.native_flac_decode = True
    got16, got24 = h.process_src_audio(paths["e2e_44k"]), h.process_src_audio(paths["e2e24_44k"])
    assert torch.equal(_bits(got16), _bits(want16))
    want24, _peak = audio_in.load_stereo_48k(paths["e2e24_44k"], gpu_device, flac_on_gpu=True)
    assert got24 is not None and got24.shape == want16.shape and got24.is_cuda and torch.equal(_bits(got24), _bits(want24))
    assert torch.equal(_bits(h.process_target_audio(paths["e2e24_44k"])), _bits(want24))
    h.use_native_audio_in = False                              # the switch only matters under use_native_audio_in
    with pytest.raises(RuntimeError, match="no audio input backend"):
        h.process_src_audio(paths["e2e24_44k"])
